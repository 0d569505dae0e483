"""bvh_scene_winding_prepare / bvh_scene_winding_number on the GPU: the prepared arrays bit for bit against bvh_winding_prepare on each BLAS and against the f32
restatements (tests/test_scene_winding.py scene_moments_host), the two-level walk against its restatement (scene_walk_host) and the f64 brute force over world
triangles, one identity instance against bvh_winding_number, inside / outside classification on instanced closed meshes, the stackless pass at both levels,
bvh_scene_update and BVH_SCENE_WINDING_KEEP_BLAS, buffer hygiene, errors and the Python binding."""
import ctypes as C

import numpy as np
import pytest

from test_deep_trees import stairs_steps
from test_gpu_query import caterpillar
from test_gpu_scene import Blases
from test_gpu_winding import TOL_FACTOR, TOL_FLOOR, prepare, winding, wmesh
from test_point_query import E_INVALID
from test_scene import identity, make_instances, mat34
from test_scene_point import flat_world_tris
from test_scene_winding import (KEEP_BLAS, scene_conditioning, scene_make_points, scene_moments_host, scene_walk_host, scene_winding_brute_force,
                                transform_kinds)
from test_winding import WIND_NAN_BITS, moments_host, stack_depth_all_open, tree_arrays

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32
N_POINTS = 1536
# the BLAS set of the mixed scenes: every mesh of the issue, all four builders (0, 1: layout 0; 2, 3: layout 1), all three triangle formats
BLAS_SET = [("uniform_2", 0, 0), ("uniform_3", 1, 1), ("uniform_64", 2, 2), ("uniform_65", 3, 0), ("uniform_1000", 1, 0), ("bunny_320", 3, 1), ("cornell32", 2, 0)]
SMALL = (0, 1, 2, 3, 6)                                             # (the instances beyond the first 14 place these: the references stay quick)
CASES = [(1, 3), (2, 0), (3, 1), (65, 2), (200, 3)]                 # (instances, top-level algo): every top-level builder


def builder_of(b):
    return b[0] if isinstance(b, tuple) else b


def input_of(b):
    return b[1] if isinstance(b, tuple) else None


def blas_trees(pkg, blases, meshes):
    """[(nodes, leaves, layout, root, tris)] as the restatements take them"""
    out = []
    for b, tris in zip(blases, meshes):
        t = builder_of(b).download()
        out.append((t["nodes"], t["leaves"], t["layout"], int(t["root"]), tris))
    return out


def download_top(pkg, ctx, scene):
    """(nodes, leaves, layout, root) of the scene's top-level tree, or None with one instance"""
    t = scene.tlas()
    n = int(t.n_leaves)
    if n < 2:
        return None
    nodes = np.empty(2 * n - 1 if t.layout == 0 else n - 1, dtype=pkg.BVH2_NODE)
    leaves = np.empty(n, dtype=pkg.PRIMREF) if t.layout == 1 else None
    assert pkg.lib().bvh_download(ctx.handle, C.byref(t), nodes.ctypes.data, leaves.ctypes.data if leaves is not None else None, None, None, None) == 0
    return nodes, leaves, int(t.layout), int(t.root)


def mixed_instances(pkg, rng, n_inst, n_blas, spacing=3.0):
    """identity, rotation x uniform scale, non-uniform scale + shear and a reflection in turn, on a jittered grid; with 3 or more instances the last is
    singular, with more than 3 the one before it names a BLAS out of range"""
    side = int(np.ceil(n_inst ** (1 / 3)))
    mats, blas = [], []
    for k in range(n_inst):
        t = np.array([k % side, (k // side) % side, k // (side * side)], dtype=np.float64) * spacing + rng.uniform(-0.2, 0.2, 3) * spacing
        mats.append(list(transform_kinds(rng, t).values())[k % 4])
        blas.append(k % n_blas if k < 2 * n_blas else SMALL[k % len(SMALL)] % n_blas)
    inst = make_instances(pkg, mats, blas)
    if n_inst >= 3:
        inst["object_to_world"][-1] = mat34(np.zeros((3, 3)), (1, 1, 1))
    if n_inst > 3:
        inst["blas"][-2] = n_blas + 5
    return inst


def check_arrays(pkg, scene, blases, trees, host, what):
    """check 1: the BLAS moments byte-equal to bvh_winding_prepare on that BLAS and to moments_host; maps, instance moments and top-level moments byte-equal to
    the restatement"""
    for b, (bl, tree) in enumerate(zip(blases, trees)):
        got = scene.winding_moments(b)
        assert got.tobytes() == host["blas"][b].tobytes(), f"{what}: BLAS {b} moments differ from moments_host"
        bd = builder_of(bl)
        flat = prepare(pkg, bd._ctx, bd.result, input_of(bl))
        try:
            assert got.tobytes() == flat.download(pkg.WINDING_MOMENT, len(got)).tobytes(), f"{what}: BLAS {b} moments differ from bvh_winding_prepare"
        finally:
            flat.free()
    imom, maps = scene.winding_instances()
    assert maps.tobytes() == host["maps"].tobytes(), f"{what}: maps differ on instances {np.nonzero((maps.view(np.uint32).reshape(len(maps), -1) != host['maps'].view(np.uint32).reshape(len(maps), -1)).any(axis=1))[0][:8]}"
    assert imom.tobytes() == host["inst"].tobytes(), f"{what}: instance moments differ on {np.nonzero((imom.view(np.uint32).reshape(len(imom), -1) != host['inst'].view(np.uint32).reshape(len(imom), -1)).any(axis=1))[0][:8]}"
    top = scene.winding_moments(None)
    assert len(top) == len(imom) - 1 and top.tobytes() == host["top"].tobytes(), f"{what}: top-level moments differ"


def check_walk(pkg, what, trees, inst, top, host, pts, dist, diag, bf, got, beta):
    """check 2, the flat test's rule and constants: on the well-conditioned points |w_gpu - scene_walk_host(f64)| <= 8 * max |walk(f32) - walk(f64)| (floor
    2^-20); at beta = +inf the same bound against the f64 brute force; NaN points answer the canonical NaN"""
    xyz = pts["point"]
    dead = np.isnan(xyz).any(axis=1)
    with np.errstate(invalid="ignore"):
        well = dist > 1e-4 * diag
    assert well.mean() >= 0.95, f"{what}: only {well.mean():.4f} of the points are well-conditioned"
    assert (got.view(np.uint32)[dead] == WIND_NAN_BITS).all(), f"{what}: a NaN point does not answer NaN"
    assert not np.isnan(got[~dead]).any(), f"{what}: NaN on a live point"
    w64 = scene_walk_host(pkg, trees, inst, top, host, xyz, beta, np.float64)
    w32 = scene_walk_host(pkg, trees, inst, top, host, xyz, beta, np.float32)
    tol = max(TOL_FACTOR * float(np.abs(w32[well].astype(np.float64) - w64[well]).max()), TOL_FLOOR)
    err = float(np.abs(got[well].astype(np.float64) - w64[well]).max())
    print(f"{what} beta {beta}: |gpu - host f64| max {err:.3e}, tol {tol:.3e}, |host f64 - brute| max {float(np.abs(w64[well] - bf[well]).max()):.3e}")
    assert err <= tol, f"{what} beta {beta}: {err:.3e} > {tol:.3e}"
    if np.isinf(beta):
        err = float(np.abs(got[well].astype(np.float64) - bf[well]).max())
        assert err <= tol, f"{what} beta inf against the brute force: {err:.3e} > {tol:.3e}"


@pytest.mark.parametrize("n_inst,tlas_algo", CASES)
def test_arrays_bitwise_and_walk_against_the_restatement(pkg, n_inst, tlas_algo):
    rng = np.random.default_rng(40 + n_inst)
    meshes = [wmesh(pkg, name) for name, _, _ in BLAS_SET]
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(algo, m, fmt=fmt) for (_, algo, fmt), m in zip(BLAS_SET, meshes)]
        assert {builder_of(b).result.layout for b in blases} == {0, 1}
        trees = blas_trees(pkg, blases, meshes)
        # (one instance: of uniform_1000; two: uniform_1000 and bunny_320)
        inst = mixed_instances(pkg, rng, n_inst, len(meshes))
        if n_inst <= 2:
            inst["blas"] = [4, 5][:n_inst]
        scene = pkg.Scene(sc_ctx).build(tlas_algo, blases, inst)
        sc_ctx.set_profiling(2)
        scene.winding_prepare()
        top = download_top(pkg, sc_ctx, scene)
        host = scene_moments_host(pkg, trees, inst, top)
        what = f"{n_inst} instances"
        check_arrays(pkg, scene, blases, trees, host, what)
        flat, _, _ = flat_world_tris(pkg, meshes, inst)
        pts = scene_make_points(pkg, flat, N_POINTS, 31 + n_inst)
        dist, diag = scene_conditioning(pkg, pts, flat)
        bf = scene_winding_brute_force(pkg, meshes, inst, pts["point"])
        for beta in (2.0, np.inf):
            got = scene.winding_number(pts, beta=beta)
            check_walk(pkg, what, trees, inst, top, host, pts, dist, diag, bf, got, beta)
        kt = sc_ctx.kernel_times()
        sc_ctx.set_profiling(0)
        assert {"k_scene_winding_climb", "k_scene_winding_finish", "k_scene_winding_inst", "k_scene_winding", "k_scene_winding_deep"} <= set(kt), sorted(kt)
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("name,algo,fmt", [("uniform_1000", 1, 0), ("bunny_320", 3, 1), ("cornell32", 2, 2)])
def test_one_identity_instance_against_the_flat_call(pkg, name, algo, fmt):
    """check 3: one identity instance opens the nodes bvh_winding_number opens on the BLAS and adds bit-equal terms, so the two GPU answers agree within the
    bound (they can differ by the order of the f64 sum only)"""
    tris = wmesh(pkg, name)
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        b = bl.add(algo, tris, fmt=fmt)
        bd, inp = builder_of(b), input_of(b)
        inst = make_instances(pkg, [identity()], [0])
        scene = pkg.Scene(sc_ctx).build(3, [b], inst).winding_prepare()
        trees = blas_trees(pkg, [b], [tris])
        host = scene_moments_host(pkg, trees, inst)
        pts = scene_make_points(pkg, tris, N_POINTS, 7 + len(tris))
        dist, diag = scene_conditioning(pkg, pts, tris)
        with np.errstate(invalid="ignore"):
            well = dist > 1e-4 * diag
        assert well.mean() >= 0.95
        mom = prepare(pkg, bd._ctx, bd.result, inp)
        try:
            assert scene.winding_moments(0).tobytes() == mom.download(pkg.WINDING_MOMENT, len(tris) - 1).tobytes()
            for beta in (2.0, np.inf):
                got = scene.winding_number(pts, beta=beta)
                ref = winding(pkg, bd._ctx, bd.result, mom, pts, beta, inp)
                w64 = scene_walk_host(pkg, trees, inst, None, host, pts["point"], beta, np.float64)
                w32 = scene_walk_host(pkg, trees, inst, None, host, pts["point"], beta, np.float32)
                tol = max(TOL_FACTOR * float(np.abs(w32[well].astype(np.float64) - w64[well]).max()), TOL_FLOOR)
                err = float(np.abs(got[well].astype(np.float64) - ref[well]).max())
                print(f"{name} beta {beta}: |scene - flat| max {err:.3e}, tol {tol:.3e}, bytes equal: {got.tobytes() == ref.tobytes()}")
                assert err <= tol and np.array_equal(np.isnan(got), np.isnan(ref))
        finally:
            mom.free()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_classification_on_instanced_closed_meshes(pkg):
    """check 4, with test_classification_on_a_closed_mesh's thresholds: at beta 2, w > 0.5 is the brute force's answer on every point farther than 1e-3 of the
    diagonal from the world surface; the bodies are apart, so the exact value is 0 or 1 (-1 inside the reflected one)"""
    tris = wmesh(pkg, "bunny_320")
    rng = np.random.default_rng(17)
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(algo, tris, fmt=algo % 3) for algo in range(4)]
        kinds = ["identity", "similarity", "shear", "similarity", "identity", "shear", "similarity", "mirror"]
        mats = [transform_kinds(rng, np.array([k % 2, (k // 2) % 2, k // 4], dtype=np.float64) * 14.0)[kind] for k, kind in enumerate(kinds)]
        inst = make_instances(pkg, mats, np.arange(len(mats)) % 4)
        flat, _, _ = flat_world_tris(pkg, [tris] * 4, inst)
        pts = scene_make_points(pkg, flat, N_POINTS, 3)
        dist, diag = scene_conditioning(pkg, pts, flat)
        bf = scene_winding_brute_force(pkg, [tris] * 4, inst, pts["point"])
        with np.errstate(invalid="ignore"):
            clear = dist > 1e-3 * diag
        assert clear.mean() >= 0.9 and 0.02 < (bf[clear] > 0.5).mean() < 0.98
        assert (np.abs(bf[clear] - np.rint(bf[clear])) <= 1e-6).all() and set(np.rint(bf[clear]).astype(int).tolist()) <= {-1, 0, 1}
        for tl in range(4):
            got = pkg.Scene(sc_ctx).build(tl, blases, inst).winding_number(pts, beta=2.0)
            print(f"top-level algo {tl}: max |gpu - brute| {float(np.abs(got[clear] - bf[clear]).max()):.4f}, min |w - 0.5| {float(np.abs(got[clear] - 0.5).min()):.4f}")
            assert ((got > 0.5) == (bf > 0.5))[clear].all(), f"top-level algo {tl}: {np.count_nonzero(((got > 0.5) != (bf > 0.5)) & clear)} points misclassified"
    finally:
        bl.close(); sc_ctx.close()


def top_stack_need_all_open(top, n_inst, active, blas_need):
    """the deepest short stack of k_scene_winding when everything is opened (beta = +inf): at a top-level node whose two children are both opened (an internal
    node, or a leaf with an active instance) the left is entered and the right pushed; inside an instance its BLAS's own pushes come on top"""
    nodes, leaves, layout, root = top
    _, tni, prims = tree_arrays(nodes, leaves, layout)
    opened = lambda c: c < tni or (c < 2 * n_inst - 1 and prims[c - tni] < n_inst and active[prims[c - tni]])
    best, work = 0, [(int(root), 0)]
    while work:
        v, d = work.pop()
        if v >= tni:
            best = max(best, d + blas_need)
            continue
        l, r = int(nodes["left"][v]), int(nodes["right"][v])
        if opened(l) and opened(r):
            work.append((l, d + 1)); work.append((r, d))
        else:
            for ch in (l, r):
                if opened(ch):
                    work.append((ch, d))
    return best


def test_deep_blas_takes_the_stackless_pass(pkg):
    """check 5a: a caterpillar BLAS deeper than the 64-entry stack under five instances.  At beta = +inf every query opens every node of every instance, so every
    live query overflows and is finished by k_scene_winding_deep; at beta 2 the far side nodes are approximated and the short stack suffices"""
    H = 250
    tris, nodes, root, n = caterpillar(pkg, H, 7 + H)
    assert stack_depth_all_open(nodes, root, n - 1) > 64
    c = pkg.Context(0)
    sc_ctx = pkg.Context(0)
    try:
        d_nodes, d_tris = c.upload(nodes), c.upload(tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        rng = np.random.default_rng(H)
        offs = np.array([(0, 0, 0), (100, 0, 0), (0, 100, 0), (100, 100, 0), (200, 50, 0)], dtype=np.float64)
        mats = [mat34(np.eye(3), offs[0])] + [list(transform_kinds(rng, offs[k]).values())[k % 4] for k in range(1, 5)]
        inst = make_instances(pkg, mats, [0] * 5)
        scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst).winding_prepare()
        trees = [(nodes, None, 0, root, tris)]
        top = download_top(pkg, sc_ctx, scene)
        host = scene_moments_host(pkg, trees, inst, top)
        assert scene.winding_moments(0).tobytes() == host["blas"][0].tobytes() and scene.winding_moments(None).tobytes() == host["top"].tobytes()
        flat, _, _ = flat_world_tris(pkg, [tris], inst)
        pts = scene_make_points(pkg, flat, 300, 5)
        dist, diag = scene_conditioning(pkg, pts, flat)
        bf = scene_winding_brute_force(pkg, [tris], inst, pts["point"])
        for beta in (2.0, np.inf):
            got = scene.winding_number(pts, beta=beta)
            check_walk(pkg, f"caterpillar {H}", trees, inst, top, host, pts, dist, diag, bf, got, beta)
        scene.close(); d_nodes.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()


def stairs_instances(pkg, L=65, q=2.2, s=5e-11):
    """the deep top-level scene of tests/test_deep_trees.py tlas_scene — 2L instances of one mesh, uniform scale 0.05 p at base, p growing by q per step, so
    that the pairs chain up — over the range of scales f32 solid angles allow (a product of three lengths must stay finite): 5e-11 to 4e11"""
    p, base = stairs_steps(L, q, s)
    return make_instances(pkg, [mat34(np.eye(3) * (0.05 * p[k]), base[k]) for k in range(len(p))], [0] * len(p)), p, base


@pytest.mark.parametrize("tlas_algo", [2, 3])
def test_deep_top_level_tree_takes_the_stackless_pass(pkg, tlas_algo):
    """check 5b: the staircase scene the other scene tests overflow the top level with, over a BLAS (a caterpillar of height 40 in the unit cube) that fits the
    64-entry stack on its own.  At beta = +inf everything is opened, left child first, so the stack need is a property of the downloaded trees alone: the test
    asserts that the top level's entries plus the BLAS's exceed the stack while the BLAS's alone do not"""
    tris, nodes, root, n = caterpillar(pkg, 40, 11)
    shrink = F32(1.0 / 1100.0)                                      # (monotone: the scaled boxes still hold the scaled triangles)
    tris = tris.copy(); nodes = nodes.copy()
    for f in ("v1", "v2", "v3"):
        tris[f] = tris[f] * shrink
    nodes["min"] = nodes["min"] * shrink; nodes["max"] = nodes["max"] * shrink
    blas_need = stack_depth_all_open(nodes, root, n - 1)
    inst, p, base = stairs_instances(pkg)
    c = pkg.Context(0)
    sc_ctx = pkg.Context(0)
    try:
        d_nodes, d_tris = c.upload(nodes), c.upload(tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        scene = pkg.Scene(sc_ctx).build(tlas_algo, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst).winding_prepare()
        trees = [(nodes, None, 0, root, tris)]
        top = download_top(pkg, sc_ctx, scene)
        host = scene_moments_host(pkg, trees, inst, top)
        need = top_stack_need_all_open(top, len(inst), host["active"], blas_need)
        print(f"top-level algo {tlas_algo}: stack need with everything opened {need}, of which the BLAS {blas_need}")
        assert blas_need <= 64 < need
        assert scene.winding_moments(0).tobytes() == host["blas"][0].tobytes() and scene.winding_moments(None).tobytes() == host["top"].tobytes()
        # points in and around random instances, at each instance's own scale (the scene spans 22 orders of magnitude)
        rng = np.random.default_rng(tlas_algo)
        m = 512
        k = rng.integers(0, len(inst), m)
        pts = np.zeros(m, dtype=pkg.POINT_QUERY)
        pts["point"] = (base[k] + 0.05 * p[k][:, None] * rng.uniform(-1.0, 2.0, (m, 3))).astype(F32)
        pts["radius"] = np.inf
        for j, cidx in enumerate(range(m - 8, m)):
            pts["point"][cidx, j % 3] = np.nan
        flat, _, _ = flat_world_tris(pkg, [tris], inst)
        dist, _ = scene_conditioning(pkg, pts, flat)
        dist = dist / (0.05 * p[k])                                # conditioning at the scale of the instance the point is aimed at
        bf = scene_winding_brute_force(pkg, [tris], inst, pts["point"])
        for beta in (2.0, np.inf):
            got = scene.winding_number(pts, beta=beta)
            check_walk(pkg, f"stairs algo {tlas_algo}", trees, inst, top, host, pts, dist, 1.0, bf, got, beta)
        scene.close(); d_nodes.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()


def test_update_and_keep_blas(pkg):
    """check 6: after bvh_scene_update the query is refused until a prepare; a prepare with BVH_SCENE_WINDING_KEEP_BLAS then gives the arrays and answers of a
    full prepare byte for byte"""
    rng = np.random.default_rng(21)
    meshes = [wmesh(pkg, "uniform_65"), wmesh(pkg, "bunny_320")]
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    L = pkg.lib()
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        inst = mixed_instances(pkg, rng, 20, 2)
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        moved = mixed_instances(pkg, np.random.default_rng(22), 20, 2, spacing=3.5)
        moved["blas"][:4] = 1 - moved["blas"][:4]
        flat, _, _ = flat_world_tris(pkg, meshes, moved)
        pts = scene_make_points(pkg, flat, 512, 23)
        d_pts = sc_ctx.upload(pts)
        sent = np.full(512 * 4, 0x5A, dtype=np.uint8)
        d_w = sc_ctx.upload(sent)
        call = lambda: L.bvh_scene_winding_number(scene.handle, d_pts.ptr, 512, 2.0, d_w.ptr)
        p, n = C.c_void_p(), C.c_uint32()
        assert call() == E_INVALID                                  # never prepared
        assert L.bvh_scene_winding_prepare(scene.handle, KEEP_BLAS) == 0 and call() == 0      # (nothing to keep yet: a full prepare)
        d_w.upload(sent)
        assert L.bvh_scene_update(scene.handle, moved.ctypes.data, 0, None) == 0
        assert call() == E_INVALID                                  # stale
        assert L.bvh_scene_winding_moments(scene.handle, pkg.INVALID, C.byref(p), C.byref(n)) == E_INVALID
        assert L.bvh_scene_winding_instances(scene.handle, C.byref(p), C.byref(p)) == E_INVALID
        assert L.bvh_scene_winding_moments(scene.handle, 0, C.byref(p), C.byref(n)) == 0 and n.value == len(meshes[0]) - 1      # the BLAS part is not stale
        sc_ctx.synchronize()
        assert d_w.download(np.uint8, len(sent)).tobytes() == sent.tobytes()
        scene._winding_ready = False
        scene.winding_prepare(keep_blas=True)
        kept = (scene.winding_number(pts), scene.winding_moments(0), scene.winding_moments(1), scene.winding_moments(None)) + scene.winding_instances()
        scene.winding_prepare(keep_blas=False)
        full = (scene.winding_number(pts), scene.winding_moments(0), scene.winding_moments(1), scene.winding_moments(None)) + scene.winding_instances()
        for a, b in zip(kept, full):
            assert a.tobytes() == b.tobytes()
        # ... and they are the restatement's on the moved instances and the refit top-level tree (its topology is the build's, so a fresh build may answer otherwise)
        trees = blas_trees(pkg, blases, meshes)
        top = download_top(pkg, sc_ctx, scene)
        host = scene_moments_host(pkg, trees, moved, top)
        assert full[3].tobytes() == host["top"].tobytes() and full[4].tobytes() == host["inst"].tobytes() and full[5].tobytes() == host["maps"].tobytes()
        dist, diag = scene_conditioning(pkg, pts, flat)
        check_walk(pkg, "after update", trees, moved, top, host, pts, dist, diag, scene_winding_brute_force(pkg, meshes, moved, pts["point"]), full[0], 2.0)
        # a new build discards everything
        scene.build(3, blases, inst)
        assert call() == E_INVALID and L.bvh_scene_winding_moments(scene.handle, 0, C.byref(p), C.byref(n)) == E_INVALID
        scene.close(); d_pts.free(); d_w.free()
    finally:
        bl.close(); sc_ctx.close()


def test_buffers_untouched_and_errors_write_nothing(pkg):
    """checks 7 and 8"""
    tris = wmesh(pkg, "uniform_1000")
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    L = pkg.lib()
    try:
        b = bl.add(3, tris)
        inst = make_instances(pkg, [identity(), mat34(np.diag([1.0, 2.0, 0.5]), (2.0, 0, 0))], [0, 0])
        flat, _, _ = flat_world_tris(pkg, [tris], inst)
        pts = scene_make_points(pkg, flat, 700, 4)
        m = len(pts)
        guard = 64
        sent = np.full(2 * guard + m * 4, 0x5A, dtype=np.uint8)
        d_w, d_pts = sc_ctx.upload(sent), sc_ctx.upload(pts)
        w = d_w.ptr + guard
        scene = pkg.Scene(sc_ctx)
        assert L.bvh_scene_winding_prepare(scene.handle, 0) == E_INVALID                                   # not built
        assert L.bvh_scene_winding_number(scene.handle, d_pts.ptr, m, 2.0, w) == E_INVALID
        scene.build(2, [b], inst)
        assert L.bvh_scene_winding_number(scene.handle, d_pts.ptr, m, 2.0, w) == E_INVALID                 # moments missing
        assert L.bvh_scene_winding_prepare(scene.handle, 2) == E_INVALID and L.bvh_scene_winding_prepare(scene.handle, 0xFFFFFFFE) == E_INVALID
        assert L.bvh_scene_winding_number(scene.handle, d_pts.ptr, m, 2.0, w) == E_INVALID                 # (a refused prepare prepared nothing)
        assert L.bvh_scene_winding_prepare(scene.handle, 0) == 0
        cases = {
            "null scene": L.bvh_scene_winding_number(None, d_pts.ptr, m, 2.0, w), "null points": L.bvh_scene_winding_number(scene.handle, None, m, 2.0, w),
            "null w": L.bvh_scene_winding_number(scene.handle, d_pts.ptr, m, 2.0, None), "beta -1": L.bvh_scene_winding_number(scene.handle, d_pts.ptr, m, -1.0, w),
            "beta -inf": L.bvh_scene_winding_number(scene.handle, d_pts.ptr, m, -np.inf, w), "beta nan": L.bvh_scene_winding_number(scene.handle, d_pts.ptr, m, np.nan, w),
            "w over the points": L.bvh_scene_winding_number(scene.handle, d_pts.ptr, m, 2.0, d_pts.ptr + 16),
            "points over w": L.bvh_scene_winding_number(scene.handle, w + 4 * (m - 1), m, 2.0, w),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        p, n = C.c_void_p(), C.c_uint32()
        assert L.bvh_scene_winding_moments(scene.handle, 1, C.byref(p), C.byref(n)) == E_INVALID           # no such BLAS
        assert L.bvh_scene_winding_moments(scene.handle, 0, None, C.byref(n)) == E_INVALID
        assert L.bvh_scene_winding_instances(scene.handle, None, None) == E_INVALID
        assert L.bvh_scene_winding_number(scene.handle, d_pts.ptr, 0, 2.0, w) == 0                          # n_points == 0: nothing is touched
        sc_ctx.synchronize()
        assert d_w.download(np.uint8, len(sent)).tobytes() == sent.tobytes(), "an error or n_points == 0 wrote to the answers"
        runs = []
        for _ in range(2):
            d_w.upload(sent)
            assert L.bvh_scene_winding_number(scene.handle, d_pts.ptr, m, 2.0, w) == 0
            out = d_w.download(np.uint8, len(sent))
            assert (out[:guard] == 0x5A).all() and (out[-guard:] == 0x5A).all()
            runs.append(out[guard:-guard].tobytes())
        assert runs[0] == runs[1]                                   # two calls on the same arrays: the same bytes
        got = np.frombuffer(runs[0], dtype=np.float32)
        dead = np.isnan(pts["point"]).any(axis=1)
        assert dead.sum() == 8 and (got.view(np.uint32)[dead] == WIND_NAN_BITS).all() and not np.isnan(got[~dead]).any()
        assert d_pts.download(pkg.POINT_QUERY, m).tobytes() == pts.tobytes()
        assert got.tobytes() == scene.winding_number(pts).tobytes()
        scene.close(); d_w.free(); d_pts.free()
    finally:
        bl.close(); sc_ctx.close()


def test_python_binding_and_signed_distance(pkg):
    """check 9"""
    tris = wmesh(pkg, "bunny_320")
    rng = np.random.default_rng(9)
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        b = bl.add(3, tris)
        mats = [transform_kinds(rng, np.array([k * 12.0, 0.0, 0.0]))[kind] for k, kind in enumerate(["identity", "similarity", "shear"])]
        inst = make_instances(pkg, mats, [0, 0, 0])
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        flat, _, _ = flat_world_tris(pkg, [tris], inst)
        pts = scene_make_points(pkg, flat, 1024, 2)[:-8]
        xyz = np.ascontiguousarray(pts["point"])
        w = scene.winding_number(xyz)                               # prepares on first use
        assert w.dtype == np.float32 and w.shape == (len(xyz),) and scene._winding_ready
        assert scene.winding_number(pts).tobytes() == w.tobytes()
        d = sc_ctx.upload(pts)
        assert scene.winding_number(d).tobytes() == w.tobytes() and scene.winding_number(d.ptr, n_points=len(pts)).tobytes() == w.tobytes()
        d.free()
        assert scene.winding_number(pts, beta=3.0).tobytes() != w.tobytes()
        assert scene.winding_number(np.zeros((0, 3), dtype=F32)).shape == (0,)
        sd, hits = scene.signed_distance(xyz)
        cp = scene.closest_point(xyz)
        assert hits.dtype == pkg.INSTANCE_POINT_HIT and hits.tobytes() == cp.tobytes()
        with np.errstate(invalid="ignore"):
            want = np.where(w > F32(0.5), -np.sqrt(cp["dist2"]), np.sqrt(cp["dist2"])).astype(F32)
        assert sd.tobytes() == want.tobytes() and (sd < 0).any() and (sd > 0).any()
        bf = scene_winding_brute_force(pkg, [tris], inst, xyz)
        dist, diag = scene_conditioning(pkg, pts, flat)
        clear = dist > 1e-3 * diag
        assert ((sd < 0) == (bf > 0.5))[clear].all()                # negative exactly inside the bodies
        assert scene.signed_distance(pts)[0].tobytes() == sd.tobytes()
        # after an update the binding prepares again
        moved = inst.copy(); moved["object_to_world"][1][3] += 1.0
        scene.update(moved)
        assert not scene._winding_ready
        w2 = scene.winding_number(xyz)
        assert scene._winding_ready and w2.tobytes() != w.tobytes()
        assert scene.winding_prepare().winding_number(xyz).tobytes() == w2.tobytes()                    # (what an explicit full prepare gives)
        imom, maps = scene.winding_instances()
        assert imom.dtype == pkg.WINDING_MOMENT and maps.dtype == pkg.WINDING_MAP and len(imom) == len(maps) == 3
        scene.close()
    finally:
        bl.close(); sc_ctx.close()
