"""bvh_scene_closest_point on the GPU: closest and any-within-radius answers against the two-level numpy brute force (tests/test_scene_point.py) for 1 to 64
instances over BLASes of every builder and triangle format, anisotropic / sheared and far-offset instances (where a walk that measures in object space goes
wrong), one identity instance against bvh_closest_point, independence from the builders, deep BLASes through the stackless pass, bvh_scene_update after moves
and after a BLAS refit, coincident instances, rejections and buffer hygiene."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_point_query import first_descent_pushes, make_points
from test_gpu_query import caterpillar
from test_gpu_refit import jitter, no_negzero
from test_gpu_scene import MESH_SIZES, TLAS_ALGO, Blases, root_boxes, scene_instances, world_tris
from test_query import E_INVALID
from test_scene import identity, make_instances, mat34
from test_scene_point import instance_set, near_surface_points, scene_below, scene_point_brute_force, scene_point_recompute, scene_points, shear_matrix

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32


def with_shear(pkg, rng, inst, n_active):
    """every sixth of the first n_active instances becomes rotation x diag(0.25 .. 4) x shear x rotation at its own translation: the sixth kind"""
    for k in range(5, n_active, 6):
        inst["object_to_world"][k] = mat34(shear_matrix(rng), inst["object_to_world"][k].reshape(3, 4)[:, 3])
    return inst


def check_exact(pkg, pts, blas_tris, inst, bf, closest, anyhit, what):
    well = bf["well"]
    print(f"{what}: {well.sum()} of {len(well)} well-conditioned, {bf['hit'].sum()} hits")
    assert well.mean() >= 0.99, f"{what}: only {well.mean():.4f} of the queries are well-conditioned"
    ref = bf["closest"]
    for f in ("point", "dist2", "u", "v"):
        eq = (closest[f].view(np.uint32) == ref[f].view(np.uint32)).reshape(len(pts), -1).all(axis=1)
        assert eq[well].all(), f"{what}: closest {f} differs on {np.count_nonzero(~eq & well)} well-conditioned queries (first {np.nonzero(~eq & well)[0][:6]})"
    for f in ("prim", "instance"):
        assert (closest[f] == ref[f])[well].all(), f"{what}: closest {f} differs on {np.count_nonzero((closest[f] != ref[f]) & well)} well-conditioned queries"
    assert scene_point_recompute(pkg, pts, blas_tris, inst, closest).all(), f"{what}: a closest record is not an accepted candidate (or not the miss record)"
    assert scene_point_recompute(pkg, pts, blas_tris, inst, anyhit).all(), f"{what}: an any record is not an accepted candidate (or not the miss record)"
    assert not scene_below(pkg, closest, ref).any(), f"{what}: closest below the brute force"
    assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"])[well].all(), f"{what}: any-hit hit / miss differs"


@pytest.mark.parametrize("n_inst", [1, 2, 3, 64])
def test_exact_against_brute_force(pkg, n_inst):
    rng = np.random.default_rng(n_inst)
    meshes = [no_negzero(pkg.meshgen.uniform(n, 31 + n)) for n in MESH_SIZES[n_inst]]
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo], fmt=algo % 3) for algo in range(4)]
        inst = scene_instances(pkg, rng, n_inst, 4, 1.5)
        inactive = ({n_inst - 1, n_inst - 2, n_inst - 3} if n_inst > 3 else {n_inst - 1}) if n_inst >= 3 else set()
        inst = with_shear(pkg, rng, inst, n_inst - len(inactive))
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[n_inst], blases, inst)
        pts = scene_points(pkg, world_tris(pkg, meshes, inst), 1024, 100 + n_inst)
        bf = scene_point_brute_force(pkg, pts, meshes, inst, root_boxes(pkg, blases))
        assert bf["hit"].sum() > len(pts) // 2 and (~bf["hit"]).sum() > 20
        closest, anyhit = scene.closest_point(pts, query="closest"), scene.closest_point(pts, query="any")
        check_exact(pkg, pts, meshes, inst, bf, closest, anyhit, f"{n_inst} instances")
        for out in (closest, anyhit):
            assert not set(out["instance"][out["prim"] != pkg.INVALID].tolist()) & inactive, "an inactive instance answered"
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("kind", ["shear", "far"])
def test_anisotropic_and_far_offset_instances(pkg, kind):
    """every instance is rotation x diag(0.25 .. 4) x shear x rotation ("shear": object-space distances are off by up to 16x either way), or rigid with
    translations up to 4096 ("far": the mapped point carries an absolute error that dwarfs a near-surface distance)"""
    rng = np.random.default_rng(7 if kind == "shear" else 8)
    mesh = no_negzero(pkg.meshgen.uniform(300, 41))
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        inst = instance_set(pkg, rng, kind, 8)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        pts = scene_points(pkg, world_tris(pkg, [mesh], inst), 1024, 9, bounded=False)
        bf = scene_point_brute_force(pkg, pts, [mesh], inst, root_boxes(pkg, [b]))
        assert bf["hit"].all()
        check_exact(pkg, pts, [mesh], inst, bf, scene.closest_point(pts, query="closest"), scene.closest_point(pts, query="any"), kind)
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("algo", [1, 3])
def test_one_identity_instance_equals_closest_point(pkg, algo):
    mesh = no_negzero(pkg.meshgen.sponza_like(20_000, 3))
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        b = bl.add(algo, mesh)
        assert b.result.layout == (0 if algo == 1 else 1)
        pts = make_points(pkg, mesh, 4096, 8)
        ref = b.closest_point(pts, query="closest")
        scene = pkg.Scene(sc_ctx).build(3, [b], make_instances(pkg, [identity()], [0]))
        got = scene.closest_point(pts, query="closest")
        for f in ("dist2", "prim"):
            bad = np.nonzero(got[f].view(np.uint32) != ref[f].view(np.uint32))[0]
            assert bad.size == 0, f"{f} differs on {bad.size} queries, e.g. {bad[:4]}: scene {got[bad[:4]]} closest_point {ref[bad[:4]]} points {pts[bad[:4]]}"
        for f in ("point", "u", "v"):
            assert np.array_equal(got[f], ref[f]), f
        hit = ref["prim"] != pkg.INVALID
        assert hit.sum() > 500 and (~hit).sum() > 50 and (got["instance"][hit] == 0).all() and (got["instance"][~hit] == pkg.INVALID).all()
        # the binding takes what the builders' closest_point takes: plain (n, 3) points with a radius, and device records
        xyz = np.ascontiguousarray(pts["point"][:256])
        rec = np.zeros(256, dtype=pkg.POINT_QUERY); rec["point"] = xyz; rec["radius"] = 0.5
        want = scene.closest_point(rec).tobytes()
        assert scene.closest_point(xyz, radius=0.5).tobytes() == want
        d = sc_ctx.upload(rec)
        assert scene.closest_point(d).tobytes() == want and scene.closest_point(d.ptr, n_points=256).tobytes() == want
        d.free()
        with pytest.raises(pkg.BvhError):
            scene.closest_point(rec, radius=1.0)
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_independent_of_builders(pkg):
    rng = np.random.default_rng(9)
    mesh = no_negzero(pkg.meshgen.uniform(200, 77))
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(algo, mesh) for algo in range(4)]
        inst = with_shear(pkg, rng, scene_instances(pkg, rng, 64, 1, 1.2), 61)
        pts = scene_points(pkg, world_tris(pkg, [mesh], inst), 1024, 5)
        bf = scene_point_brute_force(pkg, pts, [mesh], inst, root_boxes(pkg, blases[:1]))
        assert bf["well"].all() and bf["hit"].sum() > 500
        outs = []
        for tl in range(4):                                   # top-level builders over the same BLAS
            outs.append(pkg.Scene(sc_ctx).build(tl, [blases[3]], inst).closest_point(pts, query="closest"))
        for b in range(3):                                    # BLAS builders of the same mesh
            outs.append(pkg.Scene(sc_ctx).build(3, [blases[b]], inst).closest_point(pts, query="closest"))
        assert outs[0].tobytes() == bf["closest"].tobytes()
        for o in outs[1:]:
            assert o.tobytes() == outs[0].tobytes()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("H", [70, 250])
def test_deep_blas_takes_the_stackless_pass(pkg, H):
    tris, nodes, root, n = caterpillar(pkg, H, 3 + H)
    c = pkg.Context(0)
    sc_ctx = pkg.Context(0)
    try:
        d_nodes, d_tris = c.upload(nodes), c.upload(tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        offs = np.array([(0, 0, 0), (100, 0, 0), (0, 100, 0), (100, 100, 0), (200, 50, 0)], dtype=np.float64)
        inst = make_instances(pkg, [mat34(np.eye(3), t) for t in offs], [0] * len(offs))
        scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
        rng = np.random.default_rng(H)
        m = 500
        pts = np.zeros(m, dtype=pkg.POINT_QUERY)
        base = offs[rng.integers(0, len(offs), m)]
        pts["point"] = np.stack([base[:, 0] + rng.uniform(-1, 1, m), base[:, 1] + rng.uniform(-1, 1, m), rng.uniform(-3, -0.5, m)], axis=1)
        pts["point"][: m // 6, 2] = 0.0                           # on the face at z = 0
        pts["radius"] = np.inf
        pts["radius"][m // 2: 3 * m // 4] = 5.0                   # the far side nodes are culled: no push, the short stack suffices
        pts["point"][3 * m // 4:, 2] = rng.uniform(1000, 1000 + 2 * H, m - 3 * m // 4)     # among the far triangles
        # an unbounded query passes every box until its first candidate, so whichever instance it enters first its first descent there pushes one entry per
        # chain node: more than the short stack holds
        pushes = [min(first_descent_pushes(nodes, root, n - 1, pts["point"][j].astype(np.float64) - t) for t in offs) for j in range(m // 2)]
        assert max(pushes) > 64
        bf = scene_point_brute_force(pkg, pts, [tris], inst)
        assert bf["well"].all() and bf["hit"].all()
        sc_ctx.set_profiling(2)
        closest, anyhit = scene.closest_point(pts, query="closest"), scene.closest_point(pts, query="any")
        kt = sc_ctx.kernel_times()
        sc_ctx.set_profiling(0)
        assert {"k_scene_closest_point", "k_scene_closest_point_deep"} <= set(kt)
        assert closest.tobytes() == bf["closest"].tobytes()
        assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"]).all() and scene_point_recompute(pkg, pts, [tris], inst, anyhit).all()
        scene.close(); d_nodes.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()


def test_update_after_moves_and_blas_refit(pkg):
    rng = np.random.default_rng(21)
    meshes = [no_negzero(pkg.meshgen.uniform(n, 5 + n)) for n in (150, 120)]
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        inst = scene_instances(pkg, rng, 64, 2, 1.5)
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        rng2 = np.random.default_rng(22)
        moved = with_shear(pkg, rng2, scene_instances(pkg, rng2, 64, 2, 1.7), 61)      # (the matrices change kind too: s2 is refreshed by the update)
        moved["blas"][:8] = 1 - np.minimum(moved["blas"][:8], 1)
        scene.update(moved)
        pts = scene_points(pkg, world_tris(pkg, meshes, moved), 1024, 23)
        bf = scene_point_brute_force(pkg, pts, meshes, moved, root_boxes(pkg, blases))
        closest, anyhit = scene.closest_point(pts, query="closest"), scene.closest_point(pts, query="any")
        check_exact(pkg, pts, meshes, moved, bf, closest, anyhit, "after update")
        fresh = pkg.Scene(sc_ctx).build(3, blases, moved).closest_point(pts, query="closest")
        assert fresh.tobytes() == closest.tobytes()
        m0 = jitter(meshes[0], 3, 2e-2)
        blases[0].refit(m0)
        bl.ctxs[0].synchronize()                              # (the refit ran on the BLAS's own stream: complete before the scene reads the root box)
        scene.update(moved)
        meshes2 = [m0, meshes[1]]
        bf2 = scene_point_brute_force(pkg, pts, meshes2, moved, root_boxes(pkg, blases))
        check_exact(pkg, pts, meshes2, moved, bf2, scene.closest_point(pts, query="closest"), scene.closest_point(pts, query="any"), "after BLAS refit")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("tlas_algo", [0, 3])
def test_coincident_instances_tie_to_the_lower_index(pkg, tlas_algo):
    """two instances place the same triangles identically, so every answer ties on dist2; one BLAS also holds a far-off extra triangle that stretches its world
    box, so the two are not walked alike.  The lower instance index must win whichever of them that is."""
    mesh = no_negzero(pkg.meshgen.uniform(120, 12))
    v = np.concatenate([mesh["v1"], mesh["v2"], mesh["v3"]])
    lo, hi = v.min(axis=0), v.max(axis=0)
    extra = np.zeros(1, dtype=pkg.meshgen.TRIANGLE)                   # (appended: the prim indices of the shared triangles are the same in both BLASes)
    extra["v1"] = (hi[0] + 50, lo[1], lo[2] - 5); extra["v2"] = (hi[0] + 51, lo[1], lo[2] - 5); extra["v3"] = (hi[0] + 50, lo[1] + 1, lo[2] - 5)
    stretched = no_negzero(np.concatenate([mesh, extra]))
    pts = near_surface_points(pkg, mesh, 1024, np.random.default_rng(tlas_algo))
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        plain, far = bl.add(3, mesh), bl.add(1, stretched)
        for order in ((plain, far), (far, plain)):
            blas_tris = [mesh, stretched] if order[0] is plain else [stretched, mesh]
            inst = make_instances(pkg, [identity(), identity()], [0, 1])
            got = pkg.Scene(sc_ctx).build(tlas_algo, list(order), inst).closest_point(pts, query="closest")
            bf = scene_point_brute_force(pkg, pts, blas_tris, inst, root_boxes(pkg, list(order)))
            assert (got["prim"] != pkg.INVALID).all()
            assert (got["instance"] == 0).all(), f"stretched BLAS at index {1 if order[0] is plain else 0}: {np.count_nonzero(got['instance'])} ties went to instance 1"
            assert bf["well"].mean() >= 0.99
            assert got[bf["well"]].tobytes() == bf["closest"][bf["well"]].tobytes()
    finally:
        bl.close(); sc_ctx.close()


def test_rejections_and_hygiene(pkg):
    mesh = no_negzero(pkg.meshgen.uniform(100, 3))
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    L = pkg.lib()
    try:
        b = bl.add(3, mesh)
        inst = make_instances(pkg, [identity(), mat34(np.eye(3), (2.0, 0, 0))], [0, 0])
        scene = pkg.Scene(sc_ctx)
        pts = scene_points(pkg, world_tris(pkg, [mesh], inst), 250, 4)
        n = len(pts)
        d_pts = sc_ctx.upload(pts)
        pad = 32
        hits = sc_ctx.alloc((n + 2 * pad) * 32)
        pattern = np.full((n + 2 * pad) * 32, 0xAB, dtype=np.uint8)
        hits.upload(pattern)
        h = hits.ptr + pad * 32
        assert L.bvh_scene_closest_point(scene.handle, d_pts.ptr, n, h, 0) == E_INVALID              # not built
        scene.build(2, [b], inst)
        assert L.bvh_scene_closest_point(None, d_pts.ptr, n, h, 0) == E_INVALID
        assert L.bvh_scene_closest_point(scene.handle, d_pts.ptr, n, h, 2) == E_INVALID              # query kind
        assert L.bvh_scene_closest_point(scene.handle, d_pts.ptr, n, h, -1) == E_INVALID
        assert L.bvh_scene_closest_point(scene.handle, None, n, h, 0) == E_INVALID
        assert L.bvh_scene_closest_point(scene.handle, d_pts.ptr, n, None, 0) == E_INVALID
        assert L.bvh_scene_closest_point(scene.handle, d_pts.ptr, n, d_pts.ptr + 16, 0) == E_INVALID   # overlapping
        assert L.bvh_scene_closest_point(scene.handle, h + 32 * (n - 1), n, h, 0) == E_INVALID          # (points inside the last hit record)
        assert L.bvh_scene_closest_point(scene.handle, d_pts.ptr, 0, h, 0) == 0
        sc_ctx.synchronize()
        assert np.array_equal(hits.download(np.uint8, pattern.size), pattern), "an error or n_points == 0 wrote to the hits"
        bf = scene_point_brute_force(pkg, pts, [mesh], inst, root_boxes(pkg, [b]))
        for kind in (0, 1):
            assert L.bvh_scene_closest_point(scene.handle, d_pts.ptr, n, h, kind) == 0
            sc_ctx.synchronize()
            got = hits.download(np.uint8, pattern.size)
            assert np.array_equal(got[: pad * 32], pattern[: pad * 32]) and np.array_equal(got[-pad * 32:], pattern[-pad * 32:])
            rec = np.frombuffer(got[pad * 32: -pad * 32].tobytes(), dtype=pkg.INSTANCE_POINT_HIT)
            assert scene_point_recompute(pkg, pts, [mesh], inst, rec).all()
            if kind == 0:
                assert rec[bf["well"]].tobytes() == bf["closest"][bf["well"]].tobytes()
            assert d_pts.download(pkg.POINT_QUERY, n).tobytes() == pts.tobytes()
        scene.close(); d_pts.free(); hits.free()
    finally:
        bl.close(); sc_ctx.close()
