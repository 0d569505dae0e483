"""bvh_build_many_ploc on the GPU: every tree of a batch byte for byte against bvh_build_ex(BVH_PLOCPP) of that mesh alone on a second context (sizes around the
search radius, every class switch and the wave hand-over, degenerate meshes, all three formats) and against the CPU oracle, clamped NaN / inf inputs as valid
trees, 20 000 meshes validated structurally, independence from position / batch / call with guard bytes, the slices through the consumers (bvh_intersect,
bvh_closest_point, a Scene, bvh_refit_ex), and every rejection."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_build_many import FILL, Guarded, cut, device_input, no_negzero, rays_at

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
F32 = np.float32
E_INVALID = -10001
PLOC = 2
BOUNDARY_COUNTS = [2, 3, 4, 5, 8, 9, 10, 16, 17, 18, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 511, 512, 513, 700, 1100]
ARRAYS = ("nodes", "leaves", "prim_aabbs", "sorted_keys", "sorted_vals", "scene")


@pytest.fixture(scope="module")
def ctx2(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def boundary_meshes(pkg):
    """the issue's sizes, cut in turn from the three generators, + identical triangles (all areas equal: ties go by position) + coplanar meshes"""
    names = ["uniform", "sponza", "bunny"]
    meshes = [cut(pkg, names[k % 3], 131 * k, c) for k, c in enumerate(BOUNDARY_COUNTS)]
    for c in (37, 150):
        meshes.append(np.repeat(cut(pkg, "uniform", 7, 1), c))
    for c in (20, 90):
        flat = cut(pkg, "sponza", 500, c)
        for f in ("v1", "v2", "v3"):
            a = flat[f]; a[:, 2] = 1.25; flat[f] = a
        meshes.append(flat)
    return meshes


def clamped_meshes(pkg):
    """NaN / +-inf vertices: stage E clamps the boxes to +-FLT_MAX, so candidate areas are inf or NaN — one mesh for the wave path, one for the workgroup path"""
    meshes = []
    for c in (30, 70):
        bad = cut(pkg, "bunny", 900, c)
        v1, v2, v3 = bad["v1"], bad["v2"], bad["v3"]
        v1[1, 0] = np.nan; v2[2, 1] = np.inf; v3[3, 2] = -np.inf
        v1[4] = np.nan; v2[4] = np.nan; v3[4] = np.nan                      # a triangle that is NaN on every axis
        v1[5, 0] = np.inf; v2[5, 0] = np.inf; v3[5, 0] = np.inf            # ... and one that is +inf on a whole axis
        bad["v1"], bad["v2"], bad["v3"] = v1, v2, v3
        meshes.append(bad)
    return meshes


def extent_area_f32(tris):
    """Aabb::area of the mesh's extent in f32 arithmetic, the expression of the builders: 2 * (ex*ey + ex*ez + ey*ez)"""
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        e = (v.max(axis=0) - v.min(axis=0)).astype(F32)
        return F32(2) * F32(F32(F32(e[0] * e[1]) + F32(e[0] * e[2])) + F32(e[1] * e[2]))


def many_ploc(pkg, ctx, inp, ranges, n_tris):
    tris = inp.d_tris if inp.tri_format != pkg.TRI_INDEXED else None
    return ctx.build_many_ploc((tris, ranges), tri_format=inp.tri_format, vertices=inp.d_vertices, indices=inp.d_indices, n_vertices=inp.n_vertices, n_tris=n_tris)


def alone(pkg, ctx2, tris_in, count):
    """bvh_build_ex(BVH_PLOCPP) of one mesh on the second context, every array read back"""
    L = pkg.lib()
    r = pkg.Result()
    rc = L.bvh_build_ex(ctx2.handle, PLOC, C.byref(tris_in), count, C.byref(r), None)
    assert rc == 0, rc
    assert (r.layout, r.root, r.n_internal) == (1, 0, count - 1)
    nodes = np.empty(count - 1, dtype=pkg.BVH2_NODE); leaves = np.empty(count, dtype=pkg.PRIMREF)
    keys = np.empty(count, dtype=np.uint32); vals = np.empty(count, dtype=np.uint32)
    scene = np.empty(1, dtype=pkg.AABB); boxes = np.empty(count, dtype=pkg.AABB)
    assert L.bvh_download(ctx2.handle, C.byref(r), nodes.ctypes.data, leaves.ctypes.data, keys.ctypes.data, vals.ctypes.data, scene.ctypes.data) == 0
    assert L.bvh_dev_download(ctx2.handle, boxes.ctypes.data, r.d_prim_aabbs, boxes.nbytes) == 0
    return {"nodes": nodes, "leaves": leaves, "sorted_keys": keys, "sorted_vals": vals, "scene": scene, "prim_aabbs": boxes}


def slices(mt, whole, m):
    n, off, noff = int(mt.ranges["count"][m]), int(mt.out_off[m]), int(mt.node_off[m])
    return {"nodes": whole["nodes"][noff:noff + n - 1], "leaves": whole["leaves"][off:off + n], "sorted_keys": whole["sorted_keys"][off:off + n],
            "sorted_vals": whole["sorted_vals"][off:off + n], "scene": whole["scenes"][m:m + 1], "prim_aabbs": whole["prim_aabbs"][off:off + n]}


def assert_same_tree(got, ref, what):
    for k in ARRAYS:
        assert got[k].tobytes() == ref[k].tobytes(), f"{what}: {k} differs"


def check_against_alone(pkg, ctx2, mt, whole, which):
    ctx2.reserve(int(mt.ranges["count"].max()))
    for m in which:
        ref = alone(pkg, ctx2, mt.tris(m), int(mt.ranges["count"][m]))
        assert_same_tree(slices(mt, whole, m), ref, f"fmt {mt.input.tri_format} mesh {m} ({int(mt.ranges['count'][m])} triangles) against bvh_build_ex")


def validate_structure(pkg, mt, whole):
    """numpy, all meshes at once (PLOC layout): each leaf and each internal node but the root has exactly one parent, everything is reached from node 0, each
    internal box is the union of its children's, the root box is the extent, leaves hold {prim, stage E box} in sorted order, prims are a permutation per mesh,
    keys ascend (ties by index)"""
    counts = mt.ranges["count"].astype(np.int64); M = mt.n_meshes
    out_off, node_off, total = mt.out_off, mt.node_off, mt.total
    nodes, leaves = whole["nodes"], whole["leaves"]; N = len(nodes)
    assert N == total - M and len(leaves) == total
    mesh_of_node = np.repeat(np.arange(M), counts - 1)
    ni = (counts - 1)[mesh_of_node]
    # children as global ids: internal node i of mesh m -> node_off[m] + i, leaf j -> N + out_off[m] + j
    gchild = []
    for side in ("left", "right"):
        ch = nodes[side].astype(np.int64)
        assert (ch < 2 * ni + 1).all(), "a child index beyond the mesh's clusters"
        gchild.append(np.where(ch >= ni, N + out_off[mesh_of_node] + ch - ni, node_off[mesh_of_node] + ch))
    gl, gr = gchild
    refs = np.bincount(np.concatenate([gl, gr]), minlength=N + total)
    want = np.ones(N + total, dtype=np.int64); want[node_off] = 0
    assert np.array_equal(refs, want), "a cluster has no parent or several"
    bmin = np.concatenate([nodes["min"], leaves["min"]]); bmax = np.concatenate([nodes["max"], leaves["max"]])
    assert np.array_equal(nodes["min"], np.minimum(bmin[gl], bmin[gr])) and np.array_equal(nodes["max"], np.maximum(bmax[gl], bmax[gr])), "an internal box is not the union"
    seen = np.zeros(N + total, dtype=bool); frontier = node_off.copy()
    for _ in range(int(counts.max()) + 1):                                  # level by level from the roots: everything is reached (no detached cycle)
        seen[frontier] = True
        f = frontier[frontier < N]
        if len(f) == 0:
            break
        frontier = np.concatenate([gl[f], gr[f]])
    assert seen.all(), "clusters that node 0 does not reach"
    assert nodes["min"][node_off].tobytes() == whole["scenes"]["min"].tobytes() and nodes["max"][node_off].tobytes() == whole["scenes"]["max"].tobytes()
    # leaves
    mesh_of_pos = np.repeat(np.arange(M), counts)
    prim = leaves["prim"].astype(np.int64)
    assert (prim < counts[mesh_of_pos]).all()
    gprim = out_off[mesh_of_pos] + prim
    assert np.array_equal(np.bincount(gprim, minlength=total), np.ones(total, dtype=np.int64)), "leaf primitives are not a permutation per mesh"
    assert np.array_equal(prim, whole["sorted_vals"].astype(np.int64)), "leaf order is not the sorted order"
    lb = whole["prim_aabbs"][gprim]
    assert leaves["min"].tobytes() == lb["min"].tobytes() and leaves["max"].tobytes() == lb["max"].tobytes(), "leaf boxes are not stage E's"
    k = whole["sorted_keys"].astype(np.int64); v = whole["sorted_vals"].astype(np.int64)
    same_mesh = mesh_of_pos[1:] == mesh_of_pos[:-1]
    assert ((k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (v[1:] > v[:-1])))[same_mesh].all(), "keys are not ascending {key, index}"


# ---- 1. parity at the boundaries ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_parity_at_the_boundaries(pkg, orc, ctx, ctx2, fmt):
    meshes = boundary_meshes(pkg)
    for t in meshes:
        assert np.isfinite(extent_area_f32(t)), "the identity's precondition: a finite f32 extent area"
    inp, ranges, n_tris, bufs = device_input(pkg, ctx, meshes, fmt, gap=4 if fmt == pkg.TRI_PACKED36 else 1)
    assert all(ranges[k + 1][0] > ranges[k][0] + ranges[k][1] for k in range(len(ranges) - 1)), "gaps between the meshes"
    mt = many_ploc(pkg, ctx, inp, ranges, n_tris)
    try:
        ctx.synchronize()
        whole = mt.download_all()
        assert "roots" not in whole and whole["leaves"] is not None
        check_against_alone(pkg, ctx2, mt, whole, range(mt.n_meshes))
        validate_structure(pkg, mt, whole)
        d = mt.download(9)                                                  # the per-mesh read-back names the same bytes
        assert d["layout"] == 1 and d["root"] == 0
        assert_same_tree(d, slices(mt, whole, 9), "download(9)")
        # the CPU oracle: one mesh per path (wave 33, workgroup 257, ordinary tail 700) and two more (a global iteration first: 1100; identical triangles: 150)
        for m in (BOUNDARY_COUNTS.index(33), BOUNDARY_COUNTS.index(257), BOUNDARY_COUNTS.index(700), BOUNDARY_COUNTS.index(1100), len(BOUNDARY_COUNTS) + 1):
            ref = orc.build_tree(2, meshes[m])
            got = slices(mt, whole, m)
            assert got["leaves"].tobytes() == ref["leaves"].tobytes(), f"mesh {m}: leaves differ from the oracle"
            assert got["nodes"].tobytes() == ref["nodes"].tobytes(), f"mesh {m}: nodes differ from the oracle"
    finally:
        mt.free()
        for b in bufs:
            b.free()


def test_host_meshes_every_format_one_tree(pkg, ctx):
    """a list of host meshes through the binding's own packing: the trees do not depend on the format"""
    meshes = [cut(pkg, "uniform", 40 * k, c) for k, c in enumerate([7, 64, 65, 300, 600])]
    got = []
    for fmt in (0, 1, 2):
        mt = ctx.build_many_ploc(meshes, tri_format=fmt)
        ctx.synchronize()
        whole = mt.download_all()
        got.append(b"".join(whole[k].tobytes() for k in ("nodes", "leaves", "prim_aabbs", "scenes", "sorted_keys", "sorted_vals")))
        mt.free()
    assert got[0] == got[1] == got[2]


# ---- 2. clamped inputs ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_clamped_inputs_give_valid_trees(pkg, ctx, fmt):
    meshes = clamped_meshes(pkg)
    assert not any(np.isfinite(extent_area_f32(t)) for t in meshes)          # (outside the identity's precondition: no byte comparison here)
    inp, ranges, n_tris, bufs = device_input(pkg, ctx, meshes, fmt, gap=4)
    mt = many_ploc(pkg, ctx, inp, ranges, n_tris)
    try:
        ctx.synchronize()                                                   # the stream drains: every round found its mutual pair
        whole = mt.download_all()
        for k in ("nodes", "leaves", "prim_aabbs", "scenes"):
            assert not np.isnan(whole[k]["min"]).any() and not np.isnan(whole[k]["max"]).any()
        validate_structure(pkg, mt, whole)
    finally:
        mt.free()
        for b in bufs:
            b.free()


# ---- 3. many meshes -------------------------------------------------------------------------------------------------------------------------------------------
def test_twenty_thousand_meshes(pkg, ctx, ctx2):
    rng = np.random.default_rng(2024)
    counts = rng.integers(2, 513, 20_000)
    src = no_negzero(pkg.meshgen.uniform(400_000, 9))
    firsts = rng.integers(0, len(src) - 512, 20_000)                        # (meshes may share triangles)
    d = ctx.upload(src)
    ranges = np.stack([firsts, counts], axis=1)
    try:
        mt = ctx.build_many_ploc((d, ranges), n_tris=len(src))
        ctx.synchronize()
        whole = mt.download_all()
        validate_structure(pkg, mt, whole)
        sample = np.random.default_rng(5).choice(20_000, 64, replace=False)
        sample[:6] = [0, 19_999, int(np.argmax(counts == 64)), int(np.argmax(counts == 65)), int(np.argmax(counts == 512)), int(np.argmax(counts == 2))]
        check_against_alone(pkg, ctx2, mt, whole, sample.tolist())
        mt.free()
        one = ctx.build_many_ploc((d, [[5, 77]]), n_tris=len(src))           # n_meshes == 1
        ctx.synchronize()
        w1 = one.download_all()
        validate_structure(pkg, one, w1)
        check_against_alone(pkg, ctx2, one, w1, [0])
        one.free()
    finally:
        d.free()


# ---- 4. independence, guard bytes -----------------------------------------------------------------------------------------------------------------------------
def out_sizes(total, n):
    return [(total - n) * 32, total * 28, total * 24, n * 24, total * 4, total * 4]


def raw_many_ploc(pkg, ctx, inp, ranges, n_tris, keys=True):
    """bvh_build_many_ploc through the C ABI into guarded, pre-filled arrays: (rc, [payload bytes of the six arrays], guards intact?)"""
    rg = pkg.many_check_ranges(ranges, n_tris, inp.tri_format)
    _, _, total = pkg.many_ploc_layout(rg["count"]); n = len(rg)
    g = [Guarded(pkg, ctx, s) for s in out_sizes(total, n)]
    out = pkg.ManyPlocOut(g[0].ptr, g[1].ptr, g[2].ptr, g[3].ptr, g[4].ptr if keys else None, g[5].ptr if keys else None)
    rc = pkg.lib().bvh_build_many_ploc(ctx.handle, PLOC, C.byref(inp), n_tris, rg.ctypes.data, n, C.byref(out), None)
    ctx.synchronize()
    parts = [x.read() for x in g]
    intact = all((lo == FILL).all() and (hi == FILL).all() for lo, _, hi in parts)
    for x in g:
        x.free()
    return rc, [p[1].tobytes() for p in parts], intact


def test_independent_of_position_batch_and_call(pkg, ctx):
    probe = {c: cut(pkg, "sponza", 77, c) for c in (50, 200, 600)}         # one mesh per path
    filler = [cut(pkg, "uniform", 61 * k, c) for k, c in enumerate([3, 64, 65, 130, 512, 9, 40])]
    batches = [list(probe.values()) + filler, filler[:3] + [probe[600], probe[50]] + filler[3:] + [probe[200]], [probe[200]] + filler[::-1] + [probe[50], probe[600]]]
    where = [{50: 0, 200: 1, 600: 2}, {600: 3, 50: 4, 200: len(filler) + 2}, {200: 0, 50: len(filler) + 1, 600: len(filler) + 2}]
    seen = {}
    for b, (meshes, pos) in enumerate(zip(batches, where)):
        inp, ranges, n_tris, bufs = device_input(pkg, ctx, meshes, pkg.TRI_PADDED64, gap=b)
        host_in = bufs[0].download(np.uint8, bufs[0].nbytes)
        rc, arrays, intact = raw_many_ploc(pkg, ctx, inp, ranges, n_tris)
        assert rc == 0 and intact, "guard bytes around an output array were written"
        rc2, arrays2, intact2 = raw_many_ploc(pkg, ctx, inp, ranges, n_tris)
        assert rc2 == 0 and intact2 and arrays == arrays2, "two identical calls differ"
        assert bufs[0].download(np.uint8, bufs[0].nbytes).tobytes() == host_in.tobytes(), "the input was written"
        counts = [len(t) for t in meshes]
        out_off, node_off, _ = pkg.many_ploc_layout(counts)
        for c, m in pos.items():
            assert counts[m] == c
            o, no = int(out_off[m]), int(node_off[m])
            sl = (arrays[0][32 * no:32 * (no + c - 1)], arrays[1][28 * o:28 * (o + c)], arrays[2][24 * o:24 * (o + c)], arrays[3][24 * m:24 * (m + 1)],
                  arrays[4][4 * o:4 * (o + c)], arrays[5][4 * o:4 * (o + c)])
            assert seen.setdefault(c, sl) == sl, f"the {c}-triangle mesh depends on its place in batch {b}"
        for x in bufs:
            x.free()
    # without the optional arrays: the others are the same bytes, the optional ones stay untouched
    inp, ranges, n_tris, bufs = device_input(pkg, ctx, batches[0], pkg.TRI_PADDED64)
    rc, a, ok = raw_many_ploc(pkg, ctx, inp, ranges, n_tris)
    rc2, b2, ok2 = raw_many_ploc(pkg, ctx, inp, ranges, n_tris, keys=False)
    assert rc == 0 and rc2 == 0 and ok and ok2 and a[:4] == b2[:4] and set(b2[4]) == {FILL} and set(b2[5]) == {FILL}
    for x in bufs:
        x.free()


# ---- 5. consumers ---------------------------------------------------------------------------------------------------------------------------------------------
def consumer_meshes(pkg):
    return [cut(pkg, ["uniform", "sponza", "bunny"][k % 3], 97 * k, c) for k, c in enumerate([64, 300, 512])]


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_queries_on_slices_answer_as_single_trees(pkg, ctx, ctx2, fmt):
    meshes = consumer_meshes(pkg)
    inp, ranges, n_tris, bufs = device_input(pkg, ctx, meshes, fmt, gap=4)
    mt = many_ploc(pkg, ctx, inp, ranges, n_tris)
    tris_arg = inp.d_tris if fmt != pkg.TRI_INDEXED else None
    lb = ctx.build_many((tris_arg, ranges), algo=pkg.ALGO_TWOPASS, tri_format=fmt, vertices=inp.d_vertices, indices=inp.d_indices, n_vertices=inp.n_vertices, n_tris=n_tris)
    ctx.reserve(1024); ctx2.reserve(1024)
    try:
        ctx.synchronize()
        for m, tris in enumerate(meshes):
            single = pkg.BUILDERS[PLOC]().build(ctx2, tris)
            rays = rays_at(pkg, tris, 4096, 10 + m)
            pts = np.zeros(4096, dtype=pkg.POINT_QUERY)
            pts["point"] = rays["origin"]; pts["radius"] = np.inf
            want_hits, want_pts = single.intersect(rays), single.closest_point(pts)
            assert (want_hits["prim"] != pkg.INVALID).sum() > 100
            t = mt.tris(m)
            kw = dict(tris=t.d_tris, vertices=t.d_vertices, indices=t.d_indices, n_vertices=t.n_vertices, tri_format=fmt)
            b = mt.builder(m)
            assert isinstance(b, pkg.BUILDERS[PLOC]) and b.result.layout == 1
            assert b.intersect(rays, **kw).tobytes() == want_hits.tobytes(), f"mesh {m}: bvh_intersect on the slice differs from the single build's"
            assert b.closest_point(pts, **kw).tobytes() == want_pts.tobytes(), f"mesh {m}: bvh_closest_point on the slice differs from the single build's"
            if fmt == pkg.TRI_PADDED64:                                     # the slice's own d_tris names its triangles
                assert b.intersect(rays).tobytes() == want_hits.tobytes()
            l = lb.builder(m)                                               # answers do not depend on the builder
            assert l.intersect(rays, **kw).tobytes() == want_hits.tobytes(), f"mesh {m}: the LBVH batch's tree answers differently"
            assert l.closest_point(pts, **kw).tobytes() == want_pts.tobytes(), f"mesh {m}: the LBVH batch's tree answers differently"
    finally:
        mt.free(); lb.free()
        for x in bufs:
            x.free()


def test_scene_over_many_ploc_trees(pkg, ctx, ctx2):
    rng = np.random.default_rng(64)
    counts = rng.integers(8, 200, 64)
    meshes = [cut(pkg, "uniform", 53 * k, int(c)) for k, c in enumerate(counts)]
    mt = ctx.build_many_ploc(meshes)
    inst = np.zeros(64, dtype=pkg.INSTANCE)
    for k in range(64):
        inst["object_to_world"][k] = np.array([1, 0, 0, 1.5 * (k % 4), 0, 1, 0, 1.5 * ((k // 4) % 4), 0, 0, 1, 1.5 * (k // 16)], dtype=F32)
        inst["blas"][k] = (k * 7) % 64
    world = []
    for k in range(64):
        w = meshes[inst["blas"][k]].copy()
        for f in ("v1", "v2", "v3"):
            w[f] = w[f] + inst["object_to_world"][k][[3, 7, 11]]
        world.append(w)
    rays = rays_at(pkg, np.concatenate(world), 4096, 3)
    keep, sc_ref = [], pkg.Context(0)
    try:
        ctx.synchronize()
        scene = pkg.Scene(ctx).build(pkg.ALGO_HPLOC, [mt.blas(m) for m in range(64)], inst)
        got = scene.intersect(rays)
        scene.close()
        ref_blas = []                                                       # individually built trees, copied out of the building context's arena
        for tris in meshes:
            n = len(tris)
            b = pkg.BUILDERS[PLOC]().build(ctx2, tris)
            dn, dl, dt = ctx2.alloc((n - 1) * 32), ctx2.alloc(n * 28), ctx2.upload(tris); keep += [dn, dl, dt]
            assert pkg.lib().bvh_dev_copy(ctx2.handle, dn.ptr, b.result.d_nodes, (n - 1) * 32) == 0
            assert pkg.lib().bvh_dev_copy(ctx2.handle, dl.ptr, b.result.d_leaves, n * 28) == 0
            r = pkg.Result.from_buffer_copy(b.result)
            r.d_nodes, r.d_leaves, r.d_tris, r.d_prim_aabbs, r.d_sorted_keys, r.d_sorted_vals, r.d_scene_extent, r.d_morton_keys = dn.ptr, dl.ptr, dt.ptr, None, None, None, None, None
            ref_blas.append(pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0)))
        ctx2.synchronize()
        ref_scene = pkg.Scene(sc_ref).build(pkg.ALGO_HPLOC, ref_blas, inst)
        want = ref_scene.intersect(rays)
        ref_scene.close()
        assert (want["prim"] != pkg.INVALID).sum() > 400
        assert got.tobytes() == want.tobytes()
    finally:
        mt.free(); sc_ref.close()
        for x in keep:
            x.free()


def test_refit_of_a_slice(pkg, ctx, ctx2):
    meshes = consumer_meshes(pkg)
    mt = ctx.build_many_ploc(meshes)
    ctx.reserve(1024); ctx2.reserve(1024)
    rng = np.random.default_rng(8)
    try:
        ctx.synchronize()
        before = mt.download_all()
        for m in (0, 2):
            tris = meshes[m]
            moved = tris.copy()
            for f in ("v1", "v2", "v3"):
                moved[f] = (moved[f] + rng.normal(0.0, 0.05, moved[f].shape)).astype(F32)
            moved = no_negzero(moved)
            d_moved, d_moved2 = ctx.upload(moved), ctx2.upload(moved)
            b = mt.builder(m)
            b.refit_ex(tris=d_moved)
            ctx.synchronize()
            got = mt.download(m)
            single = pkg.BUILDERS[PLOC]().build(ctx2, tris)
            single.refit_ex(tris=d_moved2)
            ctx2.synchronize()
            want = single.download()
            boxes = np.empty(len(tris), dtype=pkg.AABB)
            assert pkg.lib().bvh_dev_download(ctx2.handle, boxes.ctypes.data, single.result.d_prim_aabbs, boxes.nbytes) == 0
            want["prim_aabbs"] = boxes
            assert_same_tree(got, want, f"refit of mesh {m} against the refit of the single build")
            assert got["nodes"].tobytes() != slices(mt, before, m)["nodes"].tobytes()
            d_moved.free(); d_moved2.free()
        after = mt.download_all()                                           # the other mesh's slice was not touched
        assert_same_tree(slices(mt, after, 1), slices(mt, before, 1), "mesh 1 after its neighbours' refits")
    finally:
        mt.free()


def test_kernel_times_name_both_kernels(pkg):
    c = pkg.Context(0)
    try:
        c.set_profiling(2)
        meshes = [cut(pkg, "uniform", 10 * k, n) for k, n in enumerate([10, 64, 100, 256, 400])]
        mt = c.build_many_ploc(meshes)
        c.synchronize()
        times = c.kernel_times()
        assert times["k_many_ploc_wave"][1] == 1 and times["k_many_ploc_block"][1] == 3, times
        assert mt.timings.sampled == 1 and mt.timings.ms_build > 0 and mt.timings.ms_total == mt.timings.ms_build and mt.timings.ploc_iterations == 0
        mt.free()
    finally:
        c.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(pkg, ctx):
    L = pkg.lib()
    meshes = [cut(pkg, "uniform", 0, c) for c in (12, 100, 8)]
    inp, ranges, n_tris, bufs = device_input(pkg, ctx, meshes, pkg.TRI_PADDED64)
    packed, pranges, pn, pbufs = device_input(pkg, ctx, meshes, pkg.TRI_PACKED36)
    indexed, iranges, i_n, ibufs = device_input(pkg, ctx, meshes, pkg.TRI_INDEXED)
    rg = pkg.many_check_ranges(ranges, n_tris)
    _, _, total = pkg.many_ploc_layout(rg["count"]); n = len(rg)
    sizes = out_sizes(total, n)
    g = [Guarded(pkg, ctx, s) for s in sizes]
    NODES, LEAVES, BOXES, SCENES, KEYS, VALS = range(6)

    def out_of(ptrs):
        return pkg.ManyPlocOut(*ptrs)
    good = [x.ptr for x in g]

    def with_(k, v):
        p = list(good); p[k] = v
        return out_of(p)

    def call(algo=PLOC, inp_=inp, n_tris_=n_tris, rg_=rg, n_=n, out=None, ctx_=ctx.handle, ranges_null=False, in_null=False, out_null=False):
        o = out_of(good) if out is None else out
        return L.bvh_build_many_ploc(ctx_, algo, None if in_null else C.byref(inp_), n_tris_, None if ranges_null else rg_.ctypes.data, n_, None if out_null else C.byref(o), None)

    def ranges_of(rows):
        a = np.empty(len(rows), dtype=pkg.MESH_RANGE)
        a["first"], a["count"] = [r[0] for r in rows], [r[1] for r in rows]
        return a
    bad_in = lambda **kw: pkg.BuildInput(*[kw.get(k, getattr(inp, k)) for k in ("tri_format", "morton_bits", "d_tris", "d_vertices", "d_indices", "n_vertices", "reserved")])
    irg = pkg.many_check_ranges(iranges, i_n, 2)
    cases = {
        "NULL ctx": call(ctx_=None), "NULL in": call(in_null=True), "NULL ranges": call(ranges_null=True), "NULL out": call(out_null=True),
        "NULL d_nodes": call(out=with_(NODES, None)), "NULL d_leaves": call(out=with_(LEAVES, None)), "NULL d_prim_aabbs": call(out=with_(BOXES, None)),
        "NULL d_scene_extents": call(out=with_(SCENES, None)),
        "two-pass": call(algo=0), "single-pass": call(algo=1), "HPLOC": call(algo=3), "algo 7": call(algo=7),
        "60-bit codes": call(inp_=bad_in(morton_bits=60)), "format 3": call(inp_=bad_in(tri_format=3)), "NULL d_tris": call(inp_=bad_in(d_tris=None)),
        "unaligned PACKED36": call(inp_=pkg.BuildInput(1, 30, packed.d_tris + 4, None, None, 0, 0), n_tris_=pn - 1, rg_=pkg.many_check_ranges(pranges, pn, 1)),
        "INDEXED without vertices": call(inp_=pkg.BuildInput(2, 30, None, None, indexed.d_indices, indexed.n_vertices, 0), n_tris_=i_n),
        "INDEXED with n_vertices 0": call(inp_=pkg.BuildInput(2, 30, None, indexed.d_vertices, indexed.d_indices, 0, 0), n_tris_=i_n),
        "no mesh": call(n_=0),
        "count 1": call(rg_=ranges_of([(0, 12), (12, 1), (13, 107)])), "count 0": call(rg_=ranges_of([(0, 12), (12, 0), (12, 108)])),
        "past n_tris": call(rg_=ranges_of([(0, 12), (12, 100), (113, 8)])), "first + count wraps": call(rg_=ranges_of([(0, 12), (12, 100), (0xFFFFFFFC, 8)])),
        "misaligned PACKED36 first": call(inp_=packed, n_tris_=pn, rg_=ranges_of([(0, 12), (14, 100), (116, 8)])),
        "total 2^30": call(n_tris_=1 << 31, rg_=ranges_of([(0, 1 << 29), (0, 1 << 29)]), n_=2),      # (rejected on the host: no array is touched)
        # overlaps: every pair of output arrays, and each output array against the input
        "leaves overlap nodes": call(out=with_(LEAVES, good[NODES] + 64)), "boxes overlap nodes": call(out=with_(BOXES, good[NODES] + 32)),
        "scenes inside nodes": call(out=with_(SCENES, good[NODES] + 32)), "keys inside nodes": call(out=with_(KEYS, good[NODES])),
        "vals inside nodes": call(out=with_(VALS, good[NODES] + 4)),
        "boxes overlap leaves": call(out=with_(BOXES, good[LEAVES] + 28)), "scenes inside leaves": call(out=with_(SCENES, good[LEAVES])),
        "keys inside leaves": call(out=with_(KEYS, good[LEAVES] + 28)), "vals inside leaves": call(out=with_(VALS, good[LEAVES] + 56)),
        "scenes inside boxes": call(out=with_(SCENES, good[BOXES] + 24)), "keys inside boxes": call(out=with_(KEYS, good[BOXES])),
        "vals inside boxes": call(out=with_(VALS, good[BOXES] + 48)),
        "keys overlap scenes": call(out=with_(KEYS, good[SCENES] + 8)), "vals overlap scenes": call(out=with_(VALS, good[SCENES])),
        "keys overlap vals": call(out=with_(VALS, good[KEYS] + 8)),
        "nodes end in the input": call(out=with_(NODES, inp.d_tris - sizes[NODES] + 32)), "leaves are the input": call(out=with_(LEAVES, inp.d_tris)),
        "boxes are the input": call(out=with_(BOXES, inp.d_tris + 64)), "scenes in the input": call(out=with_(SCENES, inp.d_tris + 128)),
        "keys in the input": call(out=with_(KEYS, inp.d_tris)), "vals in the input": call(out=with_(VALS, inp.d_tris + 4)),
        "leaves overlap the indices": call(inp_=indexed, n_tris_=i_n, rg_=irg, out=with_(LEAVES, indexed.d_indices + 4)),
        "vals overlap the indices": call(inp_=indexed, n_tris_=i_n, rg_=irg, out=with_(VALS, indexed.d_indices + 4)),
        "scenes overlap the vertices": call(inp_=indexed, n_tris_=i_n, rg_=irg, out=with_(SCENES, indexed.d_vertices)),
        "leaves overlap the vertices": call(inp_=indexed, n_tris_=i_n, rg_=irg, out=with_(LEAVES, indexed.d_vertices + 12)),
    }
    ctx.synchronize()
    wrong = {k: v for k, v in cases.items() if v != E_INVALID}
    assert not wrong, wrong
    for x in g:
        lo, mid, hi = x.read()
        assert (lo == FILL).all() and (mid == FILL).all() and (hi == FILL).all(), "a rejected call wrote to an output array"
    assert call() == 0                                                      # ... and the same arguments, unbroken, build
    ctx.synchronize()
    for x in g:
        lo, mid, hi = x.read()
        assert (lo == FILL).all() and (hi == FILL).all() and not (mid == FILL).all()
    assert call(inp_=indexed, n_tris_=i_n, rg_=irg) == 0 and call(inp_=packed, n_tris_=pn, rg_=pkg.many_check_ranges(pranges, pn, 1)) == 0
    ctx.synchronize()
    for algo in (pkg.ALGO_PLOCPP, pkg.ALGO_HPLOC):                          # the LBVH call still turns both away
        with pytest.raises(pkg.BvhError):
            ctx.build_many(meshes, algo=algo)
    for x in g + bufs + pbufs + ibufs:
        x.free()
