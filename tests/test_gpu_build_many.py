"""bvh_build_many on the GPU: every tree of a batch byte for byte against bvh_build_ex of that mesh alone on a second context (sizes around every path switch,
degenerate meshes, both algos, all three formats), 20 000 meshes validated structurally, independence from position / batch / call with guard words, the
slices through the consumers (bvh_intersect, bvh_closest_point, a Scene, bvh_refit), and every rejection."""
import ctypes as C

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
F32 = np.float32
E_INVALID = -10001
BOUNDARY_COUNTS = [2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 511, 512, 513, 700]
FILL = 0xA5


@pytest.fixture(scope="module")
def ctx2(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def no_negzero(tris):
    t = tris.copy()
    for f in ("v1", "v2", "v3"):
        a = t[f]; a[a == 0] = 0.0; t[f] = a
    return t


_SRC = {}


def source(pkg, name):
    if name not in _SRC:
        gen = {"uniform": lambda: pkg.meshgen.uniform(6000, 17), "sponza": lambda: pkg.meshgen.sponza_like(6000, 3), "bunny": lambda: pkg.meshgen.bunny_like(6000, 2)}[name]
        _SRC[name] = no_negzero(gen())
    return _SRC[name]


def cut(pkg, name, start, count):
    s = source(pkg, name)
    start %= len(s) - count
    return s[start:start + count].copy()


def boundary_meshes(pkg):
    """the issue's sizes, cut in turn from the three generators, + identical triangles (ties go by index), coplanar (zero extent on an axis), NaN / inf vertices —
    each degenerate kind once per path (wave, workgroup)"""
    names = ["uniform", "sponza", "bunny"]
    meshes = [cut(pkg, names[k % 3], 131 * k, c) for k, c in enumerate(BOUNDARY_COUNTS)]
    for c in (37, 150):
        same = cut(pkg, "uniform", 7, 1)
        meshes.append(np.repeat(same, c))
    for c in (20, 90):
        flat = cut(pkg, "sponza", 500, c)
        for f in ("v1", "v2", "v3"):
            a = flat[f]; a[:, 2] = 1.25; flat[f] = a
        meshes.append(flat)
    for c in (30, 70):
        bad = cut(pkg, "bunny", 900, c)
        v1, v2, v3 = bad["v1"], bad["v2"], bad["v3"]
        v1[1, 0] = np.nan; v2[2, 1] = np.inf; v3[3, 2] = -np.inf
        v1[4] = np.nan; v2[4] = np.nan; v3[4] = np.nan                      # a triangle that is NaN on every axis
        v1[5, 0] = np.inf; v2[5, 0] = np.inf; v3[5, 0] = np.inf            # ... and one that is +inf on a whole axis
        bad["v1"], bad["v2"], bad["v3"] = v1, v2, v3
        meshes.append(bad)
    for t in meshes:
        for f in ("v1", "v2", "v3"):
            assert not np.signbit(t[f][t[f] == 0]).any()
    return meshes


def flat9(tris):
    return np.ascontiguousarray(np.concatenate([tris["v1"], tris["v2"], tris["v3"]], axis=1), dtype=F32)


def device_input(pkg, ctx, meshes, fmt, gap=0):
    """the meshes laid out by hand in one input of format fmt, `gap` unused records between consecutive meshes (PACKED36: firsts rounded up to multiples of 4).
    Returns (BuildInput, ranges rows, n_tris, buffers)"""
    firsts, at = [], 0
    for t in meshes:
        if fmt == pkg.TRI_PACKED36:
            at = (at + 3) // 4 * 4
        firsts.append(at); at += len(t) + gap
    n_tris = at
    ranges = [(f, len(t)) for f, t in zip(firsts, meshes)]
    if fmt == pkg.TRI_PADDED64:
        host = np.zeros(n_tris, dtype=pkg.meshgen.TRIANGLE)
        for f, t in zip(firsts, meshes):
            host[f:f + len(t)] = t
        d = ctx.upload(host)
        return pkg.BuildInput(fmt, 30, d.ptr, None, None, 0, 0), ranges, n_tris, [d]
    if fmt == pkg.TRI_PACKED36:
        host = np.zeros((n_tris, 9), dtype=F32)
        for f, t in zip(firsts, meshes):
            host[f:f + len(t)] = flat9(t)
        d = ctx.upload(host)
        return pkg.BuildInput(fmt, 30, d.ptr, None, None, 0, 0), ranges, n_tris, [d]
    verts = np.concatenate([flat9(t).reshape(-1, 3) for t in meshes])       # vertex soup; indices per mesh, unused triples (the gaps) point at vertex 0
    idx = np.zeros((n_tris, 3), dtype=np.uint32)
    base = 0
    for f, t in zip(firsts, meshes):
        idx[f:f + len(t)] = base + np.arange(3 * len(t), dtype=np.uint32).reshape(-1, 3); base += 3 * len(t)
    dv, di = ctx.upload(verts), ctx.upload(idx)
    return pkg.BuildInput(fmt, 30, None, dv.ptr, di.ptr, len(verts), 0), ranges, n_tris, [dv, di]


def many(pkg, ctx, algo, inp, ranges, n_tris):
    tris = inp.d_tris if inp.tri_format != pkg.TRI_INDEXED else None
    return ctx.build_many((tris, ranges), algo=algo, tri_format=inp.tri_format, vertices=inp.d_vertices, indices=inp.d_indices, n_vertices=inp.n_vertices, n_tris=n_tris)


def alone(pkg, ctx2, algo, tris_in, count):
    """bvh_build_ex of one mesh on the second context, every array read back"""
    L = pkg.lib()
    r = pkg.Result()
    rc = L.bvh_build_ex(ctx2.handle, algo, C.byref(tris_in), count, C.byref(r), None)
    assert rc == 0, rc
    nodes = np.empty(2 * count - 1, dtype=pkg.BVH2_NODE); keys = np.empty(count, dtype=np.uint32); vals = np.empty(count, dtype=np.uint32)
    scene = np.empty(1, dtype=pkg.AABB); boxes = np.empty(count, dtype=pkg.AABB)
    assert L.bvh_download(ctx2.handle, C.byref(r), nodes.ctypes.data, None, keys.ctypes.data, vals.ctypes.data, scene.ctypes.data) == 0
    assert L.bvh_dev_download(ctx2.handle, boxes.ctypes.data, r.d_prim_aabbs, boxes.nbytes) == 0
    return {"nodes": nodes, "sorted_keys": keys, "sorted_vals": vals, "scene": scene, "prim_aabbs": boxes, "root": r.root}


def slices(mt, whole, m):
    n, off, noff = int(mt.ranges["count"][m]), int(mt.out_off[m]), int(mt.node_off[m])
    return {"nodes": whole["nodes"][noff:noff + 2 * n - 1], "sorted_keys": whole["sorted_keys"][off:off + n], "sorted_vals": whole["sorted_vals"][off:off + n],
            "scene": whole["scenes"][m:m + 1], "prim_aabbs": whole["prim_aabbs"][off:off + n], "root": int(whole["roots"][m])}


def assert_same_tree(got, ref, what):
    assert got["root"] == ref["root"], f"{what}: root {got['root']} != {ref['root']}"
    for k in ("prim_aabbs", "sorted_keys", "sorted_vals", "nodes", "scene"):
        assert got[k].tobytes() == ref[k].tobytes(), f"{what}: {k} differs from bvh_build_ex"


def check_against_alone(pkg, ctx2, mt, whole, which):
    ctx2.reserve(int(mt.ranges["count"].max()))
    for m in which:
        ref = alone(pkg, ctx2, mt.algo, mt.tris(m), int(mt.ranges["count"][m]))
        assert_same_tree(slices(mt, whole, m), ref, f"algo {mt.algo} fmt {mt.input.tri_format} mesh {m} ({int(mt.ranges['count'][m])} triangles)")


# ---- 1. parity at the boundaries ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("algo", [0, 1])
def test_parity_at_the_boundaries(pkg, ctx, ctx2, algo, fmt):
    meshes = boundary_meshes(pkg)
    inp, ranges, n_tris, bufs = device_input(pkg, ctx, meshes, fmt, gap=4 if fmt == pkg.TRI_PACKED36 else 1)
    if fmt == pkg.TRI_PACKED36:
        assert all(f % 4 == 0 for f, _ in ranges) and all(ranges[k + 1][0] > ranges[k][0] + ranges[k][1] for k in range(len(ranges) - 1))
    mt = many(pkg, ctx, algo, inp, ranges, n_tris)
    try:
        ctx.synchronize()
        whole = mt.download_all()
        if algo == 0:
            assert not whole["roots"].any()
        assert np.array_equal(whole["roots"], mt.roots())
        check_against_alone(pkg, ctx2, mt, whole, range(mt.n_meshes))
        d = mt.download(9)                                                  # the per-mesh read-back names the same bytes
        assert_same_tree(d, slices(mt, whole, 9), "download(9)")
    finally:
        mt.free()
        for b in bufs:
            b.free()


def test_host_meshes_every_format_one_tree(pkg, ctx):
    """a list of host meshes through the binding's own packing: the trees do not depend on the format"""
    meshes = [cut(pkg, "uniform", 40 * k, c) for k, c in enumerate([7, 64, 65, 300, 600])]
    got = []
    for fmt in (0, 1, 2):
        mt = ctx.build_many(meshes, algo=pkg.ALGO_SINGLEPASS, tri_format=fmt)
        ctx.synchronize()
        whole = mt.download_all()
        got.append(b"".join(whole[k].tobytes() for k in ("nodes", "prim_aabbs", "scenes", "roots", "sorted_keys", "sorted_vals")))
        mt.free()
    assert got[0] == got[1] == got[2]


# ---- 2. many meshes -------------------------------------------------------------------------------------------------------------------------------------------
def validate_structure(pkg, mt, whole):
    """numpy, all meshes at once: each leaf is reached exactly once from its root, each internal box is the union of its children's, the root box is the mesh
    extent, leaf records hold {prim, INVALID, stage E box}, prims are a permutation per mesh, keys ascend (ties by index)"""
    counts = mt.ranges["count"].astype(np.int64); M = mt.n_meshes
    out_off, node_off, total = mt.out_off, mt.node_off, mt.total
    nodes = whole["nodes"]; N = len(nodes)
    assert N == 2 * total - M
    mesh_of_node = np.repeat(np.arange(M), 2 * counts - 1)
    local = np.arange(N) - node_off[mesh_of_node]
    ni = (counts - 1)[mesh_of_node]
    is_leaf = local >= ni
    base = node_off[mesh_of_node]
    left, right = nodes["left"].astype(np.int64), nodes["right"].astype(np.int64)
    # leaves
    assert (right[is_leaf] == pkg.INVALID).all()
    prim = left[is_leaf]; leaf_mesh = mesh_of_node[is_leaf]
    assert (prim < counts[leaf_mesh]).all()
    gprim = out_off[leaf_mesh] + prim
    assert np.array_equal(np.bincount(gprim, minlength=total), np.ones(total, dtype=np.int64)), "leaf primitives are not a permutation per mesh"
    assert np.array_equal(prim, whole["sorted_vals"].astype(np.int64)), "leaf order is not the sorted order"
    lb = whole["prim_aabbs"][gprim]
    assert nodes["min"][is_leaf].tobytes() == lb["min"].tobytes() and nodes["max"][is_leaf].tobytes() == lb["max"].tobytes()
    # internal nodes
    inner = ~is_leaf
    span = (2 * counts - 1)[mesh_of_node]
    assert (left[inner] < span[inner]).all() and (right[inner] < span[inner]).all()
    gl, gr = base[inner] + left[inner], base[inner] + right[inner]
    assert np.array_equal(nodes["min"][inner], np.minimum(nodes["min"][gl], nodes["min"][gr])) and np.array_equal(nodes["max"][inner], np.maximum(nodes["max"][gl], nodes["max"][gr]))
    refs = np.bincount(np.concatenate([gl, gr]), minlength=N)
    groot = node_off + whole["roots"].astype(np.int64)
    assert (whole["roots"] < counts - 1).all()
    want = np.ones(N, dtype=np.int64); want[groot] = 0
    assert np.array_equal(refs, want), "a node has no parent or several"
    seen = np.zeros(N, dtype=bool); frontier = groot
    for _ in range(int(counts.max()) + 1):                                  # level by level from the roots: everything is reached (no detached cycle)
        seen[frontier] = True
        f = frontier[~is_leaf[frontier]]
        if len(f) == 0:
            break
        frontier = np.concatenate([node_off[mesh_of_node[f]] + left[f], node_off[mesh_of_node[f]] + right[f]])
    assert seen.all(), "nodes that the root does not reach"
    # root box == extent
    assert nodes["min"][groot].tobytes() == whole["scenes"]["min"].tobytes() and nodes["max"][groot].tobytes() == whole["scenes"]["max"].tobytes()
    # sorted order
    mesh_of_pos = np.repeat(np.arange(M), counts)
    k = whole["sorted_keys"].astype(np.int64); v = whole["sorted_vals"].astype(np.int64)
    same_mesh = mesh_of_pos[1:] == mesh_of_pos[:-1]
    assert ((k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (v[1:] > v[:-1])))[same_mesh].all(), "keys are not ascending {key, index}"


@pytest.mark.parametrize("algo", [0, 1])
def test_twenty_thousand_meshes(pkg, ctx, ctx2, algo):
    rng = np.random.default_rng(2024)
    counts = rng.integers(2, 97, 20_000)
    total = int(counts.sum())
    src = no_negzero(pkg.meshgen.uniform(total, 9))
    # every mesh its own little cloud: a slice of the big mesh, moved and scaled per mesh
    d = ctx.upload(src)
    firsts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    ranges = np.stack([firsts, counts], axis=1)
    try:
        mt = ctx.build_many((d, ranges), algo=algo, n_tris=total)
        ctx.synchronize()
        whole = mt.download_all()
        validate_structure(pkg, mt, whole)
        sample = np.random.default_rng(5).choice(20_000, 256, replace=False)
        sample[:4] = [0, 19_999, int(np.argmax(counts == 64)), int(np.argmax(counts == 65))]
        check_against_alone(pkg, ctx2, mt, whole, sample.tolist())
        mt.free()
        one = ctx.build_many((d, [[5, 77]]), algo=algo, n_tris=total)       # n_meshes == 1
        ctx.synchronize()
        w1 = one.download_all()
        check_against_alone(pkg, ctx2, one, w1, [0])
        one.free()
    finally:
        d.free()


# ---- 3. independence, guard words -----------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """a device array with `pad` guard bytes on either side, everything pre-filled with FILL"""

    def __init__(self, pkg, ctx, nbytes, pad=256):
        self.pkg, self.ctx, self.nbytes, self.pad = pkg, ctx, nbytes, pad
        self.buf = ctx.alloc(nbytes + 2 * pad)
        self.buf.upload(np.full(nbytes + 2 * pad, FILL, dtype=np.uint8))
        self.ptr = self.buf.ptr + pad

    def read(self):
        a = self.buf.download(np.uint8, self.nbytes + 2 * self.pad)
        return a[:self.pad], a[self.pad:self.pad + self.nbytes], a[self.pad + self.nbytes:]

    def free(self):
        self.buf.free()


def raw_many(pkg, ctx, algo, inp, ranges, n_tris, keys=True):
    """bvh_build_many through the C ABI into guarded, pre-filled arrays: (rc, [payload bytes of the six arrays], guards intact?)"""
    rg = pkg.many_check_ranges(ranges, n_tris, inp.tri_format)
    _, _, total = pkg.many_layout(rg["count"]); n = len(rg)
    sizes = [(2 * total - n) * 32, total * 24, n * 24, n * 4, total * 4, total * 4]
    g = [Guarded(pkg, ctx, s) for s in sizes]
    out = pkg.ManyOut(g[0].ptr, g[1].ptr, g[2].ptr, g[3].ptr, g[4].ptr if keys else None, g[5].ptr if keys else None)
    rc = pkg.lib().bvh_build_many(ctx.handle, algo, C.byref(inp), n_tris, rg.ctypes.data, n, C.byref(out), None)
    ctx.synchronize()
    parts = [x.read() for x in g]
    intact = all((lo == FILL).all() and (hi == FILL).all() for lo, _, hi in parts)
    for x in g:
        x.free()
    return rc, [p[1].tobytes() for p in parts], intact


@pytest.mark.parametrize("algo", [0, 1])
def test_independent_of_position_batch_and_call(pkg, ctx, algo):
    probe = {c: cut(pkg, "sponza", 77, c) for c in (50, 200, 600)}         # one mesh per path
    filler = [cut(pkg, "uniform", 61 * k, c) for k, c in enumerate([3, 64, 65, 130, 512, 9, 40])]
    batches = [list(probe.values()) + filler, filler[:3] + [probe[600], probe[50]] + filler[3:] + [probe[200]], [probe[200]] + filler[::-1] + [probe[50], probe[600]]]
    where = [{50: 0, 200: 1, 600: 2}, {600: 3, 50: 4, 200: len(filler) + 2}, {200: 0, 50: len(filler) + 1, 600: len(filler) + 2}]
    seen = {}
    for b, (meshes, pos) in enumerate(zip(batches, where)):
        inp, ranges, n_tris, bufs = device_input(pkg, ctx, meshes, pkg.TRI_PADDED64, gap=b)
        host_in = bufs[0].download(np.uint8, bufs[0].nbytes)
        rc, arrays, intact = raw_many(pkg, ctx, algo, inp, ranges, n_tris)
        assert rc == 0 and intact, "guard words around an output array were written"
        rc2, arrays2, intact2 = raw_many(pkg, ctx, algo, inp, ranges, n_tris)
        assert rc2 == 0 and intact2 and arrays == arrays2, "two identical calls differ"
        assert bufs[0].download(np.uint8, bufs[0].nbytes).tobytes() == host_in.tobytes(), "the input was written"
        counts = [len(t) for t in meshes]
        out_off, node_off, _ = pkg.many_layout(counts)
        for c, m in pos.items():
            assert counts[m] == c
            o, no = int(out_off[m]), int(node_off[m])
            sl = (arrays[0][32 * no:32 * (no + 2 * c - 1)], arrays[1][24 * o:24 * (o + c)], arrays[2][24 * m:24 * (m + 1)], arrays[3][4 * m:4 * (m + 1)],
                  arrays[4][4 * o:4 * (o + c)], arrays[5][4 * o:4 * (o + c)])
            assert seen.setdefault(c, sl) == sl, f"the {c}-triangle mesh depends on its place in batch {b}"
        for x in bufs:
            x.free()
    # without the optional arrays: the others are the same bytes, the optional ones stay untouched
    inp, ranges, n_tris, bufs = device_input(pkg, ctx, batches[0], pkg.TRI_PADDED64)
    rc, a, ok = raw_many(pkg, ctx, algo, inp, ranges, n_tris)
    rc2, b2, ok2 = raw_many(pkg, ctx, algo, inp, ranges, n_tris, keys=False)
    assert rc == 0 and rc2 == 0 and ok and ok2 and a[:4] == b2[:4] and set(b2[4]) == {FILL} and set(b2[5]) == {FILL}
    for x in bufs:
        x.free()


# ---- 4. consumers ---------------------------------------------------------------------------------------------------------------------------------------------
def rays_at(pkg, tris, m, seed):
    rng = np.random.default_rng(seed)
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    o = lo - 0.5 * ext + rng.random((m, 3)) * 2.0 * ext
    k = rng.integers(0, len(tris), m)                                       # three in four aim at a point inside some triangle (small meshes are mostly empty space)
    w = rng.dirichlet([1.0, 1.0, 1.0], m)
    inside = w[:, :1] * tris["v1"][k] + w[:, 1:2] * tris["v2"][k] + w[:, 2:] * tris["v3"][k]
    target = np.where((np.arange(m) % 4 != 0)[:, None], inside, lo + rng.random((m, 3)) * ext)
    dd = target - o
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    r = np.zeros(m, dtype=pkg.RAY)
    r["origin"] = o.astype(F32); r["direction"] = dd.astype(F32); r["tmin"] = 0.0; r["tmax"] = F32(3.0e38)
    return r


def consumer_meshes(pkg):
    return [cut(pkg, ["uniform", "sponza", "bunny"][k % 3], 97 * k, c) for k, c in enumerate([40, 64, 65, 300, 512, 640])]


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("algo", [0, 1])
def test_queries_on_slices_answer_as_single_trees(pkg, ctx, ctx2, algo, fmt):
    meshes = consumer_meshes(pkg)
    inp, ranges, n_tris, bufs = device_input(pkg, ctx, meshes, fmt, gap=4)
    mt = many(pkg, ctx, algo, inp, ranges, n_tris)
    ctx.reserve(1024); ctx2.reserve(1024)
    try:
        ctx.synchronize()
        for m, tris in enumerate(meshes):
            single = pkg.BUILDERS[algo]().build(ctx2, tris)
            rays = rays_at(pkg, tris, 4096, 10 + m)
            pts = np.zeros(1024, dtype=pkg.POINT_QUERY)
            pts["point"] = rays["origin"][:1024]; pts["radius"] = np.inf
            want_hits, want_pts = single.intersect(rays), single.closest_point(pts)
            assert (want_hits["prim"] != pkg.INVALID).sum() > 100
            t = mt.tris(m)
            b = mt.builder(m)
            kw = dict(tris=t.d_tris, vertices=t.d_vertices, indices=t.d_indices, n_vertices=t.n_vertices, tri_format=fmt)
            assert b.intersect(rays, **kw).tobytes() == want_hits.tobytes(), f"mesh {m}: bvh_intersect on the slice differs"
            assert b.closest_point(pts, **kw).tobytes() == want_pts.tobytes(), f"mesh {m}: bvh_closest_point on the slice differs"
            if fmt == pkg.TRI_PADDED64:                                     # the slice's own d_tris names its triangles
                assert b.intersect(rays).tobytes() == want_hits.tobytes()
    finally:
        mt.free()
        for x in bufs:
            x.free()


def test_scene_over_many_trees(pkg, ctx, ctx2):
    rng = np.random.default_rng(64)
    counts = rng.integers(8, 200, 64)
    meshes = [cut(pkg, "uniform", 53 * k, int(c)) for k, c in enumerate(counts)]
    mt = ctx.build_many(meshes, algo=pkg.ALGO_TWOPASS)
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
            b = pkg.TwoPassLbvh().build(ctx2, tris)
            dn, dt = ctx2.alloc((2 * n - 1) * 32), ctx2.upload(tris); keep += [dn, dt]
            assert pkg.lib().bvh_dev_copy(ctx2.handle, dn.ptr, b.result.d_nodes, (2 * n - 1) * 32) == 0
            r = pkg.Result.from_buffer_copy(b.result)
            r.d_nodes, r.d_tris, r.d_prim_aabbs, r.d_sorted_keys, r.d_sorted_vals, r.d_scene_extent, r.d_morton_keys = dn.ptr, dt.ptr, None, None, None, None, None
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


@pytest.mark.parametrize("algo", [0, 1])
def test_refit_of_a_slice(pkg, ctx, ctx2, algo):
    meshes = consumer_meshes(pkg)
    mt = ctx.build_many(meshes, algo=algo)
    ctx.reserve(1024); ctx2.reserve(1024)
    rng = np.random.default_rng(8)
    try:
        ctx.synchronize()
        before = mt.download_all()
        for m in (1, 3, 5):
            tris = meshes[m]; n = len(tris)
            b = mt.builder(m)
            d_same = ctx.upload(tris)
            b.refit_ex(tris=d_same)                                         # the triangles the tree was built from: the build's arrays again
            ctx.synchronize()
            assert_same_tree(mt.download(m), slices(mt, before, m), f"refit of mesh {m} with its own triangles")
            moved = tris.copy()
            for f in ("v1", "v2", "v3"):
                moved[f] = (moved[f] + rng.normal(0.0, 0.05, moved[f].shape)).astype(F32)
            moved = no_negzero(moved)
            d_moved = ctx.upload(moved)
            b.refit_ex(tris=d_moved)
            ctx.synchronize()
            got = mt.download(m)
            rebuilt = alone(pkg, ctx2, algo, pkg.BuildInput(0, 30, d_moved.ptr, None, None, 0, 0), n)      # a rebuild's stage E boxes and extent
            assert got["prim_aabbs"].tobytes() == rebuilt["prim_aabbs"].tobytes()
            assert np.array_equal(got["scene"]["min"], rebuilt["scene"]["min"]) and np.array_equal(got["scene"]["max"], rebuilt["scene"]["max"])
            nodes, old = got["nodes"], slices(mt, before, m)["nodes"]
            assert np.array_equal(nodes["left"], old["left"]) and np.array_equal(nodes["right"], old["right"])
            leaf = nodes[n - 1:]
            assert leaf["min"].tobytes() == rebuilt["prim_aabbs"]["min"][leaf["left"]].tobytes() and leaf["max"].tobytes() == rebuilt["prim_aabbs"]["max"][leaf["left"]].tobytes()
            inner = nodes[:n - 1]
            assert np.array_equal(inner["min"], np.minimum(nodes["min"][inner["left"]], nodes["min"][inner["right"]]))
            assert np.array_equal(inner["max"], np.maximum(nodes["max"][inner["left"]], nodes["max"][inner["right"]]))
            root = nodes[got["root"]]
            assert np.array_equal(root["min"], rebuilt["scene"]["min"][0]) and np.array_equal(root["max"], rebuilt["scene"]["max"][0])
            d_same.free(); d_moved.free()
        after = mt.download_all()                                           # the other meshes' slices were not touched
        for m in (0, 2, 4):
            assert_same_tree(slices(mt, after, m), slices(mt, before, m), f"mesh {m} after its neighbours' refits")
    finally:
        mt.free()


def test_kernel_times_name_both_kernels(pkg):
    c = pkg.Context(0)
    try:
        c.set_profiling(2)
        meshes = [cut(pkg, "uniform", 10 * k, n) for k, n in enumerate([10, 64, 100, 256, 400])]
        mt = c.build_many(meshes)
        c.synchronize()
        times = c.kernel_times()
        assert times["k_many_wave"][1] == 1 and times["k_many_block"][1] == 3, times
        assert mt.timings.sampled == 1 and mt.timings.ms_build > 0 and mt.timings.ms_total == mt.timings.ms_build
        mt.free()
    finally:
        c.close()


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(pkg, ctx):
    L = pkg.lib()
    meshes = [cut(pkg, "uniform", 0, c) for c in (12, 100, 8)]
    inp, ranges, n_tris, bufs = device_input(pkg, ctx, meshes, pkg.TRI_PADDED64)
    packed, pranges, pn, pbufs = device_input(pkg, ctx, meshes, pkg.TRI_PACKED36)
    indexed, iranges, i_n, ibufs = device_input(pkg, ctx, meshes, pkg.TRI_INDEXED)
    rg = pkg.many_check_ranges(ranges, n_tris)
    _, _, total = pkg.many_layout(rg["count"]); n = len(rg)
    sizes = [(2 * total - n) * 32, total * 24, n * 24, n * 4, total * 4, total * 4]
    g = [Guarded(pkg, ctx, s) for s in sizes]

    def out_of(ptrs):
        return pkg.ManyOut(*ptrs)
    good = [x.ptr for x in g]

    def call(algo=0, inp_=inp, n_tris_=n_tris, rg_=rg, n_=n, out=None, ctx_=ctx.handle, ranges_null=False, in_null=False, out_null=False):
        o = out_of(good) if out is None else out
        return L.bvh_build_many(ctx_, algo, None if in_null else C.byref(inp_), n_tris_, None if ranges_null else rg_.ctypes.data, n_, None if out_null else C.byref(o), None)

    def ranges_of(rows):
        a = np.empty(len(rows), dtype=pkg.MESH_RANGE)
        a["first"], a["count"] = [r[0] for r in rows], [r[1] for r in rows]
        return a
    bad_in = lambda **kw: pkg.BuildInput(*[kw.get(k, getattr(inp, k)) for k in ("tri_format", "morton_bits", "d_tris", "d_vertices", "d_indices", "n_vertices", "reserved")])
    cases = {
        "NULL ctx": call(ctx_=None), "NULL in": call(in_null=True), "NULL ranges": call(ranges_null=True), "NULL out": call(out_null=True),
        "NULL d_nodes": call(out=out_of([None] + good[1:])), "NULL d_prim_aabbs": call(out=out_of(good[:1] + [None] + good[2:])),
        "NULL d_scene_extents": call(out=out_of(good[:2] + [None] + good[3:])), "NULL d_roots": call(out=out_of(good[:3] + [None] + good[4:])),
        "PLOC++": call(algo=2), "HPLOC": call(algo=3), "algo 7": call(algo=7),
        "60-bit codes": call(inp_=bad_in(morton_bits=60)), "format 3": call(inp_=bad_in(tri_format=3)), "NULL d_tris": call(inp_=bad_in(d_tris=None)),
        "unaligned PACKED36": call(inp_=pkg.BuildInput(1, 30, packed.d_tris + 4, None, None, 0, 0), n_tris_=pn - 1, rg_=pkg.many_check_ranges(pranges, pn, 1)),
        "INDEXED without vertices": call(inp_=pkg.BuildInput(2, 30, None, None, indexed.d_indices, indexed.n_vertices, 0), n_tris_=i_n),
        "INDEXED with n_vertices 0": call(inp_=pkg.BuildInput(2, 30, None, indexed.d_vertices, indexed.d_indices, 0, 0), n_tris_=i_n),
        "no mesh": call(n_=0),
        "count 1": call(rg_=ranges_of([(0, 12), (12, 1), (13, 107)])), "count 0": call(rg_=ranges_of([(0, 12), (12, 0), (12, 108)])),
        "past n_tris": call(rg_=ranges_of([(0, 12), (12, 100), (113, 8)])), "first + count wraps": call(rg_=ranges_of([(0, 12), (12, 100), (0xFFFFFFFC, 8)])),
        "misaligned PACKED36 first": call(inp_=packed, n_tris_=pn, rg_=ranges_of([(0, 12), (14, 100), (116, 8)])),
        "total 2^30": call(n_tris_=1 << 31, rg_=ranges_of([(0, 1 << 29), (0, 1 << 29)]), n_=2),      # (rejected on the host: no array is touched)
        "nodes overlap boxes": call(out=out_of([good[0], good[0] + 64] + good[2:])), "keys overlap vals": call(out=out_of(good[:4] + [good[4], good[4] + 8])),
        "roots inside nodes": call(out=out_of(good[:3] + [good[0] + 32] + good[4:])), "boxes are the input": call(out=out_of([good[0], inp.d_tris] + good[2:])),
        "nodes end in the input": call(out=out_of([inp.d_tris - sizes[0] + 32] + good[1:])),
        "vals overlap the indices": call(inp_=indexed, n_tris_=i_n, rg_=pkg.many_check_ranges(iranges, i_n, 2), out=out_of(good[:5] + [indexed.d_indices + 4])),
        "scenes overlap the vertices": call(inp_=indexed, n_tris_=i_n, rg_=pkg.many_check_ranges(iranges, i_n, 2), out=out_of(good[:2] + [indexed.d_vertices] + good[3:])),
    }
    ctx.synchronize()
    wrong = {k: v for k, v in cases.items() if v != E_INVALID}
    assert not wrong, wrong
    for x in g:
        lo, mid, hi = x.read()
        assert (lo == FILL).all() and (mid == FILL).all() and (hi == FILL).all(), "a rejected call wrote to an output array"
    assert call() == 0                                                      # ... and the same arguments, unbroken, build
    ctx.synchronize()
    assert not (g[0].read()[1] == FILL).all()
    for x in g + bufs + pbufs + ibufs:
        x.free()
