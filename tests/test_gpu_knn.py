"""bvh_knn on the GPU: the k-nearest lists of every builder, both node layouts and all three triangle formats against the numpy brute force
(tests/test_knn.py), k = 1 against bvh_closest_point, point clouds as degenerate triangles, the stackless pass on trees deeper than the short stack, queries
after a refit, an optimise and a rebuild, large sizes, buffer hygiene and errors."""
import ctypes as C

import numpy as np
import pytest

from test_knn import E_INVALID, below, knn_brute_force, recompute_knn, truncate
from test_gpu_point_query import MESHES, first_descent_pushes, make_points
from test_gpu_point_query import query as closest_query
from test_gpu_query import caterpillar, lbvh_result, mesh
from test_gpu_refit import jitter, no_negzero

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

KS = (1, 2, 8, 32)
_REF = {}


def reference(pkg, name, k):
    """(points, brute force) per mesh and k, computed once (for k = 32, the smaller k cut from it); the points are the point-query tests' own"""
    if (name, k) not in _REF:
        tris = mesh(pkg, name)
        if k == 32:
            pts = make_points(pkg, tris, 1536, 11 + len(tris))
            _REF[(name, k)] = (pts, knn_brute_force(pkg, pts, tris, k))
        else:
            pts, bf = reference(pkg, name, 32)
            _REF[(name, k)] = (pts, truncate(pkg, bf, k))
    return _REF[(name, k)]


def knn(pkg, ctx, result, pts, k, inp=None, with_counts=True):
    d_pts = ctx.upload(pts)
    hits = ctx.alloc(len(pts) * k * 8)
    counts = ctx.alloc(len(pts) * 4) if with_counts else None
    try:
        rc = pkg.lib().bvh_knn(ctx.handle, C.byref(result), C.byref(inp) if inp is not None else None, d_pts.ptr, len(pts), k, hits.ptr,
                               counts.ptr if with_counts else None)
        assert rc == 0, rc
        return hits.download(pkg.KNN_HIT, len(pts) * k).reshape(len(pts), k), (counts.download(np.uint32, len(pts)) if with_counts else None)
    finally:
        d_pts.free(); hits.free()
        if counts is not None:
            counts.free()


def rows_equal(a, b):
    k = a.shape[1]
    return (a.view(np.uint8).reshape(len(a), k * 8) == b.view(np.uint8).reshape(len(b), k * 8)).all(axis=1)


def check_exact(pkg, pts, tris, bf, hits, counts, what):
    well = bf["well"]
    assert well.mean() >= 0.99, f"{what}: only {well.mean():.4f} of the queries are well-conditioned"
    same = rows_equal(hits, bf["hits"])
    assert same[well].all(), f"{what}: lists differ on {np.count_nonzero(~same & well)} well-conditioned queries (first {np.nonzero(~same & well)[0][:6]})"
    assert (counts == bf["counts"])[well].all(), f"{what}: counts differ"
    # every query: entries are accepted candidates with bit-equal dist2, strictly ascending, the padding exact, counts the lengths; nothing below the truth
    assert recompute_knn(pkg, pts, tris, hits, counts).all(), f"{what}: a list does not recompute"
    assert not below(pkg, hits, bf["hits"]).any(), f"{what}: a list below the brute force"


@pytest.mark.parametrize("name", MESHES)
def test_exact_against_brute_force(pkg, ctx, name):
    tris = mesh(pkg, name)
    per = {}
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        keep = []
        results = [("as built", b.result)]
        if b.result.layout == 1:
            results.append(("lbvh layout", lbvh_result(pkg, ctx, b, keep)))
        for k in KS:
            pts, bf = reference(pkg, name, k)
            for label, res in results:
                h, c = knn(pkg, ctx, res, pts, k)
                check_exact(pkg, pts, tris, bf, h, c, f"{name} k {k} algo {algo} {label}")
                per.setdefault((algo, k), h)
            bh, bc = b.knn(pts, k)                                    # the Python binding, host records
            assert bh.tobytes() == per[(algo, k)].tobytes() and bh.shape == (len(pts), k) and bc.dtype == np.uint32
            assert (bc == (bh["prim"] != pkg.INVALID).sum(axis=1)).all()
        for x in keep:
            x.free()
    for k in KS:
        pts, bf = reference(pkg, name, k)
        if len(tris) > k:
            assert (bf["counts"] == k).any()
        assert (bf["counts"] == 0).any()
        well = bf["well"]
        for algo in (1, 2, 3):
            assert per[(algo, k)][well].tobytes() == per[(0, k)][well].tobytes(), f"{name} k {k}: builders {algo} and 0 differ"


def test_meshes_exercise_partial_lists_and_ties_at_place_k(pkg):
    """what the brute force alone says of the test points: partial lists on every larger mesh, exact ties at place k on the Cornell box and the Sponza-like mesh"""
    for name, k in (("cornell382", 8), ("cornell382", 32), ("sponza_20000", 8)):
        pts, bf = reference(pkg, name, k)
        partial = (bf["counts"] > 0) & (bf["counts"] < k)
        assert partial.sum() >= 100 and bf["kth_tie"].sum() >= 4 and bf["well"].all(), (name, k, int(partial.sum()), int(bf["kth_tie"].sum()))


@pytest.mark.parametrize("name", ["uniform_1000", "sponza_20000", "cornell382"])
def test_k1_equals_closest_point(pkg, ctx, name):
    tris = mesh(pkg, name)
    pts, _ = reference(pkg, name, 1)
    for algo in (0, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        h, c = knn(pkg, ctx, b.result, pts, 1)
        cp = closest_query(pkg, ctx, b.result, pts, pkg.QUERY_CLOSEST)
        assert h["dist2"][:, 0].tobytes() == cp["dist2"].tobytes() and h["prim"][:, 0].tobytes() == cp["prim"].tobytes()
        assert (c == (cp["prim"] != pkg.INVALID)).all()


@pytest.mark.parametrize("name", ["uniform_1000", "sponza_20000", "cornell382"])
def test_formats_give_identical_answers(pkg, ctx, name):
    tris = mesh(pkg, name); n = len(tris)
    k = 8
    pts, bf = reference(pkg, name, k)
    b = pkg.HPLOC().build(ctx, tris)
    packed = np.ascontiguousarray(np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1).astype(np.float32).reshape(n, 9))
    verts = packed.reshape(-1, 3)
    uniq, inv = np.unique(verts, axis=0, return_inverse=True)
    idx = inv.reshape(-1).astype(np.uint32)
    d_p, d_v, d_i = ctx.upload(packed), ctx.upload(np.ascontiguousarray(uniq.astype(np.float32))), ctx.upload(idx)
    try:
        base, bc = knn(pkg, ctx, b.result, pts, k)
        p, pc = knn(pkg, ctx, b.result, pts, k, pkg.BuildInput(pkg.TRI_PACKED36, 30, d_p.ptr, None, None, 0, 0))
        i, ic = knn(pkg, ctx, b.result, pts, k, pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, len(uniq), 0))
        assert base.tobytes() == p.tobytes() == i.tobytes() and bc.tobytes() == pc.tobytes() == ic.tobytes()
        bh, _ = b.knn(pts, k, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED)
        assert bh.tobytes() == base.tobytes()
        # a tree built FROM indexed input answers the same
        bi = pkg.PLOCNew().build_ex(ctx, n, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED)
        got, _ = bi.knn(pts, k, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED)
        assert got[bf["well"]].tobytes() == bf["hits"][bf["well"]].tobytes()
    finally:
        for x in (d_p, d_v, d_i):
            x.free()


def test_binding_fills_radius_for_plain_points(pkg, ctx):
    tris = mesh(pkg, "sponza_1000")
    pts, _ = reference(pkg, "sponza_1000", 8)
    xyz = np.ascontiguousarray(pts["point"])
    b = pkg.SinglePassLbvh().build(ctx, tris)
    for radius in (None, 0.5):
        rec = np.zeros(len(xyz), dtype=pkg.POINT_QUERY); rec["point"] = xyz; rec["radius"] = np.inf if radius is None else radius
        (h0, c0), (h1, c1) = b.knn(xyz, 8, radius=radius), b.knn(rec, 8)
        assert h0.tobytes() == h1.tobytes() and c0.tobytes() == c1.tobytes()
    with pytest.raises(pkg.BvhError):
        b.knn(pts, 8, radius=1.0)                                 # POINT_QUERY records carry their own radius
    with pytest.raises(pkg.BvhError):
        b.knn(pts, 33)


def test_point_cloud_as_degenerate_packed_triangles(pkg, ctx):
    rng = np.random.default_rng(77)
    n, m, k = 20_000, 4096, 16
    cloud = rng.random((n, 3)).astype(np.float32)
    cloud[rng.integers(0, n, 50)] = cloud[rng.integers(0, n, 50)]   # some duplicate points: exact ties, broken by index
    packed = np.ascontiguousarray(np.repeat(cloud, 3, axis=0).reshape(n, 9))
    d_p = ctx.upload(packed)
    try:
        b = pkg.HPLOC().build_ex(ctx, n, tris=d_p, tri_format=pkg.TRI_PACKED36)
        q = rng.random((m, 3)).astype(np.float32)
        q[:64] = cloud[rng.integers(0, n, 64)]                       # queries on cloud points
        h, c = b.knn(q, k, tris=d_p, tri_format=pkg.TRI_PACKED36)
        assert (c == k).all()
        for s in range(0, m, 256):
            d = cloud[None] - q[s:s + 256, None]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            order = np.lexsort((np.broadcast_to(np.arange(n), d2.shape), d2), axis=1)[:, :k]
            assert h["prim"][s:s + 256].tobytes() == order.astype(np.uint32).tobytes(), s
            assert h["dist2"][s:s + 256].tobytes() == np.take_along_axis(d2, order, axis=1).tobytes(), s
    finally:
        d_p.free()


@pytest.mark.parametrize("H", [70, 250])
def test_deep_tree_takes_the_stackless_pass(pkg, H):
    tris, nodes, root, n = caterpillar(pkg, H, 5 + H)
    rng = np.random.default_rng(H)
    m, k = 300, 8
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    pts["point"] = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-3, -0.5, m)], axis=1)
    pts["point"][: m // 6, 2] = 0.0                             # on the face at z = 0
    pts["radius"] = np.inf
    pts["radius"][m // 2: 3 * m // 4] = 5.0                     # the far side nodes are culled: no push, the short stack suffices
    pts["point"][3 * m // 4:, 2] = rng.uniform(1000, 1000 + 2 * H, m - 3 * m // 4)     # among the far triangles
    assert max(first_descent_pushes(nodes, root, n - 1, pts["point"][j].astype(np.float64)) for j in range(m // 2)) > 64
    bf = knn_brute_force(pkg, pts, tris, k)
    assert bf["well"].all() and (bf["counts"] == k).any() and (bf["counts"] == 2).any()
    c = pkg.Context(0)
    try:
        c.reserve(n)
        d_nodes, d_tris = c.upload(nodes), c.upload(tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        c.set_profiling(2)
        h, cnt = knn(pkg, c, r, pts, k)
        kt = c.kernel_times()
        c.set_profiling(0)
        assert {"k_knn", "k_knn_deep", "k_refit_plan"} <= set(kt)
        assert h.tobytes() == bf["hits"].tobytes() and cnt.tobytes() == bf["counts"].tobytes()
        h32, cnt32 = knn(pkg, c, r, pts, 32)
        bf32 = knn_brute_force(pkg, pts, tris, 32)
        assert h32.tobytes() == bf32["hits"].tobytes() and cnt32.tobytes() == bf32["counts"].tobytes()
        d_nodes.free(); d_tris.free()
    finally:
        c.close()


_MOVED = {}


def moved_reference(pkg, key, tris, seed, k):
    """(points, brute force) of the refit test's two meshes: the same for every builder, computed once"""
    if key not in _MOVED:
        pts = make_points(pkg, tris, 1024, seed)
        _MOVED[key] = (pts, knn_brute_force(pkg, pts, tris, k))
    return _MOVED[key]


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_query_after_refit_optimize_and_rebuild(pkg, algo):
    a = mesh(pkg, "uniform_20000"); moved = jitter(a, 19, 2e-3)
    other = mesh(pkg, "sponza_20000")
    k = 8
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        pts, bf = moved_reference(pkg, "moved", moved, 8, k)
        b.knn(pts, k)                                         # (the plan of the ctx's own tree is made here and kept)
        b.refit(moved)
        check_exact(pkg, pts, moved, bf, *b.knn(pts, k), f"refit algo {algo}")
        b.optimize(3)
        check_exact(pkg, pts, moved, bf, *b.knn(pts, k), f"optimize algo {algo}")
        b2 = pkg.BUILDERS[algo]().build(c, other)
        pts2, bf2 = moved_reference(pkg, "other", other, 9, k)
        check_exact(pkg, pts2, other, bf2, *b2.knn(pts2, k), f"rebuild algo {algo}")
    finally:
        c.close()


@pytest.mark.parametrize("name,n", [("sponza", 262_144), ("uniform", 2_000_000)])
def test_large_trees(pkg, ctx, name, n):
    tris = no_negzero(pkg.meshgen.sponza_like(n, 3) if name == "sponza" else pkg.meshgen.uniform(n, 9))
    m, k = 1_000_003, 8
    pts = make_points(pkg, tris, m, 23)
    res = {}
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        h, c = b.knn(pts, k)
        assert recompute_knn(pkg, pts, tris, h, c).all()
        res[algo] = h
    for algo in (1, 2, 3):
        same = rows_equal(res[algo], res[0])
        assert same.mean() >= 0.999, f"builders {algo} / 0 agree on {same.mean():.5f}"
    sample = np.random.default_rng(1).choice(m, 64, replace=False)
    bf = knn_brute_force(pkg, pts[sample], tris, k)
    well = bf["well"]
    assert well.mean() >= 0.95
    for algo in (0, 3):
        assert res[algo][sample][well].tobytes() == bf["hits"][well].tobytes()


def test_buffers_untouched_outside_the_answers(pkg, ctx):
    tris = mesh(pkg, "uniform_1000")
    b = pkg.HPLOC().build(ctx, tris)
    m, extra = 1000, 37                                       # (1000 is no multiple of the 64 queries of a workgroup)
    pts = make_points(pkg, tris, m, 3)
    d_pts = ctx.upload(pts)
    L = pkg.lib()
    try:
        for k in (1, 5, 8, 13, 32):
            s_hits = np.frombuffer(np.full((m * k + extra) * 8, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.KNN_HIT)
            s_cnt = np.full(m + extra, 0xA5A5A5A5, dtype=np.uint32)
            hits, counts = ctx.upload(s_hits), ctx.upload(s_cnt)
            try:
                assert L.bvh_knn(ctx.handle, C.byref(b.result), None, d_pts.ptr, m, k, hits.ptr, counts.ptr) == 0
                out, cnt = hits.download(pkg.KNN_HIT, m * k + extra), counts.download(np.uint32, m + extra)
                assert out[m * k:].tobytes() == s_hits[m * k:].tobytes() and cnt[m:].tobytes() == s_cnt[m:].tobytes()
                assert recompute_knn(pkg, pts, tris, out[: m * k].reshape(m, k), cnt[:m]).all()
                assert d_pts.download(pkg.POINT_QUERY, m).tobytes() == pts.tobytes()
                # d_counts == NULL: the same lists, the counts array untouched
                hits.upload(s_hits); counts.upload(s_cnt)
                assert L.bvh_knn(ctx.handle, C.byref(b.result), None, d_pts.ptr, m, k, hits.ptr, None) == 0
                assert hits.download(pkg.KNN_HIT, m * k + extra).tobytes() == out.tobytes()
                assert counts.download(np.uint32, m + extra).tobytes() == s_cnt.tobytes()
                # n_points == 0: nothing touched
                hits.upload(s_hits)
                assert L.bvh_knn(ctx.handle, C.byref(b.result), None, d_pts.ptr, 0, k, hits.ptr, counts.ptr) == 0
                assert hits.download(pkg.KNN_HIT, m * k + extra).tobytes() == s_hits.tobytes()
                assert counts.download(np.uint32, m + extra).tobytes() == s_cnt.tobytes()
            finally:
                hits.free(); counts.free()
    finally:
        d_pts.free()


def test_fewer_triangles_than_k(pkg, ctx):
    tris = mesh(pkg, "uniform_3")
    pts, bf = reference(pkg, "uniform_3", 32)
    assert bf["counts"].max() == 3
    for algo in (0, 1, 2, 3):
        h, c = pkg.BUILDERS[algo]().build(ctx, tris).knn(pts, 32)
        assert h.tobytes() == bf["hits"].tobytes() and c.tobytes() == bf["counts"].tobytes()


def test_errors_write_nothing(pkg):
    tris = mesh(pkg, "uniform_1000"); n = len(tris)
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        m, k = 256, 8
        pts = make_points(pkg, tris, m, 4)
        d_pts = c.upload(pts)
        s_hits = np.frombuffer(np.full(m * k * 8, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.KNN_HIT)
        s_cnt = np.full(m, 0x5A5A5A5A, dtype=np.uint32)
        hits, counts = c.upload(s_hits), c.upload(s_cnt)
        L = pkg.lib()

        def call(res=b.result, inp=None, p=d_pts.ptr, m_=m, k_=k, h=hits.ptr, cn=counts.ptr, ctx=c.handle):
            return L.bvh_knn(ctx, C.byref(res) if res is not None else None, C.byref(inp) if inp is not None else None, p, m_, k_, h, cn)

        def variant(**kw):
            r = pkg.Result.from_buffer_copy(b.result)
            for key, v in kw.items():
                setattr(r, key, v)
            return r
        cases = {
            "null ctx": call(ctx=None), "null tree": call(res=None), "null points": call(p=None), "null hits": call(h=None),
            "n_leaves 1": call(res=variant(n_leaves=1)), "layout 2": call(res=variant(layout=2)), "null nodes": call(res=variant(d_nodes=None)),
            "layout 1 without leaves": call(res=variant(d_leaves=None)), "root not internal": call(res=variant(root=n - 1)),
            "no triangles": call(res=variant(d_tris=None)), "bad format": call(inp=pkg.BuildInput(7, 30, b.result.d_tris, None, None, 0, 0)),
            "packed unaligned": call(inp=pkg.BuildInput(pkg.TRI_PACKED36, 30, b.result.d_tris + 4, None, None, 0, 0)),
            "indexed without vertices": call(inp=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, None, b.result.d_tris, 3, 0)),
            "k 0": call(k_=0), "k 33": call(k_=33), "k 2^32 - 1": call(k_=0xFFFFFFFF),
            "hits over points": call(h=d_pts.ptr + 16), "points over hits": call(p=hits.ptr + 8 * (m * k - 1)),
            "counts over points": call(cn=d_pts.ptr + 16 * (m - 1)), "counts over hits": call(cn=hits.ptr + 8 * (m * k - 1)),
            "points over counts": call(p=counts.ptr + 4 * (m - 1)), "hits over counts": call(h=counts.ptr + 4 * (m - 1)),
            "n_points * k = 2^32": call(m_=1 << 27, k_=32), "n_points * k above 2^32": call(m_=0xFFFFFFFF, k_=2),
            "above capacity": call(res=variant(n_leaves=n + 1_000_000, root=0)),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {key: v for key, v in cases.items() if v != E_INVALID}
        c.synchronize()
        assert hits.download(pkg.KNN_HIT, m * k).tobytes() == s_hits.tobytes() and counts.download(np.uint32, m).tobytes() == s_cnt.tobytes()
        # adjacent ranges are no overlap
        both = c.alloc(m * k * 8 + m * 4)
        try:
            assert L.bvh_knn(c.handle, C.byref(b.result), None, d_pts.ptr, m, k, both.ptr, both.ptr + m * k * 8) == 0
        finally:
            c.synchronize(); both.free()
        # on a fresh ctx (capacity 0) a caller tree is refused until bvh_ctx_reserve
        c2 = pkg.Context(0)
        try:
            assert L.bvh_knn(c2.handle, C.byref(b.result), None, d_pts.ptr, m, k, hits.ptr, counts.ptr) == E_INVALID
        finally:
            c2.close()
        assert hits.download(pkg.KNN_HIT, m * k).tobytes() == s_hits.tobytes() and counts.download(np.uint32, m).tobytes() == s_cnt.tobytes()
        d_pts.free(); hits.free(); counts.free()
    finally:
        c.close()
