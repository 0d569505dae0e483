"""bvh_closest_point on the GPU: closest-point and any-within-radius answers of every builder, both node layouts and all three triangle formats against the
numpy brute force (tests/test_point_query.py), the stackless pass on trees deeper than the short stack, queries after a refit, an optimise and a rebuild,
large sizes, buffer hygiene and errors."""
import ctypes as C

import numpy as np
import pytest

from test_point_query import E_INVALID, below, point_brute_force, recompute_points
from test_gpu_query import caterpillar, lbvh_result, mesh
from test_gpu_refit import jitter, no_negzero

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

SIZES = [2, 3, 63, 64, 65, 1000, 20_000]
MESHES = [f"uniform_{n}" for n in SIZES] + ["sponza_1000", "sponza_20000", "cornell32", "cornell82", "cornell382"]


def make_points(pkg, tris, m, seed):
    """a mix: uniform points inside and outside the scene box, points exactly on vertices, on edges and on faces, near-surface points (vertices jittered by
    1e-3 of the extent), points on triangles' box planes; radii infinite, finite (wide and narrow-band), zero, negative and NaN; NaN coordinates"""
    rng = np.random.default_rng(seed)
    v1, v2, v3 = (tris[f].astype(np.float32) for f in ("v1", "v2", "v3"))
    v = np.concatenate([v1, v2, v3]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3); diag = float(np.linalg.norm(ext))
    n = len(tris)
    p = (lo - 0.5 * ext + rng.random((m, 3)) * 2.0 * ext).astype(np.float32)      # inside and outside the box
    k = m // 8
    t = rng.integers(0, n, size=6 * k)
    p[0:k] = v[rng.integers(0, len(v), size=k)]                                           # on vertices
    a, b = v1[t[k:2 * k]], v2[t[k:2 * k]]
    p[k:2 * k] = (a + b) * np.float32(0.5)                                                # on edges (dist2 0 or tiny)
    w = rng.dirichlet((1.0, 1.0, 1.0), size=k).astype(np.float32)
    i = t[2 * k:3 * k]
    p[2 * k:3 * k] = (v1[i] * w[:, :1] + v2[i] * w[:, 1:2]) + v3[i] * w[:, 2:]         # on faces
    p[3 * k:4 * k] = (v[rng.integers(0, len(v), size=k)] + rng.normal(0, 1e-3, (k, 3)) * ext).astype(np.float32)   # near-surface
    ax = rng.integers(0, 3, size=k)
    p[4 * k + np.arange(k), ax] = v[rng.integers(0, len(v), size=k), ax]                 # on box planes
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    pts["point"] = p
    choice = rng.integers(0, 4, size=m)
    pts["radius"] = np.where(choice == 0, np.inf, np.where(choice == 1, rng.random(m) * 0.3 * diag, np.where(choice == 2, 2e-3 * diag, rng.random(m) * 0.05 * diag)))
    s = rng.choice(m - 8, size=40, replace=False)
    pts["radius"][s[:10]] = 0.0
    pts["radius"][s[10:20]] = -rng.random(10)
    pts["radius"][s[20:25]] = -np.inf
    pts["radius"][s[25:35]] = np.nan
    pts["radius"][s[35:]] = -0.0
    for j, c in enumerate(range(m - 8, m)):                                               # NaN coordinates
        pts["point"][c, j % 3] = np.nan
    return pts


_REF = {}


def reference(pkg, name):
    if name not in _REF:
        tris = mesh(pkg, name)
        pts = make_points(pkg, tris, 1536, 11 + len(tris))
        _REF[name] = (pts, point_brute_force(pkg, pts, tris))
    return _REF[name]


def query(pkg, ctx, result, pts, kind, inp=None):
    d_pts = ctx.upload(pts)
    hits = ctx.alloc(len(pts) * 32)
    try:
        rc = pkg.lib().bvh_closest_point(ctx.handle, C.byref(result), C.byref(inp) if inp is not None else None, d_pts.ptr, len(pts), hits.ptr, kind)
        assert rc == 0, rc
        return hits.download(pkg.POINT_HIT, len(pts))
    finally:
        d_pts.free(); hits.free()


def check_exact(pkg, pts, tris, bf, closest, anyhit, what):
    well = bf["well"]
    assert well.mean() >= 0.99, f"{what}: only {well.mean():.4f} of the queries are well-conditioned"
    ref = bf["closest"]
    diff = (closest.view(np.uint8).reshape(-1, 32) != ref.view(np.uint8).reshape(-1, 32)).any(axis=1)
    assert not (diff & well).any(), f"{what}: closest differs on {np.count_nonzero(diff & well)} well-conditioned queries (first {np.nonzero(diff & well)[0][:6]})"
    hit_any = anyhit["prim"] != pkg.INVALID
    assert (hit_any == bf["hit"])[well].all(), f"{what}: any-hit hit/miss differs"
    # every query: reported hits are accepted candidates with bit-equal records, misses the exact miss record; no closest answer below the brute force
    assert recompute_points(pkg, pts, tris, closest).all(), f"{what}: a closest record is not an accepted candidate of its prim (or not the miss record)"
    assert recompute_points(pkg, pts, tris, anyhit).all(), f"{what}: an any record is not an accepted candidate of its prim (or not the miss record)"
    assert not below(pkg, closest, ref).any(), f"{what}: closest below the brute force"


@pytest.mark.parametrize("name", MESHES)
def test_exact_against_brute_force(pkg, ctx, name):
    tris = mesh(pkg, name)
    pts, bf = reference(pkg, name)
    assert bf["hit"].any() and not bf["hit"].all()
    per_algo = {}
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        keep = []
        results = [("as built", b.result)]
        if b.result.layout == 1:
            results.append(("lbvh layout", lbvh_result(pkg, ctx, b, keep)))
        for label, res in results:
            c = query(pkg, ctx, res, pts, pkg.QUERY_CLOSEST)
            a = query(pkg, ctx, res, pts, pkg.QUERY_ANY)
            check_exact(pkg, pts, tris, bf, c, a, f"{name} algo {algo} {label}")
            per_algo.setdefault(algo, c)
        assert b.closest_point(pts, query="closest").tobytes() == per_algo[algo].tobytes()      # the Python binding, host records
        for k in keep:
            k.free()
    well = bf["well"]
    for algo in (1, 2, 3):
        assert per_algo[algo][well].tobytes() == per_algo[0][well].tobytes(), f"{name}: builders {algo} and 0 differ"


def test_binding_fills_radius_for_plain_points(pkg, ctx):
    tris = mesh(pkg, "sponza_1000")
    pts, _ = reference(pkg, "sponza_1000")
    xyz = np.ascontiguousarray(pts["point"])
    b = pkg.SinglePassLbvh().build(ctx, tris)
    for radius in (None, 0.5):
        rec = np.zeros(len(xyz), dtype=pkg.POINT_QUERY); rec["point"] = xyz; rec["radius"] = np.inf if radius is None else radius
        assert b.closest_point(xyz, radius=radius).tobytes() == b.closest_point(rec).tobytes()
        d = ctx.upload(rec)
        try:
            assert b.closest_point(d, query="any").tobytes() == b.closest_point(rec, query="any").tobytes()
        finally:
            d.free()
    with pytest.raises(pkg.BvhError):
        b.closest_point(pts, radius=1.0)                          # POINT_QUERY records carry their own radius


@pytest.mark.parametrize("name", ["uniform_1000", "sponza_20000", "cornell382"])
def test_formats_give_identical_answers(pkg, ctx, name):
    tris = mesh(pkg, name); n = len(tris)
    pts, bf = reference(pkg, name)
    b = pkg.HPLOC().build(ctx, tris)
    packed = np.ascontiguousarray(np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1).astype(np.float32).reshape(n, 9))
    verts = packed.reshape(-1, 3)
    uniq, inv = np.unique(verts, axis=0, return_inverse=True)
    idx = inv.reshape(-1).astype(np.uint32)
    d_p, d_v, d_i = ctx.upload(packed), ctx.upload(np.ascontiguousarray(uniq.astype(np.float32))), ctx.upload(idx)
    try:
        for kind in (pkg.QUERY_CLOSEST, pkg.QUERY_ANY):
            base = query(pkg, ctx, b.result, pts, kind)
            p = query(pkg, ctx, b.result, pts, kind, pkg.BuildInput(pkg.TRI_PACKED36, 30, d_p.ptr, None, None, 0, 0))
            i = query(pkg, ctx, b.result, pts, kind, pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, len(uniq), 0))
            assert base.tobytes() == p.tobytes() == i.tobytes()
            assert b.closest_point(pts, query=kind, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED).tobytes() == base.tobytes()
        # a tree built FROM indexed input answers the same
        bi = pkg.PLOCNew().build_ex(ctx, n, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED)
        got = bi.closest_point(pts, query="closest", vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED)
        assert got[bf["well"]].tobytes() == bf["closest"][bf["well"]].tobytes()
    finally:
        for x in (d_p, d_v, d_i):
            x.free()


def first_descent_pushes(nodes, root, ni, p):
    """stack entries the short-stack kernel holds when its first descent reaches a node with a leaf child, for a query whose radius passes every box (no
    candidate is tested before that: every box passes): at each node with two internal children the one with the smaller f64 box distance is entered and the
    other pushed"""
    def lb(c):
        d = np.maximum(np.maximum(nodes["min"][c].astype(np.float64) - p, p - nodes["max"][c].astype(np.float64)), 0.0)
        return d @ d
    v, pushes = root, 0
    while True:
        l, r = int(nodes["left"][v]), int(nodes["right"][v])
        if l >= ni or r >= ni:
            return pushes
        pushes += 1
        v = l if lb(l) <= lb(r) else r


@pytest.mark.parametrize("H", [70, 250])
def test_deep_tree_takes_the_stackless_pass(pkg, H):
    tris, nodes, root, n = caterpillar(pkg, H, 5 + H)
    rng = np.random.default_rng(H)
    m = 300
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    pts["point"] = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-3, -0.5, m)], axis=1)
    pts["point"][: m // 6, 2] = 0.0                             # on the face at z = 0
    pts["radius"] = np.inf
    pts["radius"][m // 2: 3 * m // 4] = 5.0                     # the far side nodes are culled: no push, the short stack suffices
    pts["point"][3 * m // 4:, 2] = rng.uniform(1000, 1000 + 2 * H, m - 3 * m // 4)     # among the far triangles
    assert max(first_descent_pushes(nodes, root, n - 1, pts["point"][j].astype(np.float64)) for j in range(m // 2)) > 64
    bf = point_brute_force(pkg, pts, tris)
    assert bf["well"].all() and bf["hit"].all()
    c = pkg.Context(0)
    try:
        c.reserve(n)
        d_nodes, d_tris = c.upload(nodes), c.upload(tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        c.set_profiling(2)
        closest = query(pkg, c, r, pts, pkg.QUERY_CLOSEST)
        anyhit = query(pkg, c, r, pts, pkg.QUERY_ANY)
        kt = c.kernel_times()
        c.set_profiling(0)
        assert {"k_closest_point", "k_closest_point_deep", "k_refit_plan"} <= set(kt)
        assert closest.tobytes() == bf["closest"].tobytes()
        assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"]).all() and recompute_points(pkg, pts, tris, anyhit).all()
        d_nodes.free(); d_tris.free()
    finally:
        c.close()


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_query_after_refit_optimize_and_rebuild(pkg, algo):
    a = mesh(pkg, "uniform_20000"); moved = jitter(a, 19, 2e-3)
    other = mesh(pkg, "sponza_20000")
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        pts = make_points(pkg, moved, 1024, 8)
        b.closest_point(pts)                                  # (the plan of the ctx's own tree is made here and kept)
        b.refit(moved)
        bf = point_brute_force(pkg, pts, moved)
        check_exact(pkg, pts, moved, bf, b.closest_point(pts), b.closest_point(pts, query="any"), f"refit algo {algo}")
        b.optimize(3)
        check_exact(pkg, pts, moved, bf, b.closest_point(pts), b.closest_point(pts, query="any"), f"optimize algo {algo}")
        b2 = pkg.BUILDERS[algo]().build(c, other)
        pts2 = make_points(pkg, other, 1024, 9)
        bf2 = point_brute_force(pkg, pts2, other)
        check_exact(pkg, pts2, other, bf2, b2.closest_point(pts2), b2.closest_point(pts2, query="any"), f"rebuild algo {algo}")
    finally:
        c.close()


@pytest.mark.parametrize("name,n", [("sponza", 262_144), ("uniform", 2_000_000)])
def test_large_trees(pkg, ctx, name, n):
    tris = no_negzero(pkg.meshgen.sponza_like(n, 3) if name == "sponza" else pkg.meshgen.uniform(n, 9))
    m = 1_000_003
    pts = make_points(pkg, tris, m, 23)
    res = {}
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        c, a = b.closest_point(pts), b.closest_point(pts, query="any")
        assert recompute_points(pkg, pts, tris, c).all() and recompute_points(pkg, pts, tris, a).all()
        agree = (c["prim"] != pkg.INVALID) == (a["prim"] != pkg.INVALID)
        assert agree.mean() >= 0.999, f"any / closest hit-miss agree on {agree.mean():.5f}"
        res[algo] = c
    for algo in (1, 2, 3):
        same = (res[algo].view(np.uint8).reshape(-1, 32) == res[0].view(np.uint8).reshape(-1, 32)).all(axis=1)
        assert same.mean() >= 0.999, f"builders {algo} / 0 agree on {same.mean():.5f}"
    sample = np.random.default_rng(1).choice(m, 64, replace=False)
    bf = point_brute_force(pkg, pts[sample], tris)
    well = bf["well"]
    assert well.mean() >= 0.95
    for algo in (0, 3):
        assert res[algo][sample][well].tobytes() == bf["closest"][well].tobytes()


def test_buffers_untouched_outside_the_hits(pkg, ctx):
    tris = mesh(pkg, "uniform_1000")
    b = pkg.HPLOC().build(ctx, tris)
    pts = make_points(pkg, tris, 1000, 3)
    d_pts = ctx.upload(pts)
    extra = 37
    sentinel = np.frombuffer(np.full((len(pts) + extra) * 32, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.POINT_HIT)
    hits = ctx.upload(sentinel)
    try:
        for kind in (0, 1):
            assert pkg.lib().bvh_closest_point(ctx.handle, C.byref(b.result), None, d_pts.ptr, len(pts), hits.ptr, kind) == 0
            out = hits.download(pkg.POINT_HIT, len(pts) + extra)
            assert out[len(pts):].tobytes() == sentinel[len(pts):].tobytes()
            assert recompute_points(pkg, pts, tris, out[: len(pts)]).all()
            assert d_pts.download(pkg.POINT_QUERY, len(pts)).tobytes() == pts.tobytes()
        hits.upload(sentinel)
        assert pkg.lib().bvh_closest_point(ctx.handle, C.byref(b.result), None, d_pts.ptr, 0, hits.ptr, 0) == 0      # n_points == 0: nothing touched
        assert hits.download(pkg.POINT_HIT, len(pts) + extra).tobytes() == sentinel.tobytes()
    finally:
        d_pts.free(); hits.free()


def test_errors_write_nothing(pkg):
    tris = mesh(pkg, "uniform_1000"); n = len(tris)
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        pts = make_points(pkg, tris, 256, 4)
        d_pts = c.upload(pts)
        sentinel = np.frombuffer(np.full(256 * 32, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.POINT_HIT)
        hits = c.upload(sentinel)
        L = pkg.lib()

        def call(res=b.result, inp=None, p=d_pts.ptr, m=256, h=hits.ptr, q=0, ctx=c.handle):
            return L.bvh_closest_point(ctx, C.byref(res) if res is not None else None, C.byref(inp) if inp is not None else None, p, m, h, q)

        def variant(**kw):
            r = pkg.Result.from_buffer_copy(b.result)
            for k, v in kw.items():
                setattr(r, k, v)
            return r
        cases = {
            "null ctx": call(ctx=None), "null tree": call(res=None), "null points": call(p=None), "null hits": call(h=None),
            "n_leaves 1": call(res=variant(n_leaves=1)), "layout 2": call(res=variant(layout=2)), "null nodes": call(res=variant(d_nodes=None)),
            "layout 1 without leaves": call(res=variant(d_leaves=None)), "root not internal": call(res=variant(root=n - 1)),
            "no triangles": call(res=variant(d_tris=None)), "bad format": call(inp=pkg.BuildInput(7, 30, b.result.d_tris, None, None, 0, 0)),
            "packed unaligned": call(inp=pkg.BuildInput(pkg.TRI_PACKED36, 30, b.result.d_tris + 4, None, None, 0, 0)),
            "indexed without vertices": call(inp=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, None, b.result.d_tris, 3, 0)),
            "query 2": call(q=2), "query -1": call(q=-1),
            "overlap": call(h=d_pts.ptr + 16), "overlap below": call(p=hits.ptr + 32 * 255),
            "above capacity": call(res=variant(n_leaves=n + 1_000_000, root=0)),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        c.synchronize()
        assert hits.download(pkg.POINT_HIT, 256).tobytes() == sentinel.tobytes()
        # on a fresh ctx (capacity 0) a caller tree is refused until bvh_ctx_reserve
        c2 = pkg.Context(0)
        try:
            assert L.bvh_closest_point(c2.handle, C.byref(b.result), None, d_pts.ptr, 256, hits.ptr, 0) == E_INVALID
        finally:
            c2.close()
        assert hits.download(pkg.POINT_HIT, 256).tobytes() == sentinel.tobytes()
        d_pts.free(); hits.free()
    finally:
        c.close()
