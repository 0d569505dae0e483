"""bvh_radius_search on the GPU: every triangle within the radius of every query, from every builder, both node layouts and all three triangle formats, against
the numpy brute force (tests/test_radius.py): count-only calls, sorted and unsorted fills, consistency with bvh_knn and bvh_closest_point, the stackless pass
on trees deeper than the short stack, the count / scan / fill passes and the capacity decision, answers after a refit / optimise / rebuild, errors, one larger
size."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_knn import knn
from test_gpu_multihit import chain_left
from test_gpu_point_query import make_points
from test_gpu_point_query import query as closest_query
from test_gpu_query import caterpillar, lbvh_result, mesh
from test_gpu_refit import jitter
from test_point_query import E_INVALID, F32
from test_radius import RADIUS_MESHES, RADIUS_SORTED, check_radius, radius_brute_force, radius_reference, slice_queries

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


def call(pkg, ctx, result, d_pts, m, flags, d_offsets, d_hits, capacity, total=True, inp=None):
    t = C.c_uint64(0xDEAD)
    rc = pkg.lib().bvh_radius_search(ctx.handle, C.byref(result), C.byref(inp) if inp is not None else None, d_pts, m, flags, d_offsets, d_hits, capacity,
                                     C.byref(t) if total else None)
    return rc, t.value


def search(pkg, ctx, result, pts, flags, inp=None):
    """a count-only call, then a fill with the exact capacity; returns (offsets, hits).  The count-only offsets must equal the fill's."""
    m = len(pts)
    d_pts, d_off = ctx.upload(pts), ctx.alloc((m + 1) * 4)
    hits = None
    try:
        rc, total = call(pkg, ctx, result, d_pts.ptr, m, flags, d_off.ptr, None, 0, inp=inp)
        assert rc == 0, rc
        counted = d_off.download(np.uint32, m + 1)
        assert counted[0] == 0 and counted[-1] == total
        hits = ctx.alloc(max(total, 1) * 8)
        rc, total2 = call(pkg, ctx, result, d_pts.ptr, m, flags, d_off.ptr, hits.ptr, total, inp=inp)
        assert rc == 0 and total2 == total
        off = d_off.download(np.uint32, m + 1)
        assert off.tobytes() == counted.tobytes(), "count-only and fill calls disagree on the offsets"
        return off, hits.download(pkg.KNN_HIT, total)
    finally:
        d_pts.free(); d_off.free()
        if hits is not None:
            hits.free()


@pytest.mark.parametrize("name", RADIUS_MESHES)
def test_exact_against_brute_force(pkg, ctx, name):
    tris = mesh(pkg, name)
    pts, ref = radius_reference(pkg, name)
    assert ref["well"].mean() >= 0.99, f"{name}: only {ref['well'].mean():.4f} of the queries are well-conditioned"
    every = []
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        keep = []
        results = [("as built", b.result)]
        if b.result.layout == 1:
            results.append(("lbvh layout", lbvh_result(pkg, ctx, b, keep)))
        for label, res in results:
            what = f"{name} algo {algo} {label}"
            off, hits = search(pkg, ctx, res, pts, RADIUS_SORTED)          # (asserts that the count-only offsets equal the fill call's)
            check_radius(pts, tris, ref, off, hits, True, what + " sorted")
            uoff, uhits = search(pkg, ctx, res, pts, 0)
            assert uoff.tobytes() == off.tobytes(), f"{what}: sorted and unsorted calls count differently"
            check_radius(pts, tris, ref, uoff, uhits, False, what + " unsorted")
            every.append((what, off, hits))
        poff, phits = b.radius_search(pts, sorted=True)                    # the Python binding, host records
        assert poff.tobytes() == every[-1][1].tobytes() and phits.tobytes() == every[-1][2].tobytes() and phits.dtype == pkg.KNN_HIT
        assert b.radius_search(pts, count_only=True).tobytes() == poff.tobytes()
        for k in keep:
            k.free()
    for what, off, hits in every:                                          # every query is well-conditioned: one answer, whatever the builder and the layout
        assert off.tobytes() == ref["offsets"].tobytes() and hits.tobytes() == ref["hits"].tobytes(), what


@pytest.mark.parametrize("name", ["uniform_1000", "sponza_1000", "cornell382"])
def test_consistent_with_knn_and_closest_point(pkg, ctx, name):
    tris = mesh(pkg, name)
    pts, ref = radius_reference(pkg, name)
    assert ref["well"].all()
    m = len(pts)
    for algo in (0, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        off, hits = search(pkg, ctx, b.result, pts, RADIUS_SORTED)
        counts = np.diff(off.astype(np.int64))
        lists, lens = knn(pkg, ctx, b.result, pts, 32)
        assert (np.minimum(counts, 32) == lens).all(), f"{name} algo {algo}: min(count, 32) != bvh_knn's d_counts"
        take = np.minimum(counts, 32)
        head = np.arange(32)[None] < take[:, None]
        idx = (off[:-1].astype(np.int64)[:, None] + np.arange(32)[None])[head]
        assert hits[idx].tobytes() == lists[head].tobytes(), f"{name} algo {algo}: the first min(32, count) records differ from bvh_knn(k = 32)'s list"
        assert (take < 32).any() and (counts > 32).any()
        closest = closest_query(pkg, ctx, b.result, pts, pkg.QUERY_CLOSEST)
        some = closest_query(pkg, ctx, b.result, pts, pkg.QUERY_ANY)
        has = counts > 0
        assert (has == (some["prim"] != pkg.INVALID)).all(), f"{name} algo {algo}: count > 0 and BVH_QUERY_ANY differ"
        assert (has == (closest["prim"] != pkg.INVALID)).all()
        first = hits[off[:-1][has]]
        assert first["dist2"].tobytes() == closest["dist2"][has].tobytes() and first["prim"].tobytes() == closest["prim"][has].tobytes()
        assert m == len(counts)


@pytest.mark.parametrize("name", ["uniform_1000", "cornell382"])
def test_formats_give_identical_bytes(pkg, ctx, name):
    tris = mesh(pkg, name); n = len(tris)
    pts, ref = radius_reference(pkg, name)
    b = pkg.HPLOC().build(ctx, tris)
    packed = np.ascontiguousarray(np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1).astype(np.float32).reshape(n, 9))
    uniq, inv = np.unique(packed.reshape(-1, 3), axis=0, return_inverse=True)
    idx = inv.reshape(-1).astype(np.uint32)
    d_p, d_v, d_i = ctx.upload(packed), ctx.upload(np.ascontiguousarray(uniq.astype(np.float32))), ctx.upload(idx)
    try:
        base = search(pkg, ctx, b.result, pts, RADIUS_SORTED)
        check_radius(pts, tris, ref, base[0], base[1], True, name)
        p = search(pkg, ctx, b.result, pts, RADIUS_SORTED, pkg.BuildInput(pkg.TRI_PACKED36, 30, d_p.ptr, None, None, 0, 0))
        i = search(pkg, ctx, b.result, pts, RADIUS_SORTED, pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, len(uniq), 0))
        for other in (p, i):
            assert other[0].tobytes() == base[0].tobytes() and other[1].tobytes() == base[1].tobytes()
        py = b.radius_search(pts, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED)
        assert py[0].tobytes() == base[0].tobytes() and py[1].tobytes() == base[1].tobytes()
        up = search(pkg, ctx, b.result, pts, 0, pkg.BuildInput(pkg.TRI_PACKED36, 30, d_p.ptr, None, None, 0, 0))
        check_radius(pts, tris, ref, up[0], up[1], False, name + " packed unsorted")
        # a tree built FROM indexed input answers the same
        bi = pkg.PLOCNew().build_ex(ctx, n, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED)
        got = bi.radius_search(pts, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
    finally:
        for x in (d_p, d_v, d_i):
            x.free()


def test_binding_fills_radius_for_plain_points(pkg, ctx):
    tris = mesh(pkg, "sponza_1000")
    pts, _ = radius_reference(pkg, "sponza_1000")
    xyz = np.ascontiguousarray(pts["point"])
    b = pkg.SinglePassLbvh().build(ctx, tris)
    per_query = np.linspace(0.0, 0.5, len(xyz)).astype(np.float32)
    for radius in (None, 0.5, per_query):
        rec = np.zeros(len(xyz), dtype=pkg.POINT_QUERY); rec["point"] = xyz; rec["radius"] = np.inf if radius is None else radius
        (o0, h0), (o1, h1) = b.radius_search(xyz, radius=radius), b.radius_search(rec)
        assert o0.tobytes() == o1.tobytes() and h0.tobytes() == h1.tobytes() and o0[-1] == len(h0)
    with pytest.raises(pkg.BvhError):
        b.radius_search(pts, radius=1.0)                          # POINT_QUERY records carry their own radius
    off, hits = b.radius_search(np.zeros((0, 3), dtype=np.float32))
    assert off.tolist() == [0] and len(hits) == 0
    # point clouds as degenerate packed triangles: the neighbours of a cloud point within r, itself first
    rng = np.random.default_rng(3)
    cloud = rng.random((1500, 3)).astype(np.float32)
    d_p = ctx.upload(np.ascontiguousarray(np.repeat(cloud, 3, axis=0).reshape(len(cloud), 9)))
    try:
        bc = pkg.HPLOC().build_ex(ctx, len(cloud), tris=d_p, tri_format=pkg.TRI_PACKED36)
        off, hits = bc.radius_search(cloud[:256], radius=0.1, tris=d_p, tri_format=pkg.TRI_PACKED36)
        d = cloud[None] - cloud[:256, None]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        inside = d2 <= np.float32(0.1) * np.float32(0.1)
        assert (np.diff(off.astype(np.int64)) == inside.sum(axis=1)).all() and (hits["prim"][off[:-1]] == np.arange(256)).all()
        qi = slice_queries(off)
        assert inside[qi, hits["prim"]].all() and hits["dist2"].tobytes() == d2[qi, hits["prim"]].tobytes()
    finally:
        d_p.free()


# ---- the stackless pass -----------------------------------------------------------------------------------------------------------------------------------

def box_dist_pass(lo, hi, p, r2):
    """query.hpp's box_dist_pass in f32, operation for operation"""
    with np.errstate(all="ignore"):
        g = F32(2.0 ** -16) * max(np.abs(lo).max(), np.abs(hi).max())
        d = np.maximum(np.maximum((lo - g) - p, p - (hi + g)), F32(0.0))
        lb = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        return bool(lb * (F32(1.0) - F32(2.0 ** -20)) <= r2)


def walk_stack(nodes, root, ni, p, r2):
    """k_radius_walk restated on the host for one query: both children box-tested against r2, passing leaves taken at once, of two passing internal
    children the left entered and the right pushed.  Returns the largest number of entries the short stack holds."""
    p = np.asarray(p, dtype=F32); r2 = F32(r2)
    left, right, lo, hi = nodes["left"], nodes["right"], nodes["min"].astype(F32), nodes["max"].astype(F32)
    stack, deepest = [], 0
    nl, nr = int(left[root]), int(right[root])
    while True:
        ha = nl < ni and box_dist_pass(lo[nl], hi[nl], p, r2)            # (a passing leaf is tested at once and never entered)
        hb = nr < ni and box_dist_pass(lo[nr], hi[nr], p, r2)
        if ha or hb:
            if ha and hb:
                stack.append(nr); deepest = max(deepest, len(stack))
            node = nl if ha else nr
        else:
            if not stack:
                return deepest
            node = stack.pop()
        nl, nr = int(left[node]), int(right[node])


@pytest.mark.parametrize("H", [40, 80])
def test_deep_tree_takes_the_stackless_pass(pkg, H):
    tris, made, root, n = caterpillar(pkg, H, 7 + H)
    nodes = chain_left(made, n - 1)                           # the chain below every left link: the left-first walk holds one pushed side node per level
    rng = np.random.default_rng(H)
    m = 240
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    pts["point"] = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-3, -0.5, m)], axis=1)
    g = m // 6
    pts["radius"] = np.inf                                    # [0, g): every box passes, every triangle is accepted
    pts["radius"][g:2 * g] = 5000.0                           # the same with a finite radius
    pts["radius"][2 * g:3 * g] = 5.0                          # the two near triangles; every side node is culled
    pts["point"][3 * g:4 * g, 2] = -500.0; pts["radius"][3 * g:4 * g] = 1.0      # no box passes
    pts["point"][4 * g:, 2] = rng.uniform(1000, 1000 + 2 * H, m - 4 * g)          # among the far triangles: a few side nodes pass
    pts["radius"][4 * g:] = rng.uniform(0.1, 6.5, m - 4 * g)
    r2 = pts["radius"].astype(F32) * pts["radius"].astype(F32)
    need = np.array([walk_stack(nodes, root, n - 1, pts["point"][j], r2[j]) for j in range(m)])
    if H > 64:
        assert need[:2 * g].min() > 64 and need[2 * g:4 * g].max() == 0, (need.min(), need.max())       # some queries overflow the short stack, others fit
    else:
        assert need.max() <= 64 and need.max() >= H - 1, need.max()                                    # none does
    ref = radius_brute_force(pkg, pts, tris)
    c = ref["counts"]
    assert ref["well"].all() and (c[:2 * g] == n).all() and (c[2 * g:3 * g] == 2).all() and (c[3 * g:4 * g] == 0).all() and c[4 * g:].max() > 4
    ctx = pkg.Context(0)
    try:
        ctx.reserve(n)
        d_nodes, d_tris = ctx.upload(nodes), ctx.upload(tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        ctx.set_profiling(2)
        off, hits = search(pkg, ctx, r, pts, RADIUS_SORTED)       # (asserts that the count-only and the fill call agree)
        kt = ctx.kernel_times()
        ctx.set_profiling(0)
        assert {"k_radius_count", "k_radius_fill", "k_radius_deep", "k_overlap_scan", "k_refit_plan"} <= set(kt), sorted(kt)
        assert off.tobytes() == ref["offsets"].tobytes() and hits.tobytes() == ref["hits"].tobytes(), f"H {H}"
        uoff, uhits = search(pkg, ctx, r, pts, 0)
        check_radius(pts, tris, ref, uoff, uhits, False, f"H {H} unsorted")
        assert uoff.tobytes() == ref["offsets"].tobytes()
        d_nodes.free(); d_tris.free()
    finally:
        ctx.close()


# ---- passes, capacity, buffers ------------------------------------------------------------------------------------------------------------------------------

def test_passes_and_capacity(pkg, ctx):
    name = "cornell382"
    tris = mesh(pkg, name)
    pts, ref = radius_reference(pkg, name)
    m = len(pts)
    b = pkg.HPLOC().build(ctx, tris)
    want = {}
    for flags in (RADIUS_SORTED, 0):                                     # the answers the passes below must reproduce, checked against the brute force
        want[flags] = search(pkg, ctx, b.result, pts, flags)
        check_radius(pts, tris, ref, want[flags][0], want[flags][1], flags == RADIUS_SORTED, f"{name} flags {flags}")
    exp_off = ref["offsets"]
    total = int(exp_off[-1])
    assert total > 1000 and want[RADIUS_SORTED][0].tobytes() == exp_off.tobytes() == want[0][0].tobytes()
    extra = 29
    guard_h = np.frombuffer(np.full((total + extra) * 8, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.KNN_HIT)
    guard_o = np.full(m + 1 + extra, 0xA5A5A5A5, dtype=np.uint32)
    d_pts, d_off, d_hits = ctx.upload(pts), ctx.upload(guard_o), ctx.upload(guard_h)
    try:
        for flags in (RADIUS_SORTED, 0):
            out = {}
            # d_hits == NULL counts only: offsets complete, guard words past the n_points + 1 offsets intact
            d_off.upload(guard_o); d_hits.upload(guard_h)
            assert call(pkg, ctx, b.result, d_pts.ptr, m, flags, d_off.ptr, None, 0) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_hits.download(pkg.KNN_HIT, total + extra).tobytes() == guard_h.tobytes()
            # capacity total - 1: the fill is skipped, d_hits untouched byte for byte, d_offsets still complete, *total_out set
            d_off.upload(guard_o)
            assert call(pkg, ctx, b.result, d_pts.ptr, m, flags, d_off.ptr, d_hits.ptr, total - 1) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_hits.download(pkg.KNN_HIT, total + extra).tobytes() == guard_h.tobytes()
            # the exact capacity is filled; guard records past the total intact; twice the same bytes
            for rnd in range(2):
                d_off.upload(guard_o); d_hits.upload(guard_h)
                assert call(pkg, ctx, b.result, d_pts.ptr, m, flags, d_off.ptr, d_hits.ptr, total) == (0, total)
                o, h = d_off.download(np.uint32, m + 1 + extra), d_hits.download(pkg.KNN_HIT, total + extra)
                assert o[m + 1:].tobytes() == guard_o[m + 1:].tobytes() and h[total:].tobytes() == guard_h[total:].tobytes()
                assert o[: m + 1].tobytes() == exp_off.tobytes() and h[:total].tobytes() == want[flags][1].tobytes()
                out[rnd] = (o.tobytes(), h.tobytes())
            assert out[0] == out[1], "two identical calls give different bytes"
            # total_out == NULL: the same device bytes, nothing stored on the host
            d_off.upload(guard_o); d_hits.upload(guard_h)
            rc, t = call(pkg, ctx, b.result, d_pts.ptr, m, flags, d_off.ptr, d_hits.ptr, total + extra, total=False)
            assert rc == 0 and t == 0xDEAD
            ctx.synchronize()
            assert (d_off.download(np.uint32, m + 1 + extra).tobytes(), d_hits.download(pkg.KNN_HIT, total + extra).tobytes()) == out[0]
            assert d_pts.download(pkg.POINT_QUERY, m).tobytes() == pts.tobytes()
        # n_points == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        d_off.upload(guard_o); d_hits.upload(guard_h)
        assert call(pkg, ctx, b.result, d_pts.ptr, 0, RADIUS_SORTED, d_off.ptr, d_hits.ptr, total) == (0, 0)
        o = d_off.download(np.uint32, m + 1 + extra)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes() and d_hits.download(pkg.KNN_HIT, total + extra).tobytes() == guard_h.tobytes()
        # the Python binding: a capacity that is too small is re-allocated
        poff, phits = b.radius_search(pts, sorted=True, capacity=3)
        assert poff.tobytes() == exp_off.tobytes() and phits.tobytes() == ref["hits"].tobytes()
    finally:
        d_pts.free(); d_off.free(); d_hits.free()


_MOVED = {}


def moved_reference(pkg):
    if not _MOVED:
        a = mesh(pkg, "sponza_1000"); moved = jitter(a, 23, 2e-3)
        pts = make_points(pkg, moved, 512, 29)
        _MOVED["v"] = (a, moved, pts, radius_brute_force(pkg, pts, moved))
    return _MOVED["v"]


@pytest.mark.parametrize("algo", [1, 3])
def test_after_refit_optimize_and_rebuild(pkg, algo):
    a, moved, pts, ref = moved_reference(pkg)
    assert ref["well"].mean() >= 0.99
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        b.radius_search(pts, count_only=True)                 # (the plan of the ctx's own tree is made here and kept)
        b.refit(moved)
        off, hits = b.radius_search(pts)
        check_radius(pts, moved, ref, off, hits, True, f"refit algo {algo}")
        uoff, uhits = b.radius_search(pts, sorted=False)
        check_radius(pts, moved, ref, uoff, uhits, False, f"refit algo {algo} unsorted")
        assert b.radius_search(pts, count_only=True).tobytes() == off.tobytes()
        b.optimize(3)
        ooff, ohits = b.radius_search(pts)
        check_radius(pts, moved, ref, ooff, ohits, True, f"optimised algo {algo}")
        b2 = pkg.BUILDERS[algo]().build(c, moved)
        off2, hits2 = b2.radius_search(pts)
        check_radius(pts, moved, ref, off2, hits2, True, f"rebuild algo {algo}")
    finally:
        c.close()


def test_errors_write_nothing(pkg):
    tris = mesh(pkg, "uniform_1000"); n = len(tris)
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        m = 256
        pts = make_points(pkg, tris, m, 4)
        d_pts = c.upload(pts)
        cap = 4096
        guard_h = np.frombuffer(np.full(cap * 8, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.KNN_HIT)
        guard_o = np.full(m + 1, 0x5A5A5A5A, dtype=np.uint32)
        hits, offs = c.upload(guard_h), c.upload(guard_o)
        L = pkg.lib()
        tot = C.c_uint64(0x77)

        def go(res=b.result, inp=None, p=d_pts.ptr, m_=m, flags=RADIUS_SORTED, o=offs.ptr, h=hits.ptr, k=cap, ctx=c.handle):
            return L.bvh_radius_search(ctx, C.byref(res) if res is not None else None, C.byref(inp) if inp is not None else None, p, m_, flags, o, h, k, C.byref(tot))

        def variant(**kw):
            r = pkg.Result.from_buffer_copy(b.result)
            for k, v in kw.items():
                setattr(r, k, v)
            return r
        cases = {
            "null ctx": go(ctx=None), "null tree": go(res=None), "null points": go(p=None), "null offsets": go(o=None),
            "n_leaves 1": go(res=variant(n_leaves=1)), "layout 2": go(res=variant(layout=2)), "null nodes": go(res=variant(d_nodes=None)),
            "layout 1 without leaves": go(res=variant(d_leaves=None)), "root not internal": go(res=variant(root=n - 1)),
            "no triangles": go(res=variant(d_tris=None)), "bad format": go(inp=pkg.BuildInput(7, 30, b.result.d_tris, None, None, 0, 0)),
            "packed unaligned": go(inp=pkg.BuildInput(pkg.TRI_PACKED36, 30, b.result.d_tris + 4, None, None, 0, 0)),
            "indexed without vertices": go(inp=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, None, b.result.d_tris, 3, 0)),
            "flag 2": go(flags=2), "flag 3": go(flags=3), "flag high": go(flags=0x80000000),
            "n_points 2^30": go(m_=1 << 30),
            "offsets in points": go(o=d_pts.ptr + 64), "hits in points": go(h=d_pts.ptr + 32), "hits in offsets": go(h=offs.ptr + 16),
            "offsets in hits": go(o=hits.ptr + 8 * (cap - 1)), "points in hits": go(p=hits.ptr, h=hits.ptr + 16 * 8),
            "above capacity": go(res=variant(n_leaves=n + 1_000_000, root=0)),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        assert tot.value == 0x77
        c.synchronize()
        assert hits.download(pkg.KNN_HIT, cap).tobytes() == guard_h.tobytes() and offs.download(np.uint32, m + 1).tobytes() == guard_o.tobytes()
        # a count-only call ignores the capacity's range
        assert go(h=None, k=1 << 40) == 0 and tot.value != 0x77
        # on a fresh ctx (capacity 0) a caller tree is refused until bvh_ctx_reserve
        offs.upload(guard_o)
        c2 = pkg.Context(0)
        try:
            assert go(ctx=c2.handle) == E_INVALID
        finally:
            c2.close()
        assert hits.download(pkg.KNN_HIT, cap).tobytes() == guard_h.tobytes() and offs.download(np.uint32, m + 1).tobytes() == guard_o.tobytes()
        d_pts.free(); hits.free(); offs.free()
    finally:
        c.close()


def test_one_larger_size(pkg, ctx):
    """sponza_20000 with 4096 near-surface points and finite narrow-band radii only: more workgroups than one wave's worth in the count grid, more than one
    tile in the scan, short slices"""
    tris = mesh(pkg, "sponza_20000")
    rng = np.random.default_rng(41)
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    ext = v.max(axis=0) - v.min(axis=0); diag = float(np.linalg.norm(ext))
    m = 4096
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    pts["point"] = (v[rng.integers(0, len(v), size=m)] + rng.normal(0, 1e-3, (m, 3)) * ext).astype(np.float32)
    pts["radius"] = np.where(rng.integers(0, 2, size=m) == 0, 2e-3 * diag, rng.random(m) * 0.05 * diag)
    ref = radius_brute_force(pkg, pts, tris, chunk_elems=1 << 20, workers=8)
    assert ref["well"].mean() >= 0.99 and (ref["counts"] == 0).any() and ref["counts"].max() > 32 and ref["counts"].max() < 1000
    for algo in (3, 1):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        off, hits = b.radius_search(pts, sorted=True)
        check_radius(pts, tris, ref, off, hits, True, f"sponza_20000 algo {algo}")
        assert b.radius_search(pts, count_only=True).tobytes() == off.tobytes()
