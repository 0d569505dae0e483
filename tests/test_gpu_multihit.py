"""bvh_intersect_all on the GPU: every accepted hit of every ray, from every builder, both node layouts and all three triangle formats, against the numpy brute
force (tests/test_multihit.py): sorted and unsorted fills, long slices with exact-t ties, the count / scan / fill passes and the capacity decision, the
stackless pass on trees deeper than the short stack, answers after a refit / optimise / rebuild, consistency with bvh_intersect, errors, one large size."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_query import MESHES, caterpillar, lbvh_result, make_rays, mesh, query, reference, tree_height_and_stack
from test_gpu_refit import jitter, no_negzero
from test_multihit import HITS_SORTED, all_hits_brute_force, check_all_hits, slab_rays, slab_stack, slice_rays
from test_query import E_INVALID

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

E_TOO_LARGE = -10002
_ALL = {}


def all_reference(pkg, ctx, name):
    """(rays, closest-hit brute force, all-hits brute force) per mesh, computed once; the rays are test_gpu_query.reference's"""
    if name not in _ALL:
        rays, bf = reference(pkg, ctx, name)
        ref = all_hits_brute_force(rays, mesh(pkg, name), workers=8)
        assert (ref["n_acc"] == bf["n_acc"]).all() and (ref["well"] == bf["well"]).all()
        _ALL[name] = (rays, bf, ref)
    return _ALL[name]


def call(pkg, ctx, result, d_rays, m, flags, d_offsets, d_hits, capacity, total=True, inp=None):
    t = C.c_uint64(0xDEAD)
    rc = pkg.lib().bvh_intersect_all(ctx.handle, C.byref(result), C.byref(inp) if inp is not None else None, d_rays, m, flags, d_offsets, d_hits, capacity,
                                     C.byref(t) if total else None)
    return rc, t.value


def all_hits(pkg, ctx, result, rays, flags, inp=None):
    """count-only call, then a fill with the exact capacity; returns (offsets, hits).  The count-only offsets must equal the fill's."""
    m = len(rays)
    d_rays, d_off = ctx.upload(rays), ctx.alloc((m + 1) * 4)
    hits = None
    try:
        rc, total = call(pkg, ctx, result, d_rays.ptr, m, flags, d_off.ptr, None, 0, inp=inp)
        assert rc == 0, rc
        counted = d_off.download(np.uint32, m + 1)
        assert counted[0] == 0 and counted[-1] == total
        hits = ctx.alloc(max(total, 1) * 16)
        rc, total2 = call(pkg, ctx, result, d_rays.ptr, m, flags, d_off.ptr, hits.ptr, total, inp=inp)
        assert rc == 0 and total2 == total
        off = d_off.download(np.uint32, m + 1)
        assert off.tobytes() == counted.tobytes(), "count-only and fill calls disagree on the offsets"
        return off, hits.download(pkg.HIT, total)
    finally:
        d_rays.free(); d_off.free()
        if hits is not None:
            hits.free()


@pytest.mark.parametrize("name", MESHES)
def test_exact_on_well_conditioned_rays(pkg, ctx, name):
    tris = mesh(pkg, name)
    rays, bf, ref = all_reference(pkg, ctx, name)
    well = ref["well"]
    assert well.mean() >= 0.99, f"{name}: only {well.mean():.4f} of the rays are well-conditioned"
    wrec = well[slice_rays(ref["offsets"])]
    per_algo = {}
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        keep = []
        results = [("as built", b.result)]
        if b.result.layout == 1:
            results.append(("lbvh layout", lbvh_result(pkg, ctx, b, keep)))
        for label, res in results:
            what = f"{name} algo {algo} {label}"
            off, hits = all_hits(pkg, ctx, res, rays, HITS_SORTED)
            check_all_hits(rays, tris, ref, off, hits, True, what + " sorted")
            uoff, uhits = all_hits(pkg, ctx, res, rays, 0)
            assert uoff.tobytes() == off.tobytes(), f"{what}: sorted and unsorted calls count differently"
            check_all_hits(rays, tris, ref, uoff, uhits, False, what + " unsorted")
            per_algo.setdefault(algo, (off, hits))
        poff, phits = b.intersect_all(rays, sorted=True)                  # the Python binding, host rays
        assert poff.tobytes() == per_algo[algo][0].tobytes() and phits.tobytes() == per_algo[algo][1].tobytes()
        assert b.intersect_all(rays, count_only=True).tobytes() == poff.tobytes()
        for k in keep:
            k.free()
    for algo in (1, 2, 3):                                                # identical across builders on the well-conditioned rays
        off, hits = per_algo[algo]
        assert (np.diff(off.astype(np.int64)) == np.diff(per_algo[0][0].astype(np.int64)))[well].all()
        assert hits[well[slice_rays(off)]].tobytes() == per_algo[0][1][well[slice_rays(per_algo[0][0])]].tobytes() == ref["hits"][wrec].tobytes()


def test_long_slices_and_ties(pkg, ctx):
    tris, rays = slab_stack(pkg), slab_rays(pkg)
    ref = all_hits_brute_force(rays, tris)
    assert ref["well"].all() and ref["n_acc"].min() >= 1 and ref["n_acc"].max() == 43
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        off, hits = all_hits(pkg, ctx, b.result, rays, HITS_SORTED)
        check_all_hits(rays, tris, ref, off, hits, True, f"slabs algo {algo}")
        assert off.tobytes() == ref["offsets"].tobytes() and hits.tobytes() == ref["hits"].tobytes()
        ray = slice_rays(off)
        tie = (ray[1:] == ray[:-1]) & (hits["t"][1:] == hits["t"][:-1])
        assert np.count_nonzero(tie) >= 3 * 128 and (hits["prim"][1:] > hits["prim"][:-1])[tie].all()      # equal-t records ordered by prim
        cut = np.nonzero(np.diff(off.astype(np.int64))[384:] < 43)[0] + 384                                  # tmax truncates slices exactly
        assert len(cut) and (hits["t"] < rays["tmax"][ray]).all()
        uoff, uhits = all_hits(pkg, ctx, b.result, rays, 0)
        check_all_hits(rays, tris, ref, uoff, uhits, False, f"slabs algo {algo} unsorted")


def test_passes_and_capacity(pkg, ctx):
    name = "sponza_1000"
    tris = mesh(pkg, name)
    rays, _, ref = all_reference(pkg, ctx, name)
    m = len(rays)
    b = pkg.HPLOC().build(ctx, tris)
    want = {}
    for flags in (HITS_SORTED, 0):                                       # the answers the passes below must reproduce, checked against the brute force
        want[flags] = all_hits(pkg, ctx, b.result, rays, flags)
        check_all_hits(rays, tris, ref, want[flags][0], want[flags][1], flags == HITS_SORTED, f"{name} flags {flags}")
    exp_off = want[0][0]
    total = int(exp_off[-1])
    assert total > 100 and want[HITS_SORTED][0].tobytes() == exp_off.tobytes()
    extra = 29
    guard_h = np.frombuffer(np.full((total + extra) * 16, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.HIT)
    guard_o = np.full(m + 1 + extra, 0xA5A5A5A5, dtype=np.uint32)
    d_rays, d_off, d_hits = ctx.upload(rays), ctx.upload(guard_o), ctx.upload(guard_h)
    try:
        for flags in (HITS_SORTED, 0):
            out = {}
            # count only: d_hits untouched, offsets complete, guard words past n_rays + 1 offsets intact
            d_off.upload(guard_o); d_hits.upload(guard_h)
            assert call(pkg, ctx, b.result, d_rays.ptr, m, flags, d_off.ptr, None, 0) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_hits.download(pkg.HIT, total + extra).tobytes() == guard_h.tobytes()
            # capacity total - 1: the fill is skipped, d_offsets still complete, *total_out set
            d_off.upload(guard_o)
            assert call(pkg, ctx, b.result, d_rays.ptr, m, flags, d_off.ptr, d_hits.ptr, total - 1) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_hits.download(pkg.HIT, total + extra).tobytes() == guard_h.tobytes()
            # the exact capacity is filled; guard records past the total intact; twice the same bytes
            for rnd in range(2):
                d_off.upload(guard_o); d_hits.upload(guard_h)
                assert call(pkg, ctx, b.result, d_rays.ptr, m, flags, d_off.ptr, d_hits.ptr, total) == (0, total)
                o, h = d_off.download(np.uint32, m + 1 + extra), d_hits.download(pkg.HIT, total + extra)
                assert o[m + 1:].tobytes() == guard_o[m + 1:].tobytes() and h[total:].tobytes() == guard_h[total:].tobytes()
                assert o[: m + 1].tobytes() == exp_off.tobytes() and h[:total].tobytes() == want[flags][1].tobytes()
                out[rnd] = (o.tobytes(), h.tobytes())
            assert out[0] == out[1], "two identical calls give different bytes"
            # total_out == NULL: the same device bytes
            d_off.upload(guard_o); d_hits.upload(guard_h)
            rc, t = call(pkg, ctx, b.result, d_rays.ptr, m, flags, d_off.ptr, d_hits.ptr, total + extra, total=False)
            assert rc == 0 and t == 0xDEAD
            ctx.synchronize()
            assert (d_off.download(np.uint32, m + 1 + extra).tobytes(), d_hits.download(pkg.HIT, total + extra).tobytes()) == out[0]
            assert d_rays.download(pkg.RAY, m).tobytes() == rays.tobytes()
        # n_rays == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        d_off.upload(guard_o); d_hits.upload(guard_h)
        assert call(pkg, ctx, b.result, d_rays.ptr, 0, HITS_SORTED, d_off.ptr, d_hits.ptr, total) == (0, 0)
        o = d_off.download(np.uint32, m + 1 + extra)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes() and d_hits.download(pkg.HIT, total + extra).tobytes() == guard_h.tobytes()
        # the Python binding: a capacity that is too small is re-allocated
        poff, phits = b.intersect_all(rays, sorted=True, capacity=3)
        assert poff.tobytes() == exp_off.tobytes() and phits.tobytes() == want[HITS_SORTED][1].tobytes()
    finally:
        d_rays.free(); d_off.free(); d_hits.free()


def left_first_stack(nodes, root, ni):
    """the deepest short stack of the all-hits walk (left child entered, right pushed) for a ray that passes every box"""
    deepest, work = 0, [(root, 0)]
    while work:
        v, st = work.pop()
        deepest = max(deepest, st)
        l, r = int(nodes["left"][v]), int(nodes["right"][v])
        if l < ni and r < ni:
            work.append((r, st)); work.append((l, st + 1))
        else:
            work.extend((c, st) for c in (l, r) if c < ni)
    return deepest


def chain_left(nodes, ni):
    """the same tree with the children of every node swapped where that makes the deeper internal child the left one: the left-first walk then holds one
    pushed sibling per level"""
    out = nodes.copy()

    def has_internal_child(v):
        return int(nodes["left"][v]) < ni or int(nodes["right"][v]) < ni
    for v in range(ni):
        l, r = int(nodes["left"][v]), int(nodes["right"][v])
        if l < ni and r < ni and has_internal_child(r) and not has_internal_child(l):
            out["left"][v], out["right"][v] = r, l
    return out


@pytest.mark.parametrize("H", [70, 250])
def test_deep_tree_takes_the_stackless_pass(pkg, H):
    tris, nodes, root, n = caterpillar(pkg, H, 3 + H)
    height, depth = tree_height_and_stack(nodes, root, n - 1, (0.0, 0.0, -1.0), (0.0, 0.0, 1.0))
    assert height > 64 and depth > 64, (height, depth)
    swapped = chain_left(nodes, n - 1)
    assert left_first_stack(swapped, root, n - 1) > 64
    rng = np.random.default_rng(H)
    m = 300
    rays = np.zeros(m, dtype=pkg.RAY)
    rays["origin"] = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), np.full(m, -1.0)], axis=1)
    rays["direction"] = np.stack([rng.normal(0, 1e-3, m), rng.normal(0, 1e-3, m), np.ones(m)], axis=1)
    rays["direction"][: m // 4, :2] = 0.0                     # exactly axis-parallel
    rays["tmax"] = 1e30                                       # (every ray reaches the far side nodes: it passes every chain box and every side box)
    rays["tmin"][m // 2:] = rng.uniform(0, 1000 + 2 * H, m - m // 2)
    ref = all_hits_brute_force(rays, tris)
    assert ref["well"].all() and ref["n_acc"].max() == n
    c = pkg.Context(0)
    try:
        c.reserve(n)
        d_tris = c.upload(tris)
        for label, arr in (("as made", nodes), ("chain left", swapped)):
            d_nodes = c.upload(arr)
            r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
            c.set_profiling(2)
            off, hits = all_hits(pkg, c, r, rays, HITS_SORTED)             # (asserts that the count-only and the fill call agree)
            kt = c.kernel_times()
            c.set_profiling(0)
            assert {"k_hits_count", "k_hits_fill", "k_hits_deep", "k_overlap_scan", "k_refit_plan"} <= set(kt), sorted(kt)
            assert off.tobytes() == ref["offsets"].tobytes() and hits.tobytes() == ref["hits"].tobytes(), f"H {H} {label}"
            uoff, uhits = all_hits(pkg, c, r, rays, 0)
            check_all_hits(rays, tris, ref, uoff, uhits, False, f"H {H} {label} unsorted")
            d_nodes.free()
        d_tris.free()
    finally:
        c.close()


@pytest.mark.parametrize("name", ["uniform_1000", "sponza_20000", "cornell382"])
def test_formats_give_identical_bytes(pkg, ctx, name):
    tris = mesh(pkg, name); n = len(tris)
    rays, _, ref = all_reference(pkg, ctx, name)
    b = pkg.HPLOC().build(ctx, tris)
    packed = np.ascontiguousarray(np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1).astype(np.float32).reshape(n, 9))
    uniq, inv = np.unique(packed.reshape(-1, 3), axis=0, return_inverse=True)
    idx = inv.reshape(-1).astype(np.uint32)
    d_p, d_v, d_i = ctx.upload(packed), ctx.upload(np.ascontiguousarray(uniq.astype(np.float32))), ctx.upload(idx)
    try:
        base = all_hits(pkg, ctx, b.result, rays, HITS_SORTED)
        check_all_hits(rays, tris, ref, base[0], base[1], True, name)
        p = all_hits(pkg, ctx, b.result, rays, HITS_SORTED, pkg.BuildInput(pkg.TRI_PACKED36, 30, d_p.ptr, None, None, 0, 0))
        i = all_hits(pkg, ctx, b.result, rays, HITS_SORTED, pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, len(uniq), 0))
        for other in (p, i):
            assert other[0].tobytes() == base[0].tobytes() and other[1].tobytes() == base[1].tobytes()
        py = b.intersect_all(rays, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED)
        assert py[0].tobytes() == base[0].tobytes() and py[1].tobytes() == base[1].tobytes()
        up = all_hits(pkg, ctx, b.result, rays, 0, pkg.BuildInput(pkg.TRI_PACKED36, 30, d_p.ptr, None, None, 0, 0))
        check_all_hits(rays, tris, ref, up[0], up[1], False, name + " packed unsorted")
    finally:
        for x in (d_p, d_v, d_i):
            x.free()


_MOVED = {}


def moved_reference(pkg):
    if not _MOVED:
        a = mesh(pkg, "uniform_20000"); moved = jitter(a, 17, 2e-3); other = mesh(pkg, "sponza_20000")
        rays, rays2 = make_rays(pkg, moved, 1024, 5), make_rays(pkg, other, 1024, 6)
        _MOVED["v"] = (a, moved, other, rays, rays2, all_hits_brute_force(rays, moved, workers=8), all_hits_brute_force(rays2, other, workers=8))
    return _MOVED["v"]


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_after_refit_optimize_and_rebuild(pkg, algo):
    a, moved, other, rays, rays2, ref, ref2 = moved_reference(pkg)
    assert ref["well"].mean() >= 0.99 and ref2["well"].mean() >= 0.99
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        b.intersect_all(rays, count_only=True)                # (the plan of the ctx's own tree is made here and kept)
        b.refit(moved)
        off, hits = b.intersect_all(rays)
        check_all_hits(rays, moved, ref, off, hits, True, f"refit algo {algo}")
        uoff, uhits = b.intersect_all(rays, sorted=False)
        check_all_hits(rays, moved, ref, uoff, uhits, False, f"refit algo {algo} unsorted")
        b.optimize(3)
        ooff, ohits = b.intersect_all(rays)
        check_all_hits(rays, moved, ref, ooff, ohits, True, f"optimised algo {algo}")
        w = ref["well"]
        assert (np.diff(ooff.astype(np.int64)) == np.diff(off.astype(np.int64)))[w].all()
        assert ohits[w[slice_rays(ooff)]].tobytes() == hits[w[slice_rays(off)]].tobytes(), "bvh_optimize changed the answers"
        b2 = pkg.BUILDERS[algo]().build(c, other)
        off2, hits2 = b2.intersect_all(rays2)
        check_all_hits(rays2, other, ref2, off2, hits2, True, f"rebuild algo {algo}")
    finally:
        c.close()


@pytest.mark.parametrize("name", MESHES)
def test_consistent_with_closest_hit(pkg, ctx, name):
    tris = mesh(pkg, name)
    rays, bf, ref = all_reference(pkg, ctx, name)
    well = ref["well"]
    for algo in (0, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        closest = query(pkg, ctx, b.result, rays, pkg.QUERY_CLOSEST)
        off, hits = all_hits(pkg, ctx, b.result, rays, HITS_SORTED)
        empty = np.diff(off.astype(np.int64)) == 0
        assert (empty == (closest["prim"] == pkg.INVALID))[well].all(), f"{name} algo {algo}: empty slices and closest-hit misses differ"
        has = ~empty & well
        assert hits[off[:-1][has]].tobytes() == closest[has].tobytes(), f"{name} algo {algo}: first sorted record != bvh_intersect closest"


def test_errors_write_nothing(pkg):
    tris = mesh(pkg, "uniform_1000"); n = len(tris)
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        rays = make_rays(pkg, tris, 256, 4)
        d_rays = c.upload(rays)
        cap = 4096
        guard_h = np.frombuffer(np.full(cap * 16, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.HIT)
        guard_o = np.full(257, 0x5A5A5A5A, dtype=np.uint32)
        hits, offs = c.upload(guard_h), c.upload(guard_o)
        L = pkg.lib()
        tot = C.c_uint64(0x77)

        def go(res=b.result, inp=None, r=d_rays.ptr, m=256, flags=HITS_SORTED, o=offs.ptr, h=hits.ptr, k=cap, ctx=c.handle):
            return L.bvh_intersect_all(ctx, C.byref(res) if res is not None else None, C.byref(inp) if inp is not None else None, r, m, flags, o, h, k, C.byref(tot))

        def variant(**kw):
            r = pkg.Result.from_buffer_copy(b.result)
            for k, v in kw.items():
                setattr(r, k, v)
            return r
        cases = {
            "null ctx": go(ctx=None), "null tree": go(res=None), "null rays": go(r=None), "null offsets": go(o=None),
            "n_leaves 1": go(res=variant(n_leaves=1)), "layout 2": go(res=variant(layout=2)), "null nodes": go(res=variant(d_nodes=None)),
            "layout 1 without leaves": go(res=variant(d_leaves=None)), "root not internal": go(res=variant(root=n - 1)),
            "no triangles": go(res=variant(d_tris=None)), "bad format": go(inp=pkg.BuildInput(7, 30, b.result.d_tris, None, None, 0, 0)),
            "packed unaligned": go(inp=pkg.BuildInput(pkg.TRI_PACKED36, 30, b.result.d_tris + 4, None, None, 0, 0)),
            "indexed without vertices": go(inp=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, None, b.result.d_tris, 3, 0)),
            "flag 2": go(flags=2), "flag 3": go(flags=3), "flag high": go(flags=0x80000000),
            "n_rays 2^30": go(m=1 << 30),
            "offsets in rays": go(o=d_rays.ptr + 64), "hits in rays": go(h=d_rays.ptr + 32), "hits in offsets": go(h=offs.ptr + 16),
            "offsets in hits": go(o=hits.ptr + 16 * (cap - 1)), "rays in hits": go(r=hits.ptr, h=hits.ptr + 16 * 8),
            "above capacity": go(res=variant(n_leaves=n + 1_000_000, root=0)),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        assert tot.value == 0x77
        c.synchronize()
        assert hits.download(pkg.HIT, cap).tobytes() == guard_h.tobytes() and offs.download(np.uint32, 257).tobytes() == guard_o.tobytes()
        # ranges that only touch are fine, and a count-only call ignores the capacity's range
        assert go(h=None, k=1 << 40) == 0 and tot.value != 0x77
        # on a fresh ctx (capacity 0) a caller tree is refused until bvh_ctx_reserve
        offs.upload(guard_o)
        c2 = pkg.Context(0)
        try:
            assert go(ctx=c2.handle) == E_INVALID
        finally:
            c2.close()
        assert hits.download(pkg.HIT, cap).tobytes() == guard_h.tobytes() and offs.download(np.uint32, 257).tobytes() == guard_o.tobytes()
        d_rays.free(); hits.free(); offs.free()
    finally:
        c.close()


def test_one_large_size(pkg, ctx):
    n, m = 2_000_000, 65_536
    tris = no_negzero(pkg.meshgen.uniform(n, 9))
    rng = np.random.default_rng(31)
    v = np.concatenate([tris["v1"][::97], tris["v2"][::97], tris["v3"][::97]]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = hi - lo
    # through-rays: from a point on a sphere around the scene through a random point of its box, no tmax
    centre, radius = 0.5 * (lo + hi), float(np.linalg.norm(ext))
    u = rng.normal(size=(m, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = centre + radius * u
    d = (lo + rng.random((m, 3)) * ext) - o
    rays = np.zeros(m, dtype=pkg.RAY)
    rays["origin"] = o.astype(np.float32); rays["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays["tmax"] = np.float32(3.0e38)
    b = pkg.HPLOC().build(ctx, tris)
    off, hits = b.intersect_all(rays, sorted=True)
    counts = np.diff(off.astype(np.int64))
    assert off[0] == 0 and off[-1] == len(hits) and counts.max() >= 2
    ray = slice_rays(off)
    nxt = ray[1:] == ray[:-1]
    t, p = hits["t"], hits["prim"]
    assert ((t[1:] > t[:-1]) | ((t[1:] == t[:-1]) & (p[1:] > p[:-1])))[nxt].all(), "a sorted slice is not strictly ascending"
    assert b.intersect_all(rays, count_only=True).tobytes() == off.tobytes()
    sample = np.sort(rng.choice(m, 512, replace=False))
    ref = all_hits_brute_force(rays[sample], tris, chunk_elems=1 << 21, workers=16)
    w = ref["well"]
    assert w.mean() >= 0.99
    assert (counts[sample] == ref["n_acc"])[w].all(), f"counts differ on {np.count_nonzero((counts[sample] != ref['n_acc']) & w)} sampled rays"
    sel = np.isin(ray, sample[w])
    assert hits[sel].tobytes() == ref["hits"][w[slice_rays(ref["offsets"])]].tobytes()
