"""bvh_radius_tris on the GPU: every tree triangle within the radius of every query triangle, from every builder, both node layouts and all three triangle
formats on either side, against the numpy brute force (tests/test_radius_tris.py) byte for byte: sorted and unsorted fills, count-only calls, the capacity
decision, the self mode with and without BVH_RADIUS_TRIS_SKIP_SHARED, a closed mesh, the stackless pass on trees deeper than the short stack, calls after a
refit, an optimise and a rebuild, caller-owned trees, consistency with bvh_closest_tris and bvh_intersect_tris, buffer hygiene and errors.  All shapes are
small: the brute force is every query triangle against every tree triangle, 15 terms each, computed once per input and shared across radii and tests."""
import ctypes as C

import numpy as np
import pytest

from test_closest_tris import CROSSING, E_INVALID, pair_matrix
from test_gpu_closest_tris import extent, formats_of, make_queries
from test_gpu_closest_tris import raw as closest_raw
from test_gpu_multihit import chain_left
from test_gpu_point_query import first_descent_pushes
from test_gpu_query import caterpillar, lbvh_result, mesh
from test_gpu_refit import jitter
from test_intersect_tris import as_triangles, tt_mesh, xyz
from test_radius_tris import radius_tris_brute_force, recompute_records

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

F32 = np.float32
TREES = [f"uniform_{n}" for n in (2, 3, 63, 64, 65, 1000)] + ["sponza_1000", "cornell32", "cornell82", "cornell382"]
SELF_TREES = ["uniform_65", "uniform_1000", "sponza_1000", "cornell382"]
SELF_RADII = ("zero", "band", "wide")


def radii(tris):
    d = extent(tris)[2]
    return {"zero": 0.0, "band": 2e-3 * d, "wide": 5e-2 * d, "inf": np.inf, "negative": -1.0, "nan": np.nan}


_REF, _SELF = {}, {}


def reference(pkg, name, tris=None, seed=None):
    """(queries, {radius label: (radius, brute force)}) per input, computed once, shared and never changed"""
    if name not in _REF:
        tris = mesh(pkg, name) if tris is None else tris
        q = make_queries(pkg, tris, 17 + len(tris) if seed is None else seed)
        pairs = pair_matrix(q, tris)
        _REF[name] = (q, {label: (r, radius_tris_brute_force(pkg, q, tris, r, pairs)) for label, r in radii(tris).items()})
    return _REF[name]


def self_reference(pkg, name, tris=None):
    """{(radius label, skip_shared): (radius, brute force)} of a mesh against itself, j > i"""
    if name not in _SELF:
        tris = mesh(pkg, name) if tris is None else tris
        pairs = pair_matrix(tris, tris)
        r = radii(tris)
        _SELF[name] = {(label, skip): (r[label], radius_tris_brute_force(pkg, tris, tris, r[label], pairs, self_pairs=True, skip_shared=skip))
                       for label in SELF_RADII for skip in (False, True)}
    return _SELF[name]


def padded(pkg, buf):
    return pkg.BuildInput(pkg.TRI_PADDED64, 30, buf.ptr, None, None, 0, 0)


def call(pkg, ctx, result, qin, m, radius, flags, d_offsets, d_hits, capacity, total=True, tin=None):
    t = C.c_uint64(0xDEAD)
    rc = pkg.lib().bvh_radius_tris(ctx.handle, C.byref(result), C.byref(tin) if tin is not None else None, C.byref(qin) if qin is not None else None, m, radius,
                                   flags, d_offsets, d_hits, capacity, C.byref(t) if total else None)
    return rc, t.value


def search(pkg, ctx, result, qin, m, radius, flags, tin=None):
    """a count-only call, then a fill with the exact capacity; returns (offsets, hits).  The count-only offsets must equal the fill's."""
    d_off = ctx.alloc((m + 1) * 4)
    hits = None
    try:
        rc, total = call(pkg, ctx, result, qin, m, radius, flags, d_off.ptr, None, 0, tin=tin)
        assert rc == 0, rc
        counted = d_off.download(np.uint32, m + 1)
        assert counted[0] == 0 and counted[-1] == total
        hits = ctx.alloc(max(total, 1) * 16)
        rc, total2 = call(pkg, ctx, result, qin, m, radius, flags, d_off.ptr, hits.ptr, total, tin=tin)
        assert rc == 0 and total2 == total
        off = d_off.download(np.uint32, m + 1)
        assert off.tobytes() == counted.tobytes(), "count-only and fill calls disagree on the offsets"
        return off, hits.download(pkg.TRI_HIT, total)
    finally:
        d_off.free()
        if hits is not None:
            hits.free()


def host_sorted(off, hits):
    """each slice put into ascending (dist2, prim) order on the host"""
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    return hits[np.lexsort((hits["prim"], hits["dist2"], rows))]


def same(got, bf):
    return got[0].tobytes() == bf["offsets"].tobytes() and got[1].tobytes() == bf["hits"].tobytes()


def results_of(pkg, ctx, b, keep):
    out = [("as built", b.result)]
    if b.result.layout == 1:
        out.append(("lbvh layout", lbvh_result(pkg, ctx, b, keep)))
    return out


@pytest.mark.parametrize("name", TREES)
def test_exact_against_brute_force(pkg, ctx, name):
    tris = mesh(pkg, name)
    q, ref = reference(pkg, name)
    m = len(q)
    for label, (_, bf) in ref.items():
        assert bf["well"].mean() == 1.0 and bf["ill_pairs"] == 0, f"{name} radius {label}: {bf['ill_pairs']} ill-conditioned pairs"
    assert len(ref["negative"][1]["hits"]) == 0 and len(ref["nan"][1]["hits"]) == 0 and int(ref["inf"][1]["offsets"][-1]) == (m - 8) * len(tris)
    assert 0 < len(ref["zero"][1]["hits"]) < len(ref["band"][1]["hits"]) < len(ref["wide"][1]["hits"]) <= len(ref["inf"][1]["hits"])
    assert (ref["zero"][1]["hits"]["feature"] == CROSSING).any()
    print(f"{name}: records " + ", ".join(f"{label} {len(bf['hits'])} (longest slice {int(bf['counts'].max())})" for label, (_, bf) in ref.items()))
    d_q = ctx.upload(q)
    try:
        qin = padded(pkg, d_q)
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, tris)
            keep = []
            for where, res in results_of(pkg, ctx, b, keep):
                for label, (radius, bf) in ref.items():
                    what = f"{name} algo {algo} {where} radius {label}"
                    got = search(pkg, ctx, res, qin, m, radius, pkg.RADIUS_TRIS_SORTED)      # (asserts that the count-only offsets equal the fill call's)
                    assert same(got, bf), what
                    if where == "as built" and label in ("zero", "band", "wide"):
                        uoff, uhits = search(pkg, ctx, res, qin, m, radius, 0)
                        assert uoff.tobytes() == bf["offsets"].tobytes(), what + ": the unsorted call counts differently"
                        assert host_sorted(uoff, uhits).tobytes() == bf["hits"].tobytes(), what + ": the unsorted fill is another set"
                        assert recompute_records(pkg, q, tris, radius, uoff, uhits) is None, what
            if algo == 3:                                                                       # the unsorted fill with the longest slices, once per input
                radius, bf = ref["inf"]
                uoff, uhits = search(pkg, ctx, b.result, qin, m, radius, 0)
                assert uoff.tobytes() == bf["offsets"].tobytes() and host_sorted(uoff, uhits).tobytes() == bf["hits"].tobytes()
            for k in keep:
                k.free()
    finally:
        d_q.free()


def test_binding(pkg, ctx):
    tris = mesh(pkg, "sponza_1000")
    q, ref = reference(pkg, "sponza_1000")
    b = pkg.SinglePassLbvh().build(ctx, tris)
    d_q = ctx.upload(q)
    try:
        for label in ("zero", "band", "wide", "nan"):
            radius, bf = ref[label]
            assert same(b.radius_tris(q, radius=radius), bf)
            assert same(b.radius_tris(d_q, radius=radius), bf)                                   # a device buffer of TRIANGLE records
            assert same(b.radius_tris(xyz(q).reshape(-1, 9), radius=radius), bf)                 # host floats: uploaded as PACKED36
            assert b.radius_tris(q, radius=radius, count_only=True).tobytes() == bf["offsets"].tobytes()
            uoff, uhits = b.radius_tris(q, radius=radius, sorted=False)
            assert uoff.tobytes() == bf["offsets"].tobytes() and host_sorted(uoff, uhits).tobytes() == bf["hits"].tobytes() and uhits.dtype == pkg.TRI_HIT
        bf = ref["wide"][1]
        assert same(b.radius_tris(q, radius=ref["wide"][0], capacity=3), bf)                     # a capacity that is too small is re-allocated
        off, hits = b.radius_tris(q[:0], radius=1.0)
        assert off.tolist() == [0] and len(hits) == 0 and b.radius_tris(q[:0], radius=1.0, count_only=True).tolist() == [0]
        with pytest.raises(pkg.BvhError):
            b.radius_tris(q, radius=1.0, self_pairs=True)                                        # self_pairs takes no other mesh
        with pytest.raises(pkg.BvhError):
            b.radius_tris(radius=1.0)                                                            # another mesh is required
        sref = self_reference(pkg, "sponza_1000")
        for (label, skip), (radius, sbf) in sref.items():
            assert same(b.radius_tris(self_pairs=True, skip_shared=skip, radius=radius), sbf), (label, skip)
        split = pkg.HPLOC().build_split(ctx, tris, sa_max=1.0)
        with pytest.raises(pkg.BvhError):
            split.radius_tris(self_pairs=True, radius=0.1)                                       # more leaves than triangles
    finally:
        d_q.free()


@pytest.mark.parametrize("name", SELF_TREES)
def test_self_mode_against_brute_force(pkg, ctx, name):
    tris = mesh(pkg, name); n = len(tris)
    sref = self_reference(pkg, name)
    for (label, skip), (_, bf) in sref.items():
        assert bf["ill_pairs"] == 0 and bf["well"].all()
    print(f"{name} self: " + ", ".join(f"{label}{' skip' if skip else ''} {len(bf['hits'])}" for (label, skip), (_, bf) in sref.items()))
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        keep = []
        for where, res in results_of(pkg, ctx, b, keep):
            for (label, skip), (radius, bf) in sref.items():
                flags = pkg.RADIUS_TRIS_SELF | (pkg.RADIUS_TRIS_SKIP_SHARED if skip else 0)
                what = f"{name} self algo {algo} {where} radius {label} skip {skip}"
                assert same(search(pkg, ctx, res, None, n, radius, flags | pkg.RADIUS_TRIS_SORTED), bf), what
                if where == "as built" and algo in (1, 3):
                    uoff, uhits = search(pkg, ctx, res, None, n, radius, flags)
                    assert uoff.tobytes() == bf["offsets"].tobytes() and host_sorted(uoff, uhits).tobytes() == bf["hits"].tobytes(), what + " unsorted"
                    assert recompute_records(pkg, tris, tris, radius, uoff, uhits, True, skip) is None, what
        for k in keep:
            k.free()


def test_cornell382_radius_zero_self_pairs(pkg, ctx):
    """at radius 0, 2 084 pairs j > i of cornell382 touch or cross, 2 062 of them share a vertex: BVH_RADIUS_TRIS_SKIP_SHARED leaves 22"""
    sref = self_reference(pkg, "cornell382")
    assert len(sref[("zero", False)][1]["hits"]) == 2084 and len(sref[("zero", True)][1]["hits"]) == 22
    b = pkg.HPLOC().build(ctx, mesh(pkg, "cornell382"))
    off, hits = b.radius_tris(self_pairs=True, skip_shared=True, radius=0.0)
    assert len(hits) == 22 and same((off, hits), sref[("zero", True)][1])
    assert int(b.radius_tris(self_pairs=True, skip_shared=False, radius=0.0, count_only=True)[-1]) == 2084


def test_closed_mesh_shares_vertices_bitwise(pkg, ctx):
    tris = tt_mesh(pkg, "bunny_1280"); n = len(tris)
    pairs = pair_matrix(tris, tris)
    diag = extent(tris)[2]
    b = pkg.HPLOC().build(ctx, tris)
    for radius in (0.0, 2e-3 * diag, 5e-2 * diag):
        for skip in (True, False):
            bf = radius_tris_brute_force(pkg, tris, tris, radius, pairs, self_pairs=True, skip_shared=skip)
            assert bf["ill_pairs"] == 0
            got = b.radius_tris(self_pairs=True, skip_shared=skip, radius=radius)
            print(f"bunny_1280 self radius {radius:.4g} skip_shared {skip}: {len(got[1])} pairs (brute force {len(bf['hits'])}), "
                  f"{int((got[1]['feature'] == CROSSING).sum())} crossings")
            assert same(got, bf), (radius, skip)
    assert int(b.radius_tris(self_pairs=True, skip_shared=False, radius=0.0, count_only=True)[-1]) >= 3 * n // 2       # every edge of a closed mesh is shared


@pytest.mark.parametrize("name", ["uniform_1000", "cornell382"])
def test_formats_give_identical_bytes(pkg, ctx, name):
    tris = mesh(pkg, name); n = len(tris)
    q, ref = reference(pkg, name)
    sref = self_reference(pkg, name)
    b = pkg.HPLOC().build(ctx, tris)
    tf, tbuf = formats_of(pkg, ctx, tris)
    qf, qbuf = formats_of(pkg, ctx, q)
    try:
        for label in ("band", "wide"):
            radius, bf = ref[label]
            for tn, tin in tf.items():
                for qn, qin in qf.items():
                    assert same(search(pkg, ctx, b.result, qin, len(q), radius, pkg.RADIUS_TRIS_SORTED, tin), bf), f"{name} radius {label}: tree {tn} / queries {qn}"
            u = search(pkg, ctx, b.result, qf["indexed"], len(q), radius, 0, tf["packed"])
            assert u[0].tobytes() == bf["offsets"].tobytes() and host_sorted(*u).tobytes() == bf["hits"].tobytes()
        for skip in (False, True):                                                               # the self rules compare coordinates, not indices: every format
            radius, bf = sref[("band", skip)]
            flags = pkg.RADIUS_TRIS_SORTED | pkg.RADIUS_TRIS_SELF | (pkg.RADIUS_TRIS_SKIP_SHARED if skip else 0)
            for tn, tin in tf.items():
                assert same(search(pkg, ctx, b.result, None, n, radius, flags, tin), bf), f"{name} self skip {skip}: tree {tn}"
    finally:
        for x in tbuf + qbuf:
            x.free()


def caterpillar_queries(pkg, H, m=192):
    """small triangles below the face at z = 0 (every box passes an unbounded query: the left-first descent pushes at every chain node), some coplanar with it,
    some through both near faces, and some among the far triangles"""
    rng = np.random.default_rng(H)
    c = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-3, -0.5, m)], axis=1)
    c[: m // 6, 2] = 0.25
    c[3 * m // 4:, 2] = rng.uniform(1000, 1000 + 2 * H, m - 3 * m // 4)
    q = c[:, None, :] + rng.normal(0, 0.05, (m, 3, 3))
    q[m // 6: m // 3, :, 2] = 0.0
    q[m // 3: m // 2, 0, 2] = 0.75; q[m // 3: m // 2, 1:, 2] = -0.5
    return as_triangles(pkg, q.astype(F32))


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("H", [70, 250])
def test_deep_tree_takes_the_stackless_pass(pkg, H, layout):
    tris, made, root, n = caterpillar(pkg, H, 5 + H)
    nodes = chain_left(made, n - 1)                           # the chain below every left link: the left-first walk holds one pushed side node per level
    q = caterpillar_queries(pkg, H)
    m = len(q)
    cen = xyz(q).astype(np.float64).mean(axis=1)
    # (below the faces the chain child is also the nearer one: the near-first descent of first_descent_pushes is this walk's left-first descent)
    assert min(first_descent_pushes(nodes, root, n - 1, cen[j]) for j in range(m // 6)) > 64
    pairs = pair_matrix(q, tris)
    c = pkg.Context(0)
    try:
        c.reserve(n)
        bufs = [c.upload(tris), c.upload(q)]
        r = pkg.Result(); r.d_tris = bufs[0].ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = layout
        if layout == 0:
            bufs.append(c.upload(nodes)); r.d_nodes = bufs[-1].ptr
        else:
            leaves = np.zeros(n, dtype=pkg.PRIMREF)
            leaves["prim"] = nodes["left"][n - 1:]; leaves["min"] = nodes["min"][n - 1:]; leaves["max"] = nodes["max"][n - 1:]
            bufs += [c.upload(np.ascontiguousarray(nodes[: n - 1])), c.upload(leaves)]
            r.d_nodes = bufs[-2].ptr; r.d_leaves = bufs[-1].ptr
        qin = padded(pkg, bufs[1])
        for radius in (np.inf, 5000.0, 5.0, 0.0):
            bf = radius_tris_brute_force(pkg, q, tris, radius, pairs)
            assert bf["ill_pairs"] == 0 and len(bf["hits"]) > 0
            if radius >= 5000.0:
                assert (bf["counts"][: m // 6] == n).all()   # the overflowing queries accept every triangle: the stackless pass must find them all, twice
            c.set_profiling(2)
            got = search(pkg, c, r, qin, m, radius, pkg.RADIUS_TRIS_SORTED)          # count and fill: each takes the stackless pass
            kt = c.kernel_times()
            c.set_profiling(0)
            assert {"k_radius_tris_walk", "k_radius_tris_deep", "k_overlap_scan", "k_refit_plan"} <= set(kt), sorted(kt)
            assert same(got, bf), f"H {H} layout {layout} radius {radius}"
            u = search(pkg, c, r, qin, m, radius, 0)
            assert u[0].tobytes() == bf["offsets"].tobytes() and host_sorted(*u).tobytes() == bf["hits"].tobytes()
        # self mode through the stackless pass: the caterpillar against itself, every face within reach of every other
        sbf = radius_tris_brute_force(pkg, tris, tris, np.inf, self_pairs=True, skip_shared=True)
        assert len(sbf["hits"]) == n * (n - 1) // 2
        assert same(search(pkg, c, r, None, n, np.inf, pkg.RADIUS_TRIS_SORTED | pkg.RADIUS_TRIS_SELF | pkg.RADIUS_TRIS_SKIP_SHARED), sbf)
        for b in bufs:
            b.free()
    finally:
        c.close()


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_after_refit_optimize_and_rebuild(pkg, algo):
    a = mesh(pkg, "uniform_1000"); moved = jitter(a, 19, 2e-3)
    other = mesh(pkg, "sponza_1000")
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        q, ref = reference(pkg, "uniform_1000_jittered", moved, 8)
        b.radius_tris(q, radius=0.0, count_only=True)         # (the plan of the ctx's own tree is made here and kept)
        b.refit(moved)
        for label in ("zero", "band", "wide"):
            radius, bf = ref[label]
            assert bf["ill_pairs"] == 0
            assert same(b.radius_tris(q, radius=radius), bf), f"refit algo {algo} radius {label}"
        b.optimize(3)
        for label in ("zero", "band", "wide"):
            radius, bf = ref[label]
            assert same(b.radius_tris(q, radius=radius), bf), f"optimize algo {algo} radius {label}"
        sbf = radius_tris_brute_force(pkg, moved, moved, ref["band"][0], self_pairs=True, skip_shared=True) if algo == 3 else None
        if sbf is not None:
            assert same(b.radius_tris(self_pairs=True, radius=ref["band"][0]), sbf)
        b2 = pkg.BUILDERS[algo]().build(c, other)
        q2, ref2 = reference(pkg, "sponza_1000")
        for label in ("zero", "band", "wide"):
            radius, bf = ref2[label]
            assert same(b2.radius_tris(q2, radius=radius), bf), f"rebuild algo {algo} radius {label}"
    finally:
        c.close()


def test_caller_owned_trees_use_a_per_call_plan(pkg):
    """two caller-owned layout-0 copies of different trees and the ctx's own tree, queried in turn on one ctx: each call must walk with its own tree's plan"""
    ta, tb = mesh(pkg, "uniform_1000"), mesh(pkg, "sponza_1000")
    qa, ra = reference(pkg, "uniform_1000"); qb, rb = reference(pkg, "sponza_1000")
    c = pkg.Context(0)
    try:
        ba = pkg.PLOCNew().build(c, ta)
        keep = []
        ca = lbvh_result(pkg, c, ba, keep)
        d_ta = c.upload(ta); ca.d_tris = d_ta.ptr
        bb = pkg.PLOCNew().build(c, tb)                       # the ctx's own tree is now b's; a's arrays live on in the caller's buffer
        cb = lbvh_result(pkg, c, bb, keep)
        d_qa, d_qb = c.upload(qa), c.upload(qb)
        for _ in range(2):
            for res, q, d_q, ref in ((ca, qa, d_qa, ra), (bb.result, qb, d_qb, rb), (cb, qb, d_qb, rb), (ca, qa, d_qa, ra)):
                radius, bf = ref["wide"]
                c.set_profiling(2)
                got = search(pkg, c, res, padded(pkg, d_q), len(q), radius, pkg.RADIUS_TRIS_SORTED)
                kt = c.kernel_times()
                c.set_profiling(0)
                assert same(got, bf)
                if res is not bb.result:
                    assert "k_refit_plan" in kt               # caller-owned arrays: the plan is made on every call
        for x in keep + [d_ta, d_qa, d_qb]:
            x.free()
    finally:
        c.close()


@pytest.mark.parametrize("name", ["uniform_1000", "cornell382", "sponza_1000"])
def test_consistent_with_closest_tris_and_intersect_tris(pkg, ctx, name):
    tris = mesh(pkg, name)
    q, ref = reference(pkg, name)
    m = len(q)
    b = pkg.HPLOC().build(ctx, tris)
    d_q = ctx.upload(q)
    try:
        for label, (radius, bf) in ref.items():
            off, hits = b.radius_tris(d_q, radius=radius)
            closest = closest_raw(pkg, ctx, b.result, d_q, m, radius, pkg.QUERY_CLOSEST)
            has = np.diff(off.astype(np.int64)) > 0
            assert (has == (closest["prim"] != pkg.INVALID)).all(), f"{name} radius {label}: a non-empty slice and a closest hit differ"
            assert hits[off[:-1][has]].tobytes() == closest[has].tobytes(), f"{name} radius {label}: the first sorted record is not bvh_closest_tris's"
        # the records with feature 15 at radius 0 are exactly bvh_intersect_tris's set, query by query
        off, hits = b.radius_tris(d_q, radius=0.0)
        rows = np.repeat(np.arange(m), np.diff(off.astype(np.int64)))
        cross = hits["feature"] == CROSSING
        assert cross.any() and (hits["dist2"] == 0).all()
        toff, tprims = b.intersect_tris(q)
        trows = np.repeat(np.arange(m), np.diff(toff.astype(np.int64)))
        print(f"{name}: {int(cross.sum())} crossing records of {len(hits)} at radius 0")
        assert sorted(zip(rows[cross].tolist(), hits["prim"][cross].tolist())) == sorted(zip(trows.tolist(), tprims.tolist()))
    finally:
        d_q.free()


def test_passes_capacity_and_bounds(pkg, ctx):
    name = "cornell382"
    tris = mesh(pkg, name)
    q, ref = reference(pkg, name)
    radius, bf = ref["wide"]
    m = len(q) - 5                                            # (a count that is no multiple of the workgroup)
    bf = radius_tris_brute_force(pkg, q[:m], tris, radius)
    exp_off, total = bf["offsets"], int(bf["offsets"][-1])
    assert total > 1000
    b = pkg.HPLOC().build(ctx, tris)
    extra = 29
    guard_h = np.frombuffer(np.full((total + 2 * extra) * 16, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.TRI_HIT)
    guard_o = np.full(m + 1 + 2 * extra, 0xA5A5A5A5, dtype=np.uint32)
    d_q, d_off, d_hits = ctx.upload(q), ctx.upload(guard_o), ctx.upload(guard_h)
    qin = padded(pkg, d_q)
    po, ph = d_off.ptr + 4 * extra, d_hits.ptr + 16 * extra  # guard bands in front of and behind both arrays

    def state():
        o, h = d_off.download(np.uint32, len(guard_o)), d_hits.download(pkg.TRI_HIT, len(guard_h))
        assert o[:extra].tobytes() == guard_o[:extra].tobytes() and o[extra + m + 1:].tobytes() == guard_o[extra + m + 1:].tobytes(), "a guard word around d_offsets"
        assert h[:extra].tobytes() == guard_h[:extra].tobytes() and h[extra + total:].tobytes() == guard_h[extra + total:].tobytes(), "a guard record around d_hits"
        return o[extra: extra + m + 1], h[extra: extra + total]
    try:
        for flags in (pkg.RADIUS_TRIS_SORTED, 0):
            out = {}
            # d_hits == NULL counts only: offsets complete, d_hits untouched
            d_off.upload(guard_o); d_hits.upload(guard_h)
            assert call(pkg, ctx, b.result, qin, m, radius, flags, po, None, 0) == (0, total)
            o, h = state()
            assert o.tobytes() == exp_off.tobytes() and h.tobytes() == guard_h[extra: extra + total].tobytes()
            # capacity total - 1: the fill is skipped, d_hits untouched byte for byte, d_offsets still complete, *total_out set
            d_off.upload(guard_o)
            assert call(pkg, ctx, b.result, qin, m, radius, flags, po, ph, total - 1) == (0, total)
            o, h = state()
            assert o.tobytes() == exp_off.tobytes() and h.tobytes() == guard_h[extra: extra + total].tobytes()
            # the exact capacity is filled; twice the same bytes
            for rnd in range(2):
                d_off.upload(guard_o); d_hits.upload(guard_h)
                assert call(pkg, ctx, b.result, qin, m, radius, flags, po, ph, total) == (0, total)
                o, h = state()
                assert o.tobytes() == exp_off.tobytes()
                assert (h if flags else host_sorted(o, h)).tobytes() == bf["hits"].tobytes()
                assert recompute_records(pkg, q[:m], tris, radius, o, h) is None
                out[rnd] = (o.tobytes(), h.tobytes())
            assert out[0] == out[1], "two identical calls give different bytes"
            # total_out == NULL: the same device bytes, nothing stored on the host
            d_off.upload(guard_o); d_hits.upload(guard_h)
            rc, t = call(pkg, ctx, b.result, qin, m, radius, flags, po, ph, total + extra, total=False)
            assert rc == 0 and t == 0xDEAD
            ctx.synchronize()
            o, h = state()
            assert (o.tobytes(), h.tobytes()) == out[0]
            assert d_q.download(pkg.meshgen.TRIANGLE, len(q)).tobytes() == q.tobytes()
        # n_queries == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        d_off.upload(guard_o); d_hits.upload(guard_h)
        assert call(pkg, ctx, b.result, qin, 0, radius, pkg.RADIUS_TRIS_SORTED, po, ph, total) == (0, 0)
        ctx.synchronize()
        o = d_off.download(np.uint32, len(guard_o))
        assert o[extra] == 0 and o[:extra].tobytes() == guard_o[:extra].tobytes() and o[extra + 1:].tobytes() == guard_o[extra + 1:].tobytes()
        assert d_hits.download(pkg.TRI_HIT, len(guard_h)).tobytes() == guard_h.tobytes()
    finally:
        d_q.free(); d_off.free(); d_hits.free()


def test_errors_write_nothing(pkg):
    tris = mesh(pkg, "uniform_1000"); n = len(tris)
    q, _ = reference(pkg, "uniform_1000")
    m = 256
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        d_q = c.upload(q)
        d_v, d_i = c.upload(np.ascontiguousarray(xyz(q).reshape(-1, 3))), c.upload(np.arange(3 * len(q), dtype=np.uint32))
        cap = 4096
        guard_h = np.frombuffer(np.full(cap * 16, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.TRI_HIT)
        guard_o = np.full(n + 1, 0x5A5A5A5A, dtype=np.uint32)
        hits, offs = c.upload(guard_h), c.upload(guard_o)
        L = pkg.lib()
        tot = C.c_uint64(0x77)
        pad = padded(pkg, d_q)
        indexed = pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, 3 * len(q), 0)
        none = object()
        S, SELF, SKIP = pkg.RADIUS_TRIS_SORTED, pkg.RADIUS_TRIS_SELF, pkg.RADIUS_TRIS_SKIP_SHARED

        def go(res=b.result, inp=None, qin=pad, k=m, radius=1.0, flags=S, o=offs.ptr, h=hits.ptr, cap_=cap, ctx=c.handle):
            return L.bvh_radius_tris(ctx, C.byref(res) if res is not None else None, C.byref(inp) if inp is not None else None,
                                     C.byref(qin) if qin is not none else None, k, radius, flags, o, h, cap_, C.byref(tot))

        def variant(**kw):
            r = pkg.Result.from_buffer_copy(b.result)
            for key, v in kw.items():
                setattr(r, key, v)
            return r
        nodes_bytes = (n - 1) * 32
        cases = {
            "null ctx": go(ctx=None), "null tree": go(res=None), "null offsets": go(o=None), "null queries": go(qin=none),
            "n_leaves 1": go(res=variant(n_leaves=1)), "layout 2": go(res=variant(layout=2)), "null nodes": go(res=variant(d_nodes=None)),
            "layout 1 without leaves": go(res=variant(d_leaves=None)), "root not internal": go(res=variant(root=n - 1)),
            "no triangles": go(res=variant(d_tris=None)), "bad tree format": go(inp=pkg.BuildInput(7, 30, b.result.d_tris, None, None, 0, 0)),
            "tree packed unaligned": go(inp=pkg.BuildInput(pkg.TRI_PACKED36, 30, b.result.d_tris + 4, None, None, 0, 0)),
            "tree indexed without vertices": go(inp=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, None, b.result.d_tris, 3, 0)),
            "bad query format": go(qin=pkg.BuildInput(7, 30, d_q.ptr, None, None, 0, 0)),
            "queries null tris": go(qin=pkg.BuildInput(pkg.TRI_PADDED64, 30, None, None, None, 0, 0)),
            "queries packed unaligned": go(qin=pkg.BuildInput(pkg.TRI_PACKED36, 30, d_q.ptr + 4, None, None, 0, 0)),
            "queries indexed without indices": go(qin=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, None, 3 * len(q), 0)),
            "queries indexed n_vertices 0": go(qin=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, 0, 0)),
            "flag 8": go(flags=8), "flag high": go(flags=S | 0x80000000), "skip without self": go(flags=SKIP), "sorted skip without self": go(flags=S | SKIP),
            "self with queries": go(flags=SELF, k=n), "self with another count": go(qin=none, flags=SELF | SKIP, k=n - 1),
            "too many queries": go(k=1 << 30),
            "offsets in the queries": go(o=d_q.ptr + 64), "hits in the queries": go(h=d_q.ptr + 64), "hits in the offsets": go(h=offs.ptr + 16),
            "offsets in the hits": go(o=hits.ptr + 16 * (cap - 1)),
            "queries end in the hits": go(qin=pkg.BuildInput(pkg.TRI_PADDED64, 30, hits.ptr + 16 * (cap - 1), None, None, 0, 0)),
            "hits over the query vertices": go(qin=indexed, h=d_v.ptr + 16), "offsets over the query indices": go(qin=indexed, o=d_i.ptr + 16),
            "hits over the nodes": go(h=b.result.d_nodes + nodes_bytes - 16), "offsets over the tree triangles": go(o=b.result.d_tris + 64),
            "self hits over the tree triangles": go(qin=none, flags=SELF, k=n, h=b.result.d_tris + 64),
            "hits over the leaves": go(h=b.result.d_leaves + 28 * 4) if b.result.layout == 1 else E_INVALID,
            "above capacity": go(res=variant(n_leaves=n + 1_000_000, root=0)),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        assert tot.value == 0x77
        c.synchronize()
        assert hits.download(pkg.TRI_HIT, cap).tobytes() == guard_h.tobytes() and offs.download(np.uint32, n + 1).tobytes() == guard_o.tobytes()
        # on a fresh ctx (capacity 0) a caller tree is refused until bvh_ctx_reserve
        c2 = pkg.Context(0)
        try:
            assert go(ctx=c2.handle) == E_INVALID
        finally:
            c2.close()
        assert hits.download(pkg.TRI_HIT, cap).tobytes() == guard_h.tobytes() and offs.download(np.uint32, n + 1).tobytes() == guard_o.tobytes()
        # a count-only call ignores the capacity's range; the same arguments without a fault go through, and so does the self mode
        assert go(h=None, cap_=1 << 40, radius=0.0) == 0 and tot.value != 0x77
        assert go(radius=0.0, cap_=cap) == 0
        assert go(qin=none, flags=S | SELF | SKIP, k=n, radius=0.0) == 0
        for x in (d_q, d_v, d_i, hits, offs):
            x.free()
    finally:
        c.close()
