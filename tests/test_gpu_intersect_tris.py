"""bvh_intersect_tris on the GPU: every query triangle's set of every builder and both node layouts against the numpy brute force (tests/test_intersect_tris.py:
stage-E box test, then the f64 predicate) — whole sets, 100 % of the queries, after sorting each slice —, the three triangle formats on either side, self mode,
symmetry, triangles within f32 rounding of touching, the rule cases as tiny meshes, the count / scan / fill passes and their capacity rule, the stackless pass on
a tree deeper than the short stack, queries after a refit and an optimise, non-finite coordinates, errors, and one larger size."""
import ctypes as C

import numpy as np
import pytest

from test_intersect_tris import (E_INVALID, RULE_CASES, TOTALS, as_triangles, box_pairs, crosses64, crosses_exact, near_degenerate, shifted, stage_e_boxes,
                                 tris_brute_force, tt_mesh, xyz)
from test_overlap import csr_of, leaf_boxes_of, sorted_slices
from test_gpu_overlap import check_answer, walk_stack_depth
from test_gpu_query import caterpillar, lbvh_result
from test_gpu_refit import jitter, no_negzero

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32
GUARD = 0xA5A5A5A5

_REF = {}


def reference(pkg, queries, tree, self_pairs=False):
    """(sets, (offsets, prims)) of mesh ``queries`` against mesh ``tree`` (names of tt_mesh), computed once"""
    key = (queries, tree, self_pairs)
    if key not in _REF:
        sets = tris_brute_force(tt_mesh(pkg, queries), tt_mesh(pkg, tree), self_pairs=self_pairs)
        _REF[key] = (sets, csr_of(sets))
    return _REF[key]


def packed_of(tris):
    return np.ascontiguousarray(xyz(tris).reshape(-1, 9))


def indexed_of(tris):
    """(vertices f32 (k, 3), indices u32 (3n,)) with shared vertices merged"""
    uniq, inv = np.unique(xyz(tris).reshape(-1, 3), axis=0, return_inverse=True)
    return np.ascontiguousarray(uniq.astype(F32)), np.ascontiguousarray(inv.reshape(-1).astype(np.uint32))


class DeviceMesh:
    """a mesh uploaded in one of the three formats: .inp is its bvh_build_input"""

    def __init__(self, pkg, ctx, tris, fmt=None):
        fmt = pkg.TRI_PADDED64 if fmt is None else fmt
        self.n = len(tris)
        if fmt == pkg.TRI_PADDED64:
            self.bufs = [ctx.upload(np.ascontiguousarray(tris))]
            self.inp = pkg.BuildInput(fmt, 30, self.bufs[0].ptr, None, None, 0, 0)
        elif fmt == pkg.TRI_PACKED36:
            self.bufs = [ctx.upload(packed_of(tris))]
            self.inp = pkg.BuildInput(fmt, 30, self.bufs[0].ptr, None, None, 0, 0)
        else:
            v, i = indexed_of(tris)
            self.bufs = [ctx.upload(v), ctx.upload(i)]
            self.inp = pkg.BuildInput(fmt, 30, None, self.bufs[0].ptr, self.bufs[1].ptr, len(v), 0)

    def free(self):
        for b in self.bufs:
            b.free()


def tris_call(pkg, ctx, result, queries, mode=0, tin=None, capacity=None, want_prims=True, want_total=True, guard=0):
    """one bvh_intersect_tris call on guard-filled device arrays: -> (rc, offsets, prims (capacity + guard + 1 words) or None, total or None).  queries: a host
    TRIANGLE array, a DeviceMesh, or None with an int n (self mode: pass mode=1 and queries=n).  capacity None: a count-only call first, then the exact capacity"""
    own = None
    if isinstance(queries, int):
        m, qin = queries, None
    elif isinstance(queries, DeviceMesh):
        m, qin = queries.n, queries.inp
    else:
        own = DeviceMesh(pkg, ctx, queries)
        m, qin = own.n, own.inp
    p_q = C.byref(qin) if qin is not None else None
    p_t = C.byref(tin) if tin is not None else None
    d_off = ctx.upload(np.full(m + 1 + 4, GUARD, dtype=np.uint32))
    total = C.c_uint64(0xDEAD)
    L = pkg.lib()
    try:
        if capacity is None:                                          # count first
            rc = L.bvh_intersect_tris(ctx.handle, C.byref(result), p_t, p_q, m, mode, d_off.ptr, None, 0, C.byref(total))
            assert rc == 0, rc
            capacity = total.value
        d_prims = ctx.upload(np.full(capacity + guard + 1, GUARD, dtype=np.uint32)) if want_prims else None
        try:
            rc = L.bvh_intersect_tris(ctx.handle, C.byref(result), p_t, p_q, m, mode, d_off.ptr, d_prims.ptr if d_prims else None, capacity,
                                      C.byref(total) if want_total else None)
            ctx.synchronize()
            off = d_off.download(np.uint32, m + 1 + 4)
            assert (off[m + 1:] == GUARD).all(), "d_offsets written past n_queries + 1 words"
            prims = d_prims.download(np.uint32, capacity + guard + 1) if d_prims else None
            return rc, off[: m + 1], prims, (total.value if want_total else None)
        finally:
            if d_prims:
                d_prims.free()
    finally:
        d_off.free()
        if own is not None:
            own.free()


def same(off, prims, ref_off, ref_prims):
    return off.tobytes() == ref_off.tobytes() and sorted_slices(off, prims).tobytes() == ref_prims.tobytes()


# ---- 1. every builder, both layouts -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("queries,tree", [("uniform_1000", "uniform_1000"), ("cornell382", "cornell382"), ("bunny_1280_shifted", "bunny_1280")])
def test_exact_on_every_query(pkg, ctx, queries, tree):
    q, t = tt_mesh(pkg, queries), tt_mesh(pkg, tree); n = len(t)
    sets, (ref_off, ref_prims) = reference(pkg, queries, tree)
    crossing, _ = TOTALS[(queries, None if queries == tree else tree)]
    assert int(ref_off[-1]) == (2 * crossing if queries == tree else crossing)      # a mesh against its own tree: every unordered pair from both sides
    print(f"{queries} against {tree}: {ref_off[-1]} pairs, longest slice {np.diff(ref_off.astype(np.int64)).max()}")
    dq = DeviceMesh(pkg, ctx, q)
    per_algo = {}
    try:
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, t)
            d = b.download()
            assert leaf_boxes_of(d["nodes"], d["leaves"], n, b.result.layout).tobytes() == stage_e_boxes(t).tobytes()
            keep = []
            results = [("as built", b.result)]
            if b.result.layout == 1:
                results.append(("lbvh layout", lbvh_result(pkg, ctx, b, keep)))
            for label, res in results:
                rc, off, prims, total = tris_call(pkg, ctx, res, dq, guard=16)
                assert rc == 0 and total == int(ref_off[-1])
                got = check_answer(off, prims, ref_off, ref_prims, f"{queries} algo {algo} {label}")
                per_algo.setdefault(algo, (off, got))
            o2, p2 = b.intersect_tris(q)                              # the Python binding: host arrays in, host arrays out
            assert same(o2, p2, ref_off, ref_prims)
            for k in keep:
                k.free()
    finally:
        dq.free()
    for algo in (1, 2, 3):
        assert per_algo[algo][0].tobytes() == per_algo[0][0].tobytes() and per_algo[algo][1].tobytes() == per_algo[0][1].tobytes(), f"builders {algo} and 0 differ"


def test_binding_forms_and_capacity_retry(pkg, ctx):
    q, t = tt_mesh(pkg, "bunny_1280_shifted"), tt_mesh(pkg, "bunny_1280")
    _, (ref_off, ref_prims) = reference(pkg, "bunny_1280_shifted", "bunny_1280")
    b = pkg.PLOCNew().build(ctx, t)
    dp, di = DeviceMesh(pkg, ctx, q, pkg.TRI_PACKED36), DeviceMesh(pkg, ctx, q, pkg.TRI_INDEXED)
    try:
        forms = (dict(other=q), dict(other=xyz(q)), dict(other=packed_of(q)), dict(other=dp.bufs[0], tri_format=pkg.TRI_PACKED36),
                 dict(other=dp.bufs[0].ptr, tri_format=pkg.TRI_PACKED36, n=len(q)), dict(other=q, capacity=1), dict(other=q, capacity=1 << 20),
                 dict(vertices=di.bufs[0], indices=di.bufs[1], n_vertices=di.inp.n_vertices, tri_format=pkg.TRI_INDEXED))
        for form in forms:
            off, prims = b.intersect_tris(**form)
            assert off.dtype == np.uint32 and prims.dtype == np.uint32 and len(prims) == ref_off[-1]
            assert same(off, prims, ref_off, ref_prims), list(form)
    finally:
        dp.free(); di.free()
    off, prims = b.intersect_tris(np.zeros(0, dtype=pkg.meshgen.TRIANGLE))
    assert off.tolist() == [0] and len(prims) == 0
    with pytest.raises(pkg.BvhError):
        b.intersect_tris()                                            # another mesh, or self_pairs
    with pytest.raises(pkg.BvhError):
        b.intersect_tris(q, self_pairs=True)
    with pytest.raises(pkg.BvhError):
        b.intersect_tris(np.zeros((3, 5), dtype=np.float32))


# ---- 2. formats -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_formats_on_either_side_give_identical_answers(pkg, ctx):
    t = tt_mesh(pkg, "cornell82"); n = len(t)
    _, (ref_off, ref_prims) = reference(pkg, "cornell82", "cornell82")
    _, (self_off, self_prims) = reference(pkg, "cornell82", "cornell82", True)
    assert ref_off[-1] == 2 * TOTALS[("cornell82", None)][0] and self_off[-1] == TOTALS[("cornell82", None)][0]
    fmts = (pkg.TRI_PADDED64, pkg.TRI_PACKED36, pkg.TRI_INDEXED)
    meshes = [DeviceMesh(pkg, ctx, t, f) for f in fmts]
    try:
        for algo in (1, 3):                                           # both layouts
            b = pkg.BUILDERS[algo]().build(ctx, t)
            for mt in meshes:
                for mq in meshes:
                    rc, off, prims, total = tris_call(pkg, ctx, b.result, mq, tin=mt.inp, guard=4)
                    assert rc == 0 and total == int(ref_off[-1])
                    check_answer(off, prims, ref_off, ref_prims, f"algo {algo} tree format {mt.inp.tri_format} query format {mq.inp.tri_format}")
                rc, off, prims, total = tris_call(pkg, ctx, b.result, n, mode=pkg.TRIS_SELF, tin=mt.inp, guard=4)
                assert rc == 0 and total == int(self_off[-1])
                check_answer(off, prims, self_off, self_prims, f"algo {algo} self, format {mt.inp.tri_format}")
            rc, off, prims, _ = tris_call(pkg, ctx, b.result, meshes[2], guard=4)         # tris NULL: the tree's own d_tris
            assert rc == 0 and same(off, prims[: ref_off[-1]], ref_off, ref_prims)
        # a tree built FROM indexed input answers the same
        mi = meshes[2]
        bi = pkg.PLOCNew().build_ex(ctx, n, vertices=mi.bufs[0], indices=mi.bufs[1], n_vertices=mi.inp.n_vertices, tri_format=pkg.TRI_INDEXED)
        off, prims = bi.intersect_tris(self_pairs=True, tree_vertices=mi.bufs[0], tree_indices=mi.bufs[1], tree_n_vertices=mi.inp.n_vertices,
                                       tree_tri_format=pkg.TRI_INDEXED)
        assert same(off, prims, self_off, self_prims)
    finally:
        for m in meshes:
            m.free()


# ---- 3. self mode ----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uniform_1000", "cornell382", "cornell82", "bunny_1280"])
def test_self_pairs(pkg, ctx, name):
    t = tt_mesh(pkg, name); n = len(t)
    _, (full_off, full_prims) = reference(pkg, name, name)
    _, (ref_off, ref_prims) = reference(pkg, name, name, True)
    assert int(ref_off[-1]) == TOTALS[(name, None)][0]
    owner = np.repeat(np.arange(n), np.diff(full_off.astype(np.int64)))
    assert (full_prims != owner).all()                                # no triangle crosses itself
    keep = full_prims > owner                                         # the query-mode answer filtered to j > i IS the self answer
    assert full_prims[keep].tobytes() == ref_prims.tobytes() and (np.bincount(owner[keep], minlength=n) == np.diff(ref_off.astype(np.int64))).all()
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, t)
        rc, off, prims, total = tris_call(pkg, ctx, b.result, n, mode=pkg.TRIS_SELF, guard=8)
        assert rc == 0 and total == int(ref_off[-1])
        check_answer(off, prims, ref_off, ref_prims, f"{name} algo {algo} self")
        own = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
        assert (prims[:total] > own).all()                            # j > i: every pair once, nothing with itself
        rc, off, prims, total = tris_call(pkg, ctx, b.result, t, guard=8)                   # the mesh against its own tree, on the device too
        assert rc == 0 and same(off, prims[:total], full_off, full_prims)
        o2, p2 = b.intersect_tris(self_pairs=True)
        assert same(o2, p2, ref_off, ref_prims)
        if name == "bunny_1280":                                      # a closed manifold: neighbours touch everywhere and cross nowhere
            bo, bp = b.overlap(self_pairs=True)
            assert total == 0 and len(p2) == 0 and len(bp) == TOTALS[(name, None)][1] > 0


# ---- 4. symmetry -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_against_tree_of_b_is_the_transpose_of_b_against_tree_of_a(pkg, ctx):
    a, b = tt_mesh(pkg, "bunny_1280_shifted"), tt_mesh(pkg, "bunny_1280")
    for algo in (0, 2):
        off_ab, prims_ab = pkg.BUILDERS[3 - algo]().build(ctx, b).intersect_tris(a)       # (i in a, j in b)
        off_ba, prims_ba = pkg.BUILDERS[algo]().build(ctx, a).intersect_tris(b)           # (j in b, i in a); the ctx's arena now holds this tree instead
        ab = set(zip(np.repeat(np.arange(len(a)), np.diff(off_ab.astype(np.int64))).tolist(), prims_ab.tolist()))
        ba = set(zip(prims_ba.tolist(), np.repeat(np.arange(len(b)), np.diff(off_ba.astype(np.int64))).tolist()))
        assert len(ab) == len(prims_ab) == TOTALS[("bunny_1280_shifted", "bunny_1280")][0] and ab == ba


# ---- 5. within f32 rounding of touching ----------------------------------------------------------------------------------------------------------------------------------

_NEAR = {}


def near_sets(pkg):
    if not _NEAR:
        b, a_vertex, a_edge = near_degenerate()
        for label, a in (("vertex", a_vertex), ("edge", a_edge)):
            sets = tris_brute_force(a, b)
            _NEAR[label] = (as_triangles(pkg, a), sets, csr_of(sets), crosses_exact(a, b))
        _NEAR["b"] = no_negzero(as_triangles(pkg, b))
    return _NEAR


@pytest.mark.parametrize("label", ["vertex", "edge"])
def test_near_degenerate_pairs_equal_exact_arithmetic(pkg, ctx, label):
    near = near_sets(pkg)
    b = near["b"]
    a, sets, (ref_off, ref_prims), exact = near[label]
    assert 0.2 < exact.mean() < 0.8
    for algo in (1, 3):
        bl = pkg.BUILDERS[algo]().build(ctx, b)
        rc, off, prims, total = tris_call(pkg, ctx, bl.result, a, guard=8)
        assert rc == 0 and total == int(ref_off[-1])
        got = check_answer(off, prims, ref_off, ref_prims, f"near-degenerate {label} algo {algo}")
        diagonal = np.array([i in got[off[i]:off[i + 1]] for i in range(len(a))])
        assert (diagonal == exact).all(), f"{np.count_nonzero(diagonal != exact)} of {len(a)} partners differ from exact arithmetic"


# ---- 6. the rules, as tiny meshes ------------------------------------------------------------------------------------------------------------------------------------------

def test_rule_cases_as_meshes(pkg, ctx):
    """tree triangle k = the X of case k moved to a place of its own (cases 50 apart along x, so nothing of one case's box reaches another's), query triangle k
    = its Y moved the same way; both orders"""
    shift = np.array([[50.0 * k, 0.0, 0.0] for k in range(len(RULE_CASES))], dtype=F32)[:, None, :]
    xs = (np.array([c[1] for c in RULE_CASES], dtype=F32) + shift).astype(F32)
    ys = (np.array([c[2] for c in RULE_CASES], dtype=F32) + shift).astype(F32)
    expected = np.array([c[3] for c in RULE_CASES])
    assert (crosses64(xs, ys) == expected).all() and (crosses_exact(xs, ys) == expected).all()       # the move (integers, exact in f32) changes no answer
    for tree_v, query_v in ((xs, ys), (ys, xs)):
        tree, queries = as_triangles(pkg, tree_v), as_triangles(pkg, query_v)
        ref_off, ref_prims = csr_of(tris_brute_force(queries, tree))
        assert ref_prims.tolist() == np.nonzero(expected)[0].tolist()                                # exactly the diagonal of the crossing cases
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, tree)
            rc, off, prims, total = tris_call(pkg, ctx, b.result, queries, guard=4)
            assert rc == 0 and total == int(expected.sum())
            check_answer(off, prims, ref_off, ref_prims, f"rule cases algo {algo}")
    # as ONE mesh: self mode reports nothing but the crossing cases' pairs (k, n + k)
    both = as_triangles(pkg, np.concatenate([xs, ys]))
    ref_off, ref_prims = csr_of(tris_brute_force(both, both, self_pairs=True))
    assert ref_prims.tolist() == (np.nonzero(expected)[0] + len(xs)).tolist()
    b = pkg.HPLOC().build(ctx, both)
    off, prims = b.intersect_tris(self_pairs=True)
    assert same(off, prims, ref_off, ref_prims)


# ---- 7. count only, too small a capacity, exact capacity, determinism ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [1, 3])
def test_passes_and_capacity(pkg, ctx, algo):
    q, t = tt_mesh(pkg, "uniform_1000"), tt_mesh(pkg, "uniform_1000")
    _, (ref_off, ref_prims) = reference(pkg, "uniform_1000", "uniform_1000")
    total = int(ref_off[-1])
    b = pkg.BUILDERS[algo]().build(ctx, t)
    rc, off, prims, tt = tris_call(pkg, ctx, b.result, q, capacity=0, want_prims=False)               # d_prims NULL: offsets and the total
    assert rc == 0 and tt == total and prims is None and off.tobytes() == ref_off.tobytes()
    rc, off, prims, tt = tris_call(pkg, ctx, b.result, q, capacity=total - 1, guard=8)                 # one word short: d_prims untouched, the total reported
    assert rc == 0 and tt == total and off.tobytes() == ref_off.tobytes() and (prims == GUARD).all()
    rc, off, prims, tt = tris_call(pkg, ctx, b.result, q, capacity=total, guard=8)                     # exactly enough
    assert rc == 0 and tt == total
    filled = check_answer(off, prims, ref_off, ref_prims, "exact capacity")
    rc, off2, prims2, t2 = tris_call(pkg, ctx, b.result, q, capacity=total, guard=8, want_total=False)  # no read-back: the same bytes after a synchronise
    assert rc == 0 and t2 is None and off2.tobytes() == off.tobytes() and prims2.tobytes() == prims.tobytes()
    rc, off3, prims3, _ = tris_call(pkg, ctx, b.result, q, capacity=total - 1, guard=8, want_total=False)
    assert rc == 0 and off3.tobytes() == off.tobytes() and (prims3 == GUARD).all()
    rc, off4, prims4, t4 = tris_call(pkg, ctx, b.result, q, capacity=4 * total + 100, guard=8)          # generous: nothing past the total
    assert rc == 0 and t4 == total and prims4[:total].tobytes() == prims[:total].tobytes() and (prims4[total:] == GUARD).all()
    assert filled.tobytes() == ref_prims.tobytes()


# ---- 8. a tree deeper than the short stack -----------------------------------------------------------------------------------------------------------------------------------

def caterpillar_triangles(pkg, H):
    """queries for caterpillar(H), whose triangles are parallel to z = 0 over (-10, -10) .. (30, 30): slivers that run up through all of them, through the far
    ones only, through a few, beside them all, and flat ones between two levels"""
    rng = np.random.default_rng(H)
    q = [[(0.0, 0.0, -5.0), (1.0, 0.5, 1000.0 + 2 * H), (0.5, 1.0, 1000.0 + 2 * H)]]              # through every triangle
    for _ in range(40):                                                                             # through some of the far ones
        z0 = 1000.0 + rng.uniform(0, 2 * H - 1); z1 = z0 + rng.uniform(0.5, 40.0); x, y = rng.uniform(-5, 5, 2)
        q.append([(x, y, z0), (x + 1.0, y, z1), (x, y + 1.0, z1)])
    q.append([(2.0, 2.0, 999.5), (3.0, 2.0, 1000.0 + 2 * H), (2.0, 3.0, 1000.0 + 2 * H)])          # every far triangle, neither near one
    for _ in range(20):
        q.append([(40.0, 40.0, 0.0), (41.0, 40.0, 3000.0), (40.0, 41.0, 3000.0)])                  # tall, beside everything
        q.append([(0.0, 0.0, 700.0), (5.0, 0.0, 700.25), (0.0, 5.0, 700.5)])                       # between the near pair and the far ones
    q.append([(1.0, 1.0, -0.25), (2.0, 1.0, 0.25), (1.0, 2.0, 0.25)])                              # the near triangle at z = 0 alone
    return no_negzero(as_triangles(pkg, np.array(q, dtype=F32)))


@pytest.mark.parametrize("H,deep", [(300, True), (20, False)])
def test_deep_tree_takes_the_stackless_pass(pkg, H, deep):
    """That the stackless pass did the work at H = 300 is shown by the host-side walk_stack_depth > 64 (the short stack cannot hold those queries) together with
    the whole-set comparison, as in test_gpu_overlap.  The name check below shows less: k_tris_deep is launched after every pass and returns at once while the
    overflow word is 0, so its name is in kernel_times at H = 20 too — it only pins the names bvh_ctx_kernel_times reports."""
    tris, nodes, root, n = caterpillar(pkg, H, 11 + H)
    queries = caterpillar_triangles(pkg, H)
    qb = stage_e_boxes(queries)
    depth = max(walk_stack_depth(nodes, root, n - 1, np.concatenate([qb["min"][j], qb["max"][j]])) for j in (0, 41))
    assert (depth > 64) == deep, depth
    ref_off, ref_prims = csr_of(tris_brute_force(queries, tris))
    assert ref_off[1] == n and ref_off[-1] > 2 * n and (np.diff(ref_off.astype(np.int64)) == 0).sum() >= 40
    c = pkg.Context(0)
    try:
        c.reserve(n)
        d_nodes, d_tris = c.upload(nodes), DeviceMesh(pkg, c, tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        c.set_profiling(2)
        rc, off, prims, total = tris_call(pkg, c, r, queries, tin=d_tris.inp, guard=8)
        kt = c.kernel_times()
        c.set_profiling(0)
        assert {"k_tris_count", "k_tris_deep", "k_overlap_scan", "k_tris_fill", "k_refit_plan"} <= set(kt), kt
        assert rc == 0 and total == int(ref_off[-1])
        check_answer(off, prims, ref_off, ref_prims, f"caterpillar {H}")
        d_nodes.free(); d_tris.free()
    finally:
        c.close()


# ---- 9. after refit and optimise -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_after_refit_and_optimize(pkg, algo):
    a = tt_mesh(pkg, "uniform_1000"); moved = jitter(a, 23, 2e-2)
    q = tt_mesh(pkg, "uniform_1000_shifted")
    ref_off, ref_prims = csr_of(tris_brute_force(q, moved))
    self_off, self_prims = csr_of(tris_brute_force(moved, moved, self_pairs=True))
    assert ref_off[-1] > 0 and self_off[-1] > 0
    assert ref_off.tobytes() != csr_of(tris_brute_force(q, a))[0].tobytes()       # the answer on the unmoved triangles is another one
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        b.intersect_tris(q)                                           # (the plan of the ctx's own tree is made here and kept)
        b.refit(moved)
        for state in ("refit", "optimize"):
            off, prims = b.intersect_tris(q)
            assert same(off, prims, ref_off, ref_prims), f"{state} algo {algo}"
            off, prims = b.intersect_tris(self_pairs=True)
            assert same(off, prims, self_off, self_prims), f"{state} algo {algo} self"
            b.optimize(3)
    finally:
        c.close()


def test_split_tree_answers_query_mode_and_refuses_self(pkg, ctx):
    """a build_split tree has more leaves (references) than triangles: query mode reports a pair once per reference reached and, deduplicated, equals the
    unsplit answer; self mode would read triangle i for every i < n_leaves and is refused by the binding before any call"""
    from test_split import largest_root_area
    t = tt_mesh(pkg, "cornell382"); q = tt_mesh(pkg, "cornell382_shifted")
    ref = tris_brute_force(q, t)
    assert sum(len(s) for s in ref) > 0
    for algo in (1, 3):
        b = pkg.BUILDERS[algo]().build_split(ctx, t, float(largest_root_area(t)) / 64.0)
        assert b.result.n_leaves > len(t)
        off, prims = b.intersect_tris(q)
        assert len(off) == len(q) + 1 and (prims < len(t)).all()
        got = [np.unique(prims[off[i]:off[i + 1]]) for i in range(len(q))]
        bad = [i for i in range(len(q)) if got[i].tobytes() != ref[i].tobytes()]
        assert not bad, f"algo {algo}: {len(bad)} slices differ (first {bad[:6]})"
        with pytest.raises(pkg.BvhError, match="build_split"):
            b.intersect_tris(self_pairs=True)


# ---- 10. non-finite coordinates ----------------------------------------------------------------------------------------------------------------------------------------------------

def spoiled(tris, seed):
    """a copy with 24 triangles spoiled: a NaN, +inf or -inf in one coordinate, in a whole vertex, or in one axis of all three vertices"""
    t = tris.copy()
    rng = np.random.default_rng(seed)
    idx = rng.choice(len(t), 24, replace=False)
    for k, i in enumerate(idx):
        val = (np.nan, np.inf, -np.inf)[k % 3]
        f = ("v1", "v2", "v3")[(k // 3) % 3]
        v = t[f][i].copy()
        if k % 4 == 0:
            v[:] = val
        else:
            v[k % 3] = val
        t[f][i] = v
        if k % 8 == 1:
            for g in ("v1", "v2", "v3"):
                w = t[g][i].copy(); w[1] = val; t[g][i] = w
    return t, np.sort(idx)


def test_non_finite_coordinates_in_either_mesh(pkg, ctx):
    tree, bad_t = spoiled(tt_mesh(pkg, "uniform_1000"), 5)
    queries, bad_q = spoiled(shifted(pkg, tt_mesh(pkg, "uniform_1000")), 6)
    nan_t = np.isnan(xyz(tree)).any(axis=(1, 2)); nan_q = np.isnan(xyz(queries)).any(axis=(1, 2))
    assert nan_t.sum() >= 8 and nan_q.sum() >= 8
    sets = tris_brute_force(queries, tree)                            # (stage_e_boxes restates the clamps against the reset box)
    ref_off, ref_prims = csr_of(sets)
    assert ref_off[-1] > 100
    owner = np.repeat(np.arange(len(queries)), np.diff(ref_off.astype(np.int64)))
    assert not nan_q[owner].any() and not nan_t[ref_prims].any()      # no NaN triangle in any pair
    self_off, self_prims = csr_of(tris_brute_force(tree, tree, self_pairs=True))
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tree)
        d = b.download()
        assert leaf_boxes_of(d["nodes"], d["leaves"], len(tree), b.result.layout).tobytes() == stage_e_boxes(tree).tobytes()
        rc, off, prims, total = tris_call(pkg, ctx, b.result, queries, guard=8)
        assert rc == 0 and total == int(ref_off[-1])
        got = check_answer(off, prims, ref_off, ref_prims, f"non-finite algo {algo}")
        own = np.repeat(np.arange(len(queries)), np.diff(off.astype(np.int64)))
        assert not nan_q[own].any() and not nan_t[got].any()
        rc, off, prims, total = tris_call(pkg, ctx, b.result, len(tree), mode=pkg.TRIS_SELF, guard=8)
        assert rc == 0 and total == int(self_off[-1])
        check_answer(off, prims, self_off, self_prims, f"non-finite algo {algo} self")


# ---- 11. errors write nothing ---------------------------------------------------------------------------------------------------------------------------------------------------------

def test_errors_write_nothing(pkg):
    tris = tt_mesh(pkg, "uniform_1000"); n = len(tris)
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        m = 256
        dq = DeviceMesh(pkg, c, tris[:m]); di = DeviceMesh(pkg, c, tris[:m], pkg.TRI_INDEXED); dt = DeviceMesh(pkg, c, tris, pkg.TRI_PACKED36)
        guard_off = np.full(n + 1, GUARD, dtype=np.uint32); guard_prims = np.full(4096, GUARD, dtype=np.uint32)
        d_off, d_prims = c.upload(guard_off), c.upload(guard_prims)
        total = C.c_uint64(1234567)
        L = pkg.lib()
        DEFAULT = object()

        def call(res=b.result, tin=None, q=DEFAULT, k=m, mode=0, off=d_off.ptr, prims=d_prims.ptr, cap=4096, ctx=c.handle):
            q = dq.inp if q is DEFAULT else q
            return L.bvh_intersect_tris(ctx, C.byref(res) if res is not None else None, C.byref(tin) if tin is not None else None,
                                        C.byref(q) if q is not None else None, k, mode, off, prims, cap, C.byref(total))

        def variant(**kw):
            r = pkg.Result.from_buffer_copy(b.result)
            for key, v in kw.items():
                setattr(r, key, v)
            return r

        def inp(fmt, tris_ptr=None, verts=None, idx=None, nv=0):
            return pkg.BuildInput(fmt, 30, tris_ptr, verts, idx, nv, 0)
        nodes_bytes = (n - 1) * 32
        cases = {
            "null ctx": call(ctx=None), "null tree": call(res=None), "null offsets": call(off=None),
            "null queries without self": call(q=None), "queries with self": call(k=n, mode=1), "self with n_queries != n_leaves": call(q=None, mode=1),
            "n_leaves 1": call(res=variant(n_leaves=1)), "layout 2": call(res=variant(layout=2)), "null nodes": call(res=variant(d_nodes=None)),
            "layout 1 without leaves": call(res=variant(d_leaves=None)), "root not internal": call(res=variant(root=n - 1)),
            "no triangles": call(res=variant(d_tris=None)), "mode 2": call(mode=2), "mode -1": call(mode=-1),
            "n_queries 2^30": call(k=1 << 30), "n_queries 2^32 - 1": call(k=0xFFFFFFFF),
            "above capacity": call(res=variant(n_leaves=n + 1_000_000, root=0)),
            "query format 3": call(q=inp(3, dq.bufs[0].ptr)), "query padded without tris": call(q=inp(pkg.TRI_PADDED64)),
            "query packed misaligned": call(q=inp(pkg.TRI_PACKED36, dq.bufs[0].ptr + 4)),
            "query indexed without vertices": call(q=inp(pkg.TRI_INDEXED, None, None, di.bufs[1].ptr, di.inp.n_vertices)),
            "query indexed without indices": call(q=inp(pkg.TRI_INDEXED, None, di.bufs[0].ptr, None, di.inp.n_vertices)),
            "query indexed without a vertex count": call(q=inp(pkg.TRI_INDEXED, None, di.bufs[0].ptr, di.bufs[1].ptr, 0)),
            "tree format 7": call(tin=inp(7, dt.bufs[0].ptr)), "tree indexed without indices": call(tin=inp(pkg.TRI_INDEXED, None, di.bufs[0].ptr, None, 9)),
            "offsets in queries": call(off=dq.bufs[0].ptr + 64), "prims in queries": call(prims=dq.bufs[0].ptr + 64 * (m - 1) + 60),
            "offsets in query vertices": call(q=di.inp, off=di.bufs[0].ptr), "prims in query indices": call(q=di.inp, prims=di.bufs[1].ptr + 12 * m - 4),
            "offsets in nodes": call(off=b.result.d_nodes + nodes_bytes - 4), "prims in nodes": call(prims=b.result.d_nodes),
            "prims in leaves": call(prims=b.result.d_leaves + 28 * n - 4), "offsets in tree tris": call(off=b.result.d_tris + 64 * n - 4),
            "prims in given tree tris": call(tin=dt.inp, prims=dt.bufs[0].ptr + 36 * n - 4),
            "prims in offsets": call(prims=d_off.ptr + 4 * m), "offsets in prims": call(off=d_prims.ptr + 4 * 4095),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        c.synchronize()
        assert total.value == 1234567
        assert d_off.download(np.uint32, n + 1).tobytes() == guard_off.tobytes() and d_prims.download(np.uint32, 4096).tobytes() == guard_prims.tobytes()
        assert dq.bufs[0].download(pkg.meshgen.TRIANGLE, m).tobytes() == tris[:m].tobytes()
        # arrays that end where an input begins are fine, a NULL d_prims is not an error and its capacity names no range
        assert call(prims=None, cap=1 << 40) == 0
        d_off.upload(guard_off)
        # n_queries == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        assert call(k=0) == 0
        c.synchronize()
        off = d_off.download(np.uint32, n + 1)
        assert total.value == 0 and off[0] == 0 and (off[1:] == GUARD).all() and d_prims.download(np.uint32, 4096).tobytes() == guard_prims.tobytes()
        # on a fresh ctx (capacity 0) a caller tree is refused until bvh_ctx_reserve
        d_off.upload(guard_off)
        c2 = pkg.Context(0)
        try:
            assert L.bvh_intersect_tris(c2.handle, C.byref(b.result), None, C.byref(dq.inp), m, 0, d_off.ptr, d_prims.ptr, 4096, None) == E_INVALID
        finally:
            c2.close()
        c.synchronize()
        assert d_off.download(np.uint32, n + 1).tobytes() == guard_off.tobytes()
        for x in (dq, di, dt, d_off, d_prims):
            x.free()
    finally:
        c.close()


# ---- 12. size --------------------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_twenty_thousand_triangles_against_their_shifted_copy(pkg, ctx):
    t = no_negzero(pkg.meshgen.bunny_like(20_480, 2))
    q = shifted(pkg, t)
    ref_off, ref_prims = csr_of(tris_brute_force(q, t))               # chunked: a few hundred queries against all boxes at a time
    qi, _ = box_pairs(q, t)
    print(f"bunny 20 480 against its shift: {ref_off[-1]} crossing pairs of {len(qi)} box pairs, longest slice {np.diff(ref_off.astype(np.int64)).max()}")
    assert ref_off[-1] > 1000
    b = pkg.HPLOC().build(ctx, t)
    rc, off, prims, total = tris_call(pkg, ctx, b.result, q, guard=16)
    assert rc == 0 and total == int(ref_off[-1])
    check_answer(off, prims, ref_off, ref_prims, "bunny 20 480")
