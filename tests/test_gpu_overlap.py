"""bvh_overlap on the GPU: every query's set of every builder and both node layouts against the numpy brute force (tests/test_overlap.py) — exact, 100 % of
the queries —, self-collision pairs, the count / scan / fill passes and their capacity rule, determinism, the stackless pass on trees deeper than the short
stack, queries after a refit, an optimise and a rebuild, bvh_build_boxes and top-level scene trees, errors, and one large size."""
import ctypes as C

import numpy as np
import pytest

from test_overlap import AABB, E_INVALID, as_boxes, csr_of, make_boxes, overlap_brute_force, overlap_pairs, sorted_slices, leaf_boxes_of
from test_gpu_point_query import MESHES
from test_gpu_query import caterpillar, lbvh_result, mesh
from test_gpu_refit import jitter, no_negzero

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32
GUARD = 0xA5A5A5A5
SELF_PAIRS = {"uniform_1000": 3195, "sponza_1000": 81, "cornell382": 2222, "uniform_3": 3}      # unordered overlapping pairs, computed on the CPU


def tri_boxes(tris):
    """the primitives' boxes as stage E makes them (f32 min / max of the three vertices)"""
    lo = np.minimum(np.minimum(tris["v1"], tris["v2"]), tris["v3"]); hi = np.maximum(np.maximum(tris["v1"], tris["v2"]), tris["v3"])
    return as_boxes(np.concatenate([lo, hi], axis=1))


def vertices(tris):
    return np.concatenate([tris["v1"], tris["v2"], tris["v3"]])


_REF = {}


def reference(pkg, name):
    """(boxes, kind, brute-force sets, (offsets, prims)) per mesh, computed once"""
    if name not in _REF:
        tris = mesh(pkg, name)
        leaf = tri_boxes(tris)
        boxes, kind = make_boxes(leaf, 31 + len(tris), points=vertices(tris))
        sets = overlap_brute_force(boxes, leaf)
        _REF[name] = (boxes, kind, sets, csr_of(sets))
    return _REF[name]


def overlap(pkg, ctx, result, boxes, mode=0, capacity=None, want_prims=True, want_total=True, guard=0):
    """one bvh_overlap call on guard-filled device arrays: -> (rc, offsets, prims (capacity + guard + 1 words) or None, total or None).  boxes: a host AABB
    array or (device address, count).  capacity None: a count-only call first, then the exact capacity"""
    own = None
    if isinstance(boxes, tuple):
        d_boxes, m = boxes
    else:
        m = len(boxes)
        own = ctx.upload(boxes); d_boxes = own.ptr
    d_off = ctx.upload(np.full(m + 1 + 4, GUARD, dtype=np.uint32))
    total = C.c_uint64(0xDEAD)
    try:
        if capacity is None:                                          # count first
            rc = pkg.lib().bvh_overlap(ctx.handle, C.byref(result), d_boxes, m, mode, d_off.ptr, None, 0, C.byref(total))
            assert rc == 0, rc
            capacity = total.value
        d_prims = ctx.upload(np.full(capacity + guard + 1, GUARD, dtype=np.uint32)) if want_prims else None
        try:
            rc = pkg.lib().bvh_overlap(ctx.handle, C.byref(result), d_boxes, m, mode, d_off.ptr, d_prims.ptr if d_prims else None, capacity,
                                       C.byref(total) if want_total else None)
            ctx.synchronize()
            off = d_off.download(np.uint32, m + 1 + 4)
            assert (off[m + 1:] == GUARD).all(), "d_offsets written past n_boxes + 1 words"
            prims = d_prims.download(np.uint32, capacity + guard + 1) if d_prims else None
            return rc, off[: m + 1], prims, (total.value if want_total else None)
        finally:
            if d_prims:
                d_prims.free()
    finally:
        d_off.free()
        if own is not None:
            own.free()


def check_answer(off, prims, ref_off, ref_prims, what):
    assert off.tobytes() == ref_off.tobytes(), f"{what}: offsets differ on {np.count_nonzero(off != ref_off)} words (first {np.nonzero(off != ref_off)[0][:6]})"
    total = int(ref_off[-1])
    got = sorted_slices(off, prims[:total])
    if got.tobytes() != ref_prims.tobytes():
        bad = [i for i in range(len(off) - 1) if got[off[i]:off[i + 1]].tobytes() != ref_prims[off[i]:off[i + 1]].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(off) - 1} slices differ (first {bad[:6]})")
    # (sorted slices equal to strictly increasing reference slices: no duplicates)
    assert (prims[total:] == GUARD).all(), f"{what}: d_prims written past the total"
    return got


# ---- 1. exact on every query ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MESHES)
def test_exact_on_every_query(pkg, ctx, name):
    tris = mesh(pkg, name); n = len(tris)
    boxes, kind, sets, (ref_off, ref_prims) = reference(pkg, name)
    counts = np.diff(ref_off.astype(np.int64))
    print(f"{name}: mean results per query {[round(float(counts[:1536][kind[:1536] == k].mean()), 2) for k in (0, 1, 2)]} (2 % / 10 % / 50 %), total {ref_off[-1]}")
    if n >= 3:
        assert (counts[:1536] == 0).any() and (counts[:1536] > 0).any()
    assert all((np.diff(s.astype(np.int64)) > 0).all() for s in sets)
    per_algo = {}
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        d = b.download()
        assert leaf_boxes_of(d["nodes"], d["leaves"], n, b.result.layout).tobytes() == tri_boxes(tris).tobytes()
        keep = []
        results = [("as built", b.result)]
        if b.result.layout == 1:
            results.append(("lbvh layout", lbvh_result(pkg, ctx, b, keep)))
        for label, res in results:
            rc, off, prims, total = overlap(pkg, ctx, res, boxes, guard=16)
            assert rc == 0 and total == int(ref_off[-1])
            got = check_answer(off, prims, ref_off, ref_prims, f"{name} algo {algo} {label}")
            per_algo.setdefault(algo, (off, got))
        o2, p2 = b.overlap(boxes)                                    # the Python binding: host arrays in, host arrays out
        assert o2.tobytes() == ref_off.tobytes() and sorted_slices(o2, p2).tobytes() == ref_prims.tobytes()
        for k in keep:
            k.free()
    for algo in (1, 2, 3):
        assert per_algo[algo][0].tobytes() == per_algo[0][0].tobytes() and per_algo[algo][1].tobytes() == per_algo[0][1].tobytes(), f"{name}: builders {algo} and 0 differ"


def test_binding_forms_and_capacity_retry(pkg, ctx):
    tris = mesh(pkg, "sponza_1000")
    boxes, _, _, (ref_off, ref_prims) = reference(pkg, "sponza_1000")
    b = pkg.PLOCNew().build(ctx, tris)
    flat = np.concatenate([boxes["min"], boxes["max"]], axis=1)
    d = ctx.upload(boxes)
    try:
        for form in (dict(boxes=boxes), dict(boxes=flat), dict(boxes=d), dict(boxes=d.ptr, n=len(boxes)), dict(boxes=boxes, capacity=1), dict(boxes=boxes, capacity=1 << 20)):
            off, prims = b.overlap(**form)
            assert off.dtype == np.uint32 and prims.dtype == np.uint32 and len(prims) == ref_off[-1]
            assert off.tobytes() == ref_off.tobytes() and sorted_slices(off, prims).tobytes() == ref_prims.tobytes()
    finally:
        d.free()
    off, prims = b.overlap(np.zeros(0, dtype=pkg.AABB))
    assert off.tolist() == [0] and len(prims) == 0
    with pytest.raises(pkg.BvhError):
        b.overlap()                                                   # boxes default only with self_pairs
    with pytest.raises(pkg.BvhError):
        b.overlap(np.zeros((3, 5), dtype=np.float32))


# ---- 2. self mode -------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MESHES)
def test_self_pairs(pkg, ctx, name):
    tris = mesh(pkg, name); n = len(tris)
    leaf = tri_boxes(tris)
    sets = overlap_brute_force(leaf, leaf, self_pairs=True)
    ref_off, ref_prims = csr_of(sets)
    print(f"{name}: {ref_off[-1]} overlapping pairs")
    if name in SELF_PAIRS:
        assert int(ref_off[-1]) == SELF_PAIRS[name]
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        rc, off, prims, total = overlap(pkg, ctx, b.result, (b.result.d_prim_aabbs, n), mode=pkg.OVERLAP_SELF, guard=8)
        assert rc == 0 and total == int(ref_off[-1])
        check_answer(off, prims, ref_off, ref_prims, f"{name} algo {algo} self")
        owner = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
        assert (prims[:total] > owner).all()                          # j > i: every pair once, nothing with itself
        o2, p2 = b.overlap(self_pairs=True)
        assert o2.tobytes() == ref_off.tobytes() and sorted_slices(o2, p2).tobytes() == ref_prims.tobytes()
        # n_boxes != n_leaves is an error
        d_off = ctx.upload(np.full(n + 2, GUARD, dtype=np.uint32))
        try:
            for m in (n - 1, n + 1):
                assert pkg.lib().bvh_overlap(ctx.handle, C.byref(b.result), b.result.d_prim_aabbs, m, pkg.OVERLAP_SELF, d_off.ptr, None, 0, None) == E_INVALID
            ctx.synchronize()
            assert (d_off.download(np.uint32, n + 2) == GUARD).all()
        finally:
            d_off.free()


# ---- 3. count only, too small a capacity, exact capacity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [1, 3])
def test_passes_and_capacity(pkg, ctx, algo):
    tris = mesh(pkg, "uniform_1000")
    boxes, _, _, (ref_off, ref_prims) = reference(pkg, "uniform_1000")
    total = int(ref_off[-1])
    b = pkg.BUILDERS[algo]().build(ctx, tris)
    rc, off, prims, t = overlap(pkg, ctx, b.result, boxes, capacity=0, want_prims=False)              # d_prims NULL: offsets and the total
    assert rc == 0 and t == total and prims is None and off.tobytes() == ref_off.tobytes()
    rc, off, prims, t = overlap(pkg, ctx, b.result, boxes, capacity=total - 1, guard=8)                # one word short: d_prims untouched, the total reported
    assert rc == 0 and t == total and off.tobytes() == ref_off.tobytes() and (prims == GUARD).all()
    rc, off, prims, t = overlap(pkg, ctx, b.result, boxes, capacity=total, guard=8)                    # exactly enough
    assert rc == 0 and t == total
    filled = check_answer(off, prims, ref_off, ref_prims, "exact capacity")
    raw = prims[:total].copy()
    rc, off2, prims2, t2 = overlap(pkg, ctx, b.result, boxes, capacity=total, guard=8, want_total=False)   # no read-back: the same bytes after a synchronise
    assert rc == 0 and t2 is None and off2.tobytes() == off.tobytes() and prims2.tobytes() == prims.tobytes()
    rc, off3, prims3, _ = overlap(pkg, ctx, b.result, boxes, capacity=total - 1, guard=8, want_total=False)
    assert rc == 0 and off3.tobytes() == off.tobytes() and (prims3 == GUARD).all()
    assert filled.tobytes() == ref_prims.tobytes() and raw.tobytes() == prims2[:total].tobytes()


# ---- 4. determinism --------------------------------------------------------------------------------------------------------------------------------------------

def test_two_calls_give_the_same_bytes(pkg, ctx):
    tris = mesh(pkg, "sponza_20000")
    boxes, _, _, (ref_off, _) = reference(pkg, "sponza_20000")
    for algo in (0, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        a1 = overlap(pkg, ctx, b.result, boxes)
        a2 = overlap(pkg, ctx, b.result, boxes)
        assert a1[1].tobytes() == a2[1].tobytes() == ref_off.tobytes() and a1[2].tobytes() == a2[2].tobytes()


# ---- 5. deep trees -------------------------------------------------------------------------------------------------------------------------------------------------

def walk_stack_depth(nodes, root, ni, q):
    """the deepest short stack of the kernel's walk ("enter left, push right" when both children are internal and overlap) for query box q"""
    qlo, qhi = np.asarray(q[:3], dtype=F32), np.asarray(q[3:], dtype=F32)

    def hit(c):
        return bool((qlo <= nodes["max"][c]).all() and (nodes["min"][c] <= qhi).all())
    stack, deepest, v = [], 0, root
    while True:
        l, r = int(nodes["left"][v]), int(nodes["right"][v])
        inner = [c for c in (l, r) if c < ni and hit(c)]
        if len(inner) == 2:
            stack.append(r); deepest = max(deepest, len(stack)); v = l
        elif inner:
            v = inner[0]
        elif stack:
            v = stack.pop()
        else:
            return deepest


def caterpillar_queries(H):
    rng = np.random.default_rng(H)
    q = [(-100.0, -100.0, -100.0, 100.0, 100.0, 5000.0)]                                           # covers everything
    for _ in range(120):                                                                            # the far side nodes only (some of them)
        a = rng.uniform(0, 2 * H - 1); w = rng.uniform(0, 40)
        q.append((-1.0, -1.0, 1000.0 + a, 1.0, 1.0, 1000.0 + a + w))
    q.append((-1.0, -1.0, 999.5, 1.0, 1.0, 1000.0 + 2 * H))                                        # every far triangle, neither near one
    for _ in range(40):                                                                             # nothing: below, beside, between
        q.append((-1.0, -1.0, -9.0 - rng.uniform(0, 5), 1.0, 1.0, -8.0))
        q.append((40.0, 40.0, 0.0, 50.0, 50.0, 5000.0))
        q.append((-1.0, -1.0, 0.625, 1.0, 1.0, 999.0))
    q.append((-1.0, -1.0, 0.0, 1.0, 1.0, 0.25))                                                    # the near triangle at z = 0 alone
    return as_boxes(np.array(q, dtype=F32))


@pytest.mark.parametrize("H,deep", [(300, True), (20, False)])
def test_deep_tree_takes_the_stackless_pass(pkg, H, deep):
    """caterpillar(H): chain node c_i has the children c_{i+1} and a side node s_i (both internal), shuffled left / right.  The walk enters the left child and
    pushes the right one whenever both overlap: for a box that covers everything the stack grows by one at every level whose LEFT child is the chain (about
    half of them: the side node, when entered first, is finished and popped before the chain goes on).  H = 300 therefore needs about 150 entries, far above
    the 64 of the short stack, and the stackless pass must serve those queries in the count AND in the fill pass; H = 20 is the control that stays in the
    short stack on the same code path."""
    tris, nodes, root, n = caterpillar(pkg, H, 11 + H)
    boxes = caterpillar_queries(H)
    depth = max(walk_stack_depth(nodes, root, n - 1, np.concatenate([boxes["min"][j], boxes["max"][j]])) for j in (0, 1, 2, 121))
    assert (depth > 64) == deep, depth
    leaf = tri_boxes(tris)
    ref_off, ref_prims = csr_of(overlap_brute_force(boxes, leaf))
    assert ref_off[1] == n and ref_off[-1] > n and (np.diff(ref_off.astype(np.int64)) == 0).sum() >= 120
    grown = leaf.copy()                                               # self mode takes d_boxes[i] AS primitive i's box: grown ones reach many side nodes
    grown["min"][:, 2] -= 60.0; grown["max"][:, 2] += 60.0
    grown[0] = boxes[0]                                               # ... and one reaches everything
    self_off, self_prims = csr_of(overlap_brute_force(grown, leaf, self_pairs=True))
    assert self_off[1] == n - 1
    c = pkg.Context(0)
    try:
        c.reserve(n)
        d_nodes, d_leaf = c.upload(nodes), c.upload(grown)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        c.set_profiling(2)
        rc, off, prims, total = overlap(pkg, c, r, boxes, guard=8)
        kt = c.kernel_times()
        c.set_profiling(0)
        assert {"k_overlap_count", "k_overlap_deep", "k_overlap_scan", "k_overlap_fill", "k_refit_plan"} <= set(kt), kt
        assert rc == 0 and total == int(ref_off[-1])
        check_answer(off, prims, ref_off, ref_prims, f"caterpillar {H}")
        rc, off, prims, total = overlap(pkg, c, r, (d_leaf.ptr, n), mode=pkg.OVERLAP_SELF, guard=8)
        assert rc == 0 and total == int(self_off[-1])
        check_answer(off, prims, self_off, self_prims, f"caterpillar {H} self")
        d_nodes.free(); d_leaf.free()
    finally:
        c.close()


# ---- 6. after refit, optimise, rebuild --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_after_refit_and_optimize(pkg, algo):
    a = mesh(pkg, "uniform_20000"); moved = jitter(a, 23, 2e-3)
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        leaf = tri_boxes(moved)
        boxes, _ = make_boxes(leaf, 77, points=vertices(moved))
        b.overlap(boxes)                                              # (the plan of the ctx's own tree is made here and kept)
        b.refit(moved)
        ref_off, ref_prims = csr_of(overlap_brute_force(boxes, leaf))
        off, prims = b.overlap(boxes)
        assert off.tobytes() == ref_off.tobytes() and sorted_slices(off, prims).tobytes() == ref_prims.tobytes(), f"refit algo {algo}"
        b.optimize(3)
        off, prims = b.overlap(boxes)
        assert off.tobytes() == ref_off.tobytes() and sorted_slices(off, prims).tobytes() == ref_prims.tobytes(), f"optimize algo {algo}"
        so, sp = b.overlap(self_pairs=True)
        ro, rp = csr_of(overlap_brute_force(leaf, leaf, self_pairs=True))
        assert so.tobytes() == ro.tobytes() and sorted_slices(so, sp).tobytes() == rp.tobytes()
    finally:
        c.close()


def with_root(nodes, root, new_root):
    """the same layout-0 tree with the internal records `root` and `new_root` exchanged (links follow): its root is then new_root"""
    out = nodes.copy()
    if root == new_root:
        return out
    out[[root, new_root]] = nodes[[new_root, root]]
    ni = (len(nodes) + 1) // 2 - 1
    for f in ("left", "right"):
        link = out[f][:ni].copy()
        out[f][:ni] = np.where(link == root, new_root, np.where(link == new_root, root, link))
    return out


@pytest.mark.parametrize("algo", [0, 1])
def test_rebuild_on_the_same_ctx_uses_a_fresh_plan(pkg, algo):
    """the ctx's own tree is made deep by writing the caterpillar's nodes over the builder's (bvh_dev_upload into the arena: the plan of the builder's tree no
    longer describes them), so the stackless pass really reads the plan; then the builder rebuilds on the same ctx and the plan must follow again, also when nothing but the rebuild
    says so"""
    H = 300
    tris, nodes, root, n = caterpillar(pkg, H, 5)
    boxes = caterpillar_queries(H)
    leaf = tri_boxes(tris)
    ref_off, ref_prims = csr_of(overlap_brute_force(boxes, leaf))
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, tris)
        assert b.result.layout == 0
        off, prims = b.overlap(boxes)                                 # the builder's own (shallow) tree: its plan is cached
        assert off.tobytes() == ref_off.tobytes() and sorted_slices(off, prims).tobytes() == ref_prims.tobytes()
        assert pkg.lib().bvh_dev_upload(c.handle, b.result.d_nodes, nodes.ctypes.data, nodes.nbytes) == 0
        b.result.root = root
        off, prims = b.overlap(boxes)                                 # deep now: a stale plan would walk the old topology's parents
        assert off.tobytes() == ref_off.tobytes() and sorted_slices(off, prims).tobytes() == ref_prims.tobytes()
        b.build(c, tris)
        off, prims = b.overlap(boxes)                                 # shallow again; the plan of THIS tree is cached now
        assert off.tobytes() == ref_off.tobytes() and sorted_slices(off, prims).tobytes() == ref_prims.tobytes()
        # the rebuild itself must make that plan stale.  Rebuild, then put the caterpillar (relabelled to the built root, so that only the serial can tell) over
        # the nodes through ANOTHER context, which this ctx's bookkeeping does not see: a plan kept across the rebuild would now be walked on the wrong tree
        b.build(c, tris)
        c.synchronize()
        c2 = pkg.Context(0)
        try:
            moved_nodes = with_root(nodes, root, int(b.result.root))
            assert pkg.lib().bvh_dev_upload(c2.handle, b.result.d_nodes, moved_nodes.ctypes.data, moved_nodes.nbytes) == 0
            c2.synchronize()
        finally:
            c2.close()
        off, prims = b.overlap(boxes)
        assert off.tobytes() == ref_off.tobytes() and sorted_slices(off, prims).tobytes() == ref_prims.tobytes()
    finally:
        c.close()


# ---- 7. other trees ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_build_boxes_tree(pkg, algo):
    rng = np.random.default_rng(40 + algo)
    n = 5000
    ctr = rng.random((n, 3)) * 10.0; half = rng.random((n, 3)) * 0.15
    leaf = as_boxes(np.concatenate([ctr - half, ctr + half], axis=1).astype(F32))
    boxes, _ = make_boxes(leaf, 3)
    ref_off, ref_prims = csr_of(overlap_brute_force(boxes, leaf))
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build_boxes(c, leaf)
        assert not b.result.d_tris
        off, prims = b.overlap(boxes)
        assert off.tobytes() == ref_off.tobytes() and sorted_slices(off, prims).tobytes() == ref_prims.tobytes()
        so, sp = b.overlap(self_pairs=True)                          # neighbour pairs of the boxes themselves
        ro, rp = csr_of(overlap_brute_force(leaf, leaf, self_pairs=True))
        assert ro[-1] > 0 and so.tobytes() == ro.tobytes() and sorted_slices(so, sp).tobytes() == rp.tobytes()
    finally:
        c.close()


def test_scene_top_level_tree(pkg):
    from test_gpu_scene import Blases, scene_instances
    rng = np.random.default_rng(64)
    meshes = [no_negzero(pkg.meshgen.uniform(k, 31 + k)) for k in (120, 100, 80, 60)]
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo]) for algo in range(4)]
        inst = scene_instances(pkg, rng, 64, 4, 1.5)
        for tlas_algo in (0, 2):
            scene = pkg.Scene(sc_ctx).build(tlas_algo, blases, inst)
            t = scene.tlas()
            assert t.n_leaves == 64
            world = np.zeros(64, dtype=pkg.AABB)
            assert pkg.lib().bvh_dev_download(sc_ctx.handle, world.ctypes.data, t.d_prim_aabbs, world.nbytes) == 0
            boxes, _ = make_boxes(world, 9)
            ref_off, ref_prims = csr_of(overlap_brute_force(boxes, world))
            assert ref_off[-1] > 64
            rc, off, prims, total = overlap(pkg, sc_ctx, t, boxes, guard=4)       # the answers are instance indices
            assert rc == 0 and total == int(ref_off[-1])
            check_answer(off, prims, ref_off, ref_prims, f"tlas algo {tlas_algo}")
            scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- 8. errors write nothing -----------------------------------------------------------------------------------------------------------------------------------

def test_errors_write_nothing(pkg):
    tris = mesh(pkg, "uniform_1000"); n = len(tris)
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        m = 256
        boxes = tri_boxes(tris)[:m]
        d_boxes = c.upload(boxes)
        guard_off = np.full(m + 1, GUARD, dtype=np.uint32); guard_prims = np.full(4096, GUARD, dtype=np.uint32)
        d_off, d_prims = c.upload(guard_off), c.upload(guard_prims)
        total = C.c_uint64(1234567)
        L = pkg.lib()

        def call(res=b.result, q=d_boxes.ptr, k=m, mode=0, off=d_off.ptr, prims=d_prims.ptr, cap=4096, ctx=c.handle):
            return L.bvh_overlap(ctx, C.byref(res) if res is not None else None, q, k, mode, off, prims, cap, C.byref(total))

        def variant(**kw):
            r = pkg.Result.from_buffer_copy(b.result)
            for key, v in kw.items():
                setattr(r, key, v)
            return r
        cases = {
            "null ctx": call(ctx=None), "null tree": call(res=None), "null boxes": call(q=None), "null offsets": call(off=None),
            "n_leaves 1": call(res=variant(n_leaves=1)), "layout 2": call(res=variant(layout=2)), "null nodes": call(res=variant(d_nodes=None)),
            "layout 1 without leaves": call(res=variant(d_leaves=None)), "root not internal": call(res=variant(root=n - 1)),
            "mode 2": call(mode=2), "mode -1": call(mode=-1),
            "self with n_boxes != n_leaves": call(mode=1), "n_boxes 2^30": call(k=1 << 30), "n_boxes 2^32 - 1": call(k=0xFFFFFFFF),
            "above capacity": call(res=variant(n_leaves=n + 1_000_000, root=0)),
            "offsets in boxes": call(off=d_boxes.ptr + 24), "boxes in offsets": call(q=d_off.ptr + 4, k=1),
            "prims in boxes": call(prims=d_boxes.ptr + 24 * (m - 1) + 20), "boxes in prims": call(q=d_prims.ptr + 4 * 4095, k=1),
            "prims in offsets": call(prims=d_off.ptr + 4 * m), "offsets in prims": call(off=d_prims.ptr + 4 * 4095),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        c.synchronize()
        assert total.value == 1234567
        assert d_off.download(np.uint32, m + 1).tobytes() == guard_off.tobytes() and d_prims.download(np.uint32, 4096).tobytes() == guard_prims.tobytes()
        assert d_boxes.download(pkg.AABB, m).tobytes() == boxes.tobytes()
        # a NULL d_prims is not an error, and its capacity names no range
        assert L.bvh_overlap(c.handle, C.byref(b.result), d_boxes.ptr, m, 0, d_off.ptr, None, 1 << 40, None) == 0
        d_off.upload(guard_off)
        # n_boxes == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        assert call(k=0) == 0
        c.synchronize()
        off = d_off.download(np.uint32, m + 1)
        assert total.value == 0 and off[0] == 0 and (off[1:] == GUARD).all() and d_prims.download(np.uint32, 4096).tobytes() == guard_prims.tobytes()
        # on a fresh ctx (capacity 0) a caller tree is refused until bvh_ctx_reserve
        d_off.upload(guard_off)
        c2 = pkg.Context(0)
        try:
            assert L.bvh_overlap(c2.handle, C.byref(b.result), d_boxes.ptr, m, 0, d_off.ptr, d_prims.ptr, 4096, None) == E_INVALID
        finally:
            c2.close()
        c.synchronize()
        assert d_off.download(np.uint32, m + 1).tobytes() == guard_off.tobytes()
        for x in (d_boxes, d_off, d_prims):
            x.free()
    finally:
        c.close()


# ---- 9. size -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_two_million_triangles_one_million_boxes(pkg, ctx):
    n, m = 2_000_000, 1_000_000
    tris = no_negzero(pkg.meshgen.uniform(n, 9))
    leaf = tri_boxes(tris)
    rng = np.random.default_rng(12)
    lo = leaf["min"].astype(np.float64).min(axis=0); hi = leaf["max"].astype(np.float64).max(axis=0); ext = hi - lo
    ctr = lo + rng.random((m, 3)) * ext; half = rng.random((m, 3)) * 0.02 * ext
    boxes = as_boxes(np.concatenate([ctr - half, ctr + half], axis=1).astype(F32))
    sample = np.sort(rng.choice(m, 2048, replace=False))
    qi, pj = overlap_pairs(boxes[sample], leaf)                       # chunked: a few queries against all boxes at a time
    want = np.bincount(qi, minlength=2048)
    for algo in (1, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        off, prims = b.overlap(boxes, capacity=64 * m)
        assert len(off) == m + 1 and off[0] == 0 and len(prims) == off[-1] and (np.diff(off.astype(np.int64)) >= 0).all()
        got = off[sample + 1].astype(np.int64) - off[sample]
        assert (got == want).all(), f"algo {algo}: {np.count_nonzero(got != want)} of 2048 sampled counts differ"
        print(f"2 M uniform, algo {algo}: mean results per query {off[-1] / m:.2f}")
        # every reported primitive of the sampled queries overlaps its query (and, the counts being equal, none is missing)
        ref = set(zip(qi.tolist(), pj.tolist()))
        for k, s in enumerate(sample):
            sl = prims[off[s]:off[s + 1]]
            assert len(set(sl.tolist())) == len(sl) and all((k, int(p)) in ref for p in sl), f"algo {algo} query {s}"
