"""bvh_cull on the GPU: every volume's whole set of records (primitive and straddle mask) of every builder, both node layouts and both walks against the numpy
brute force (pkg.cull_brute_force, the reference tests/test_cull.py checks) — exact, no tolerance, no volume left out —, the AUTO rule, trees from
bvh_build_boxes, after a refit and an optimise, a scene's top-level tree, the count / scan / fill passes and their capacity rule, determinism, errors, and
the hand-over of both walks to the stackless pass: the lane walk's short stack on a deep tree, the group walk's work stack on a tree made to fill it."""
import ctypes as C

import numpy as np
import pytest

from test_cull import (F32, N_SPECIAL, N_VOLUMES, PADDING, PLANE_COUNTS, Tree, by_prim, check_premises, family, fat_caterpillar, group_walk, lane_walk,
                       make_volumes, sorted_hits)
from test_gpu_overlap import tri_boxes, vertices
from test_gpu_query import caterpillar, lbvh_result, mesh
from test_gpu_refit import jitter, no_negzero
from test_overlap import E_INVALID, as_boxes, leaf_boxes_of

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
GUARD = 0xA5A5A5A5
SIZES = ["uniform_2", "uniform_3", "uniform_64", "uniform_65", "uniform_1000", "uniform_4096"]
VOLUME_COUNTS = (1, 63, 64, 65, 257)
LANE, GROUP, AUTO = 1, 2, 0
PATHS = {"lane": LANE, "group": GROUP, "auto": AUTO}


def run_cull(pkg, ctx, result, planes, path, capacity=None, want_hits=True, want_total=True, guard=0):
    """one bvh_cull call on guard-filled device arrays: -> (rc, offsets, hits (capacity + guard + 1 records) or None, total or None).  capacity None: a
    count-only call first, then the exact capacity"""
    planes = np.ascontiguousarray(planes, dtype=F32)
    m, per = planes.shape[0], planes.shape[1]
    d_planes = ctx.upload(planes) if m else ctx.alloc(16)
    d_off = ctx.upload(np.full(m + 1 + 4, GUARD, dtype=np.uint32))
    total = C.c_uint64(0xDEAD)
    L = pkg.lib()
    try:
        if capacity is None:
            rc = L.bvh_cull(ctx.handle, C.byref(result), d_planes.ptr, m, per, path, d_off.ptr, None, 0, C.byref(total))
            assert rc == 0, rc
            capacity = total.value
        d_hits = ctx.upload(np.full(2 * (capacity + guard + 1), GUARD, dtype=np.uint32)) if want_hits else None
        try:
            rc = L.bvh_cull(ctx.handle, C.byref(result), d_planes.ptr, m, per, path, d_off.ptr, d_hits.ptr if d_hits else None, capacity,
                            C.byref(total) if want_total else None)
            ctx.synchronize()
            off = d_off.download(np.uint32, m + 1 + 4)
            assert (off[m + 1:] == GUARD).all(), "d_offsets written past n_volumes + 1 words"
            hits = d_hits.download(pkg.CULL_HIT, capacity + guard + 1) if d_hits else None
            return rc, off[: m + 1], hits, (total.value if want_total else None)
        finally:
            if d_hits:
                d_hits.free()
    finally:
        d_off.free(); d_planes.free()


def untouched(hits):
    return bool((hits["prim"] == GUARD).all() and (hits["straddle"] == GUARD).all())


def check_answer(pkg, off, hits, ref_off, ref_hits, what):
    """whole sets: the offsets, and every slice's records in ascending prim order, byte for byte; nothing written past the total"""
    assert off.tobytes() == ref_off.tobytes(), f"{what}: offsets differ on {np.count_nonzero(off != ref_off)} words (first {np.nonzero(off != ref_off)[0][:6]})"
    total = int(ref_off[-1])
    got = sorted_hits(off, hits[:total])
    if got.tobytes() != ref_hits.tobytes():
        bad = [i for i in range(len(off) - 1) if got[off[i]:off[i + 1]].tobytes() != ref_hits[off[i]:off[i + 1]].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(off) - 1} slices differ (first {bad[:6]})")
    assert untouched(hits[total:]), f"{what}: d_hits written past the total"


def prefix(ref, count):
    """the reference of the first ``count`` volumes of a family"""
    off, hits = ref
    return off[: count + 1], hits[: off[count]]


def both_walks(pkg, ctx, result, vols, ref, what, paths=(LANE, GROUP, AUTO)):
    for path in paths:
        rc, off, hits, total = run_cull(pkg, ctx, result, vols, path, guard=4)
        assert rc == 0 and total == int(ref[0][-1])
        check_answer(pkg, off, hits, ref[0], ref[1], f"{what}, path {path}")


# ---- 1. exact on every volume, both walks -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SIZES)
def test_exact_on_every_volume(pkg, ctx, name):
    tris = mesh(pkg, name); n = len(tris)
    for per in PLANE_COUNTS:
        vols, ref, leaf = family(pkg, name, per)
        check_premises(ref[0], ref[1], n, f"{name} x {per} planes")
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, tris)
            if per == PLANE_COUNTS[0]:
                d = b.download()
                assert leaf_boxes_of(d["nodes"], d["leaves"], n, b.result.layout).tobytes() == leaf.tobytes()
            for count in (VOLUME_COUNTS if per == 6 else VOLUME_COUNTS[-2:]):
                both_walks(pkg, ctx, b.result, vols[:count], prefix(ref, count), f"{name} algo {algo}, {count} volumes x {per} planes")
            if b.result.layout == 1 and per == 6:                       # the same tree as caller-filled layout-0 arrays
                keep = []
                both_walks(pkg, ctx, lbvh_result(pkg, ctx, b, keep), vols, ref, f"{name} algo {algo} lbvh layout", paths=(LANE, GROUP))
                for k in keep:
                    k.free()
            for path in (PATHS if per == 6 else ()):                    # the Python binding: host arrays in, host arrays out
                off, hits = b.cull(vols, path=path)
                assert hits.dtype == pkg.CULL_HIT and off.tobytes() == ref[0].tobytes() and sorted_hits(off, hits).tobytes() == ref[1].tobytes()


def test_binding_forms(pkg, ctx):
    tris = mesh(pkg, "uniform_1000")
    vols, ref, _ = family(pkg, "uniform_1000", 6)
    b = pkg.HPLOC().build(ctx, tris)
    for form in (dict(), dict(capacity=1), dict(capacity=1 << 20), dict(path=pkg.CULL_GROUP)):
        off, hits = b.cull(vols, **form)
        assert off.tobytes() == ref[0].tobytes() and sorted_hits(off, hits).tobytes() == ref[1].tobytes()
    assert b.cull(vols, count_only=True).tobytes() == ref[0].tobytes()
    off, hits = pkg.cull(ctx, b.result, vols[7])                       # one volume as (planes, 4)
    assert off.tolist() == [0, ref[0][8] - ref[0][7]] and by_prim(hits).tobytes() == ref[1][ref[0][7]:ref[0][8]].tobytes()
    off, hits = b.cull(np.zeros((0, 6, 4), dtype=F32))
    assert off.tolist() == [0] and len(hits) == 0
    for bad in (np.zeros((3, 9, 4)), np.zeros((3, 6, 3)), np.zeros(4)):
        with pytest.raises(pkg.BvhError):
            b.cull(bad)
    with pytest.raises(pkg.BvhError):
        b.cull(vols, path="wave")


# ---- 2. the AUTO rule ---------------------------------------------------------------------------------------------------------------------------------------------

def test_auto_takes_the_walk_the_rule_names(pkg):
    """BVH_CULL_AUTO is the group walk iff n_volumes <= 65 536 and n_leaves >= 1024: each side of either bound, by the kernel names of a profiled call.  Up to
    514 volumes the answer is filled and compared whole; at the bound itself (the family repeated 256 times) the call counts only and the offsets are compared"""
    big, small = mesh(pkg, "uniform_4096"), mesh(pkg, "uniform_1000")
    assert len(small) < 1024 <= len(big)
    fam = family(pkg, "uniform_4096", 6)[0]
    c = pkg.Context(0)
    try:
        for tris, count, walk in ((big, 1, "k_cull_group"), (big, 257, "k_cull_group"), (small, 1, "k_cull_walk"), (small, 514, "k_cull_walk"),
                                  (big, 65536, "k_cull_group"), (big, 65537, "k_cull_walk")):
            b = pkg.PLOCNew().build(c, tris)
            filled = count <= 514
            ref = pkg.cull_brute_force(fam, tri_boxes(tris))
            reps = -(-count // N_VOLUMES)
            v = np.concatenate([fam] * reps)[:count]
            counts = np.tile(np.diff(ref[0].astype(np.int64)), reps)[:count]
            ref_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
            ref_hits = np.concatenate([ref[1]] * reps)[: ref_off[-1]] if filled else None
            c.set_profiling(2)
            rc, off, hits, total = run_cull(pkg, c, b.result, v, AUTO, capacity=int(ref_off[-1]) if filled else 0, want_hits=filled, guard=2)
            kt = c.kernel_times()
            c.set_profiling(0)
            other = "k_cull_walk" if walk == "k_cull_group" else "k_cull_group"
            assert walk in kt and other not in kt and {"k_cull_deep", "k_overlap_scan"} <= set(kt), (len(tris), count, kt)
            assert rc == 0 and total == int(ref_off[-1]) and off.tobytes() == ref_off.tobytes(), (len(tris), count)
            if filled:
                check_answer(pkg, off, hits, ref_off, ref_hits, f"auto {len(tris)} leaves, {count} volumes")
    finally:
        c.close()


# ---- 3. other trees -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_build_boxes_tree(pkg, algo):
    rng = np.random.default_rng(70 + algo)
    n = 3000
    ctr = rng.random((n, 3)) * 10.0; half = rng.random((n, 3)) * 0.15
    leaf = as_boxes(np.concatenate([ctr - half, ctr + half], axis=1).astype(F32))
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build_boxes(c, leaf)
        assert not b.result.d_tris
        for per in (1, 6):
            vols = make_volumes(pkg, leaf, np.concatenate([leaf["min"], leaf["max"]]), 3 + per, per, count=96)
            ref = pkg.cull_brute_force(vols, leaf)
            check_premises(ref[0], ref[1], n, "boxes")
            both_walks(pkg, c, b.result, vols, ref, f"build_boxes algo {algo} x {per}")
    finally:
        c.close()


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_after_refit_and_optimize(pkg, algo):
    a = mesh(pkg, "uniform_4096"); moved = jitter(a, 23, 2e-3)
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        leaf = tri_boxes(moved)
        vols = make_volumes(pkg, leaf, vertices(moved), 77, 6, count=96)
        b.cull(vols)                                                    # (the plan of the ctx's own tree is made here and kept)
        b.refit(moved)
        ref = pkg.cull_brute_force(vols, leaf)
        check_premises(ref[0], ref[1], len(a), "refit")
        both_walks(pkg, c, b.result, vols, ref, f"refit algo {algo}")
        b.optimize(3)
        both_walks(pkg, c, b.result, vols, ref, f"optimize algo {algo}")
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
        inst = scene_instances(pkg, rng, 48, 4, 1.5)
        for tlas_algo in (0, 2):
            scene = pkg.Scene(sc_ctx).build(tlas_algo, blases, inst)
            t = scene.tlas()
            assert t.n_leaves == 48
            world = np.zeros(48, dtype=pkg.AABB)
            assert pkg.lib().bvh_dev_download(sc_ctx.handle, world.ctypes.data, t.d_prim_aabbs, world.nbytes) == 0
            live = (world["min"] <= world["max"]).all(axis=1)          # (an inactive instance's world box is the reset box: it passes nothing)
            vols = make_volumes(pkg, world[live], np.concatenate([world["min"][live], world["max"][live]]), 9, 6, count=80)
            ref = pkg.cull_brute_force(vols, world)
            check_premises(ref[0], ref[1], int(live.sum()), "tlas")
            both_walks(pkg, sc_ctx, t, vols, ref, f"tlas algo {tlas_algo}")      # the answers are instance indices
            for path in PATHS:
                off, hits = scene.cull_instances(vols, path=path)
                assert off.tobytes() == ref[0].tobytes() and sorted_hits(off, hits).tobytes() == ref[1].tobytes()
            scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- 4. count only, too small a capacity, exact capacity, determinism ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo,path", [(1, LANE), (3, LANE), (1, GROUP), (3, GROUP)])
def test_passes_and_capacity(pkg, ctx, algo, path):
    tris = mesh(pkg, "uniform_1000")
    vols, (ref_off, ref_hits), _ = family(pkg, "uniform_1000", 6)
    total = int(ref_off[-1])
    b = pkg.BUILDERS[algo]().build(ctx, tris)
    rc, off, hits, t = run_cull(pkg, ctx, b.result, vols, path, capacity=0, want_hits=False)          # d_hits NULL: offsets and the total
    assert rc == 0 and t == total and hits is None and off.tobytes() == ref_off.tobytes()
    rc, off, hits, t = run_cull(pkg, ctx, b.result, vols, path, capacity=total - 1, guard=8)           # one record short: d_hits untouched, the total reported
    assert rc == 0 and t == total and off.tobytes() == ref_off.tobytes() and untouched(hits)
    rc, off, hits, t = run_cull(pkg, ctx, b.result, vols, path, capacity=total, guard=8)               # exactly enough
    assert rc == 0 and t == total
    check_answer(pkg, off, hits, ref_off, ref_hits, "exact capacity")
    rc, off2, hits2, t2 = run_cull(pkg, ctx, b.result, vols, path, capacity=total, guard=8, want_total=False)   # the same call again, no read-back: the same bytes
    assert rc == 0 and t2 is None and off2.tobytes() == off.tobytes() and hits2.tobytes() == hits.tobytes()
    rc, off3, hits3, _ = run_cull(pkg, ctx, b.result, vols, path, capacity=total - 1, guard=8, want_total=False)
    assert rc == 0 and off3.tobytes() == off.tobytes() and untouched(hits3)


# ---- 5. errors write nothing ------------------------------------------------------------------------------------------------------------------------------------

def test_errors_write_nothing(pkg):
    tris = mesh(pkg, "uniform_1000"); n = len(tris)
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        m, per = 64, 6
        vols = np.ascontiguousarray(family(pkg, "uniform_1000", 6)[0][:m])
        d_planes = c.upload(vols)
        guard_off = np.full(m + 1, GUARD, dtype=np.uint32); guard_hits = np.full(2 * 4096, GUARD, dtype=np.uint32)
        d_off, d_hits = c.upload(guard_off), c.upload(guard_hits)
        total = C.c_uint64(1234567)
        L = pkg.lib()
        vol_bytes = per * 16

        def call(res=b.result, q=d_planes.ptr, k=m, p=per, path=0, off=d_off.ptr, hits=d_hits.ptr, cap=4096, ctx=c.handle):
            return L.bvh_cull(ctx, C.byref(res) if res is not None else None, q, k, p, path, off, hits, cap, C.byref(total))

        def variant(**kw):
            r = pkg.Result.from_buffer_copy(b.result)
            for key, v in kw.items():
                setattr(r, key, v)
            return r
        cases = {
            "null ctx": call(ctx=None), "null tree": call(res=None), "null planes": call(q=None), "null offsets": call(off=None),
            "n_leaves 1": call(res=variant(n_leaves=1)), "layout 2": call(res=variant(layout=2)), "null nodes": call(res=variant(d_nodes=None)),
            "layout 1 without leaves": call(res=variant(d_leaves=None)), "root not internal": call(res=variant(root=n - 1)),
            "0 planes": call(p=0), "9 planes": call(p=9), "2^32 - 1 planes": call(p=0xFFFFFFFF), "path 3": call(path=3), "path -1": call(path=-1),
            "n_volumes 2^30": call(k=1 << 30), "n_volumes 2^32 - 1": call(k=0xFFFFFFFF),
            "above capacity": call(res=variant(n_leaves=n + 1_000_000, root=0)),
            "offsets in planes": call(off=d_planes.ptr + 16), "planes in offsets": call(q=d_off.ptr + 4, k=1, p=1),
            "hits in planes": call(hits=d_planes.ptr + vol_bytes * (m - 1) + 88), "planes in hits": call(q=d_hits.ptr + 8 * 4095, k=1, p=1),
            "hits in offsets": call(hits=d_off.ptr + 4 * m), "offsets in hits": call(off=d_hits.ptr + 8 * 4095),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        c.synchronize()
        assert total.value == 1234567
        assert d_off.download(np.uint32, m + 1).tobytes() == guard_off.tobytes() and d_hits.download(np.uint32, 2 * 4096).tobytes() == guard_hits.tobytes()
        assert d_planes.download(F32, vols.size).tobytes() == vols.tobytes()
        # a NULL d_hits is not an error, and its capacity names no range
        assert L.bvh_cull(c.handle, C.byref(b.result), d_planes.ptr, m, per, 0, d_off.ptr, None, 1 << 40, None) == 0
        d_off.upload(guard_off)
        # n_volumes == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        assert call(k=0) == 0
        c.synchronize()
        off = d_off.download(np.uint32, m + 1)
        assert total.value == 0 and off[0] == 0 and (off[1:] == GUARD).all() and d_hits.download(np.uint32, 2 * 4096).tobytes() == guard_hits.tobytes()
        # on a fresh ctx (capacity 0) a caller tree is refused until bvh_ctx_reserve
        d_off.upload(guard_off)
        c2 = pkg.Context(0)
        try:
            assert L.bvh_cull(c2.handle, C.byref(b.result), d_planes.ptr, m, per, 0, d_off.ptr, d_hits.ptr, 4096, None) == E_INVALID
        finally:
            c2.close()
        c.synchronize()
        assert d_off.download(np.uint32, m + 1).tobytes() == guard_off.tobytes()
        for x in (d_planes, d_off, d_hits):
            x.free()
    finally:
        c.close()


# ---- 6. the lane walk's short stack -----------------------------------------------------------------------------------------------------------------------------

def caterpillar_volumes(H):
    """six planes each: everything; z slabs over some of the far side nodes; every far triangle; nothing (below, beside, between); the near triangle alone"""
    rng = np.random.default_rng(H)

    def slab(z0, z1, x0=-100.0, x1=100.0):
        return [(0.0, 0.0, 1.0, -z0), (0.0, 0.0, -1.0, z1), (1.0, 0.0, 0.0, -x0), (-1.0, 0.0, 0.0, x1), PADDING, PADDING]
    v = [[PADDING] * 6, slab(-100.0, 5000.0)]
    for _ in range(60):
        a = rng.uniform(0, 2 * H - 1)
        v.append(slab(1000.0 + a, 1000.0 + a + rng.uniform(0, 40)))
    v.append(slab(999.5, 1000.0 + 2 * H))
    for _ in range(20):
        v += [slab(-9.0 - rng.uniform(0, 5), -8.0), slab(0.0, 5000.0, 40.0, 50.0), slab(0.625, 999.0)]
    v.append(slab(0.0, 0.25))
    return np.array(v, dtype=np.float64).astype(F32)


@pytest.mark.parametrize("H,deep", [(300, True), (20, False)])
def test_deep_tree_takes_the_stackless_pass(pkg, H, deep):
    """caterpillar(H) (tests/test_gpu_query.py): for a volume that contains everything the lane walk's stack grows by one at every level whose left child is
    the chain, about H / 2 entries.  H = 300 is far above the 64 of the short stack, so the stackless pass must serve those volumes in the count AND in the
    fill pass; H = 20 is the control that stays in the short stack on the same code path.  The depth is the host walk's."""
    tris, nodes, root, n = caterpillar(pkg, H, 11 + H)
    vols = caterpillar_volumes(H)
    tree = Tree(nodes, None, root, n, 0)
    depth = max(lane_walk(pkg, tree, vols[j], False)[1] for j in (0, 1, 2, 62))
    assert (depth > 64) == deep, depth
    leaf = tri_boxes(tris)
    ref = pkg.cull_brute_force(vols, leaf)
    counts = np.diff(ref[0].astype(np.int64))
    assert counts[0] == n and counts[1] == n and (counts == 0).sum() >= 60 and ((counts > 0) & (counts < n)).sum() >= 40
    c = pkg.Context(0)
    try:
        c.reserve(n)
        d_nodes = c.upload(nodes)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        c.set_profiling(2)
        rc, off, hits, total = run_cull(pkg, c, r, vols, LANE, guard=8)
        kt = c.kernel_times()
        c.set_profiling(0)
        assert {"k_cull_walk", "k_cull_deep", "k_overlap_scan", "k_refit_plan"} <= set(kt) and "k_cull_group" not in kt, kt
        assert rc == 0 and total == int(ref[0][-1])
        check_answer(pkg, off, hits, ref[0], ref[1], f"caterpillar {H}, lane")
        both_walks(pkg, c, r, vols, ref, f"caterpillar {H}", paths=(GROUP, AUTO))
        d_nodes.free()
    finally:
        c.close()


# ---- 7. the group walk's work stack -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels,over", [(32, True), (31, False)])
def test_group_stack_overflow_hands_over_to_the_stackless_pass(pkg, levels, over):
    """fat_caterpillar(levels) (tests/test_cull.py) makes the LIFO-256 schedule's stack grow by 256 entries per round: by the host restatement an
    all-containing volume reaches 8448 entries at 32 levels — above BVH_CULL_GROUP_STACK, the smallest such tree of the family — and exactly 8192 at 31, the
    control that stays in the group walk.  Beside it: volumes that stay far below the capacity, so marked and unmarked volumes share a launch.  Count and fill
    equal the brute force either way.  (A uniform mesh does not get there at any size that fits a test — see test_uniform_mesh_stays_in_the_group_walk.)"""
    leaf, nodes, root, n = fat_caterpillar(pkg, levels)
    tree = Tree(nodes, None, root, n, 0)
    vols = make_volumes(pkg, leaf, np.concatenate([leaf["min"], leaf["max"]]), 5, 6, count=24)
    vols[11] = vols[0]                                                  # everything, twice
    peaks = [group_walk(pkg, tree, v)[1] for v in vols]
    assert (peaks[0] > pkg.CULL_GROUP_STACK) == over and peaks[0] == 256 * (levels - 1) + 512, peaks[0]
    marked = [p > pkg.CULL_GROUP_STACK for p in peaks]
    assert peaks[11] == peaks[0] and any(marked) == over and not all(marked) and any(1 < p < pkg.CULL_GROUP_STACK // 2 for p in peaks), peaks
    ref = pkg.cull_brute_force(vols, leaf)
    check_premises(ref[0], ref[1], n, "fat caterpillar")
    c = pkg.Context(0)
    try:
        c.reserve(n)
        d_nodes = c.upload(nodes)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        c.set_profiling(2)
        rc, off, hits, total = run_cull(pkg, c, r, vols, GROUP, guard=8)
        kt = c.kernel_times()
        c.set_profiling(0)
        assert {"k_cull_group", "k_cull_deep", "k_overlap_scan", "k_refit_plan"} <= set(kt) and "k_cull_walk" not in kt, kt
        assert rc == 0 and total == int(ref[0][-1])
        check_answer(pkg, off, hits, ref[0], ref[1], f"fat caterpillar {levels}, group")
        rc, off2, hits2, _ = run_cull(pkg, c, r, vols, GROUP, guard=8)
        assert off2.tobytes() == off.tobytes() and hits2.tobytes() == hits.tobytes()      # the same bytes, served by either walk
        both_walks(pkg, c, r, vols, ref, f"fat caterpillar {levels}", paths=(LANE, AUTO))
        d_nodes.free()
    finally:
        c.close()


def test_uniform_mesh_stays_in_the_group_walk(pkg, ctx):
    """the schedule's occupancy on built trees grows by about 256 entries per doubling of the mesh: 2^17 uniform triangles reach about 2000 of the 8192
    entries (the host restatement on the downloaded trees), so one camera frustum on a large tree is served by the group walk alone; its slice is the schedule's
    emission order, byte for byte"""
    n = 1 << 17
    tris = no_negzero(pkg.meshgen.uniform(n, 3))
    leaf = tri_boxes(tris)
    vols = make_volumes(pkg, leaf, vertices(tris), 41, 6, count=N_SPECIAL + 6)
    ref = pkg.cull_brute_force(vols, leaf)
    for algo in (1, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        d = b.download()
        tree = Tree(d["nodes"], d["leaves"], b.result.root, n, b.result.layout)
        order, peak = group_walk(pkg, tree, vols[0])
        print(f"2^17 uniform, algo {algo}: occupancy {peak} of {pkg.CULL_GROUP_STACK}")
        assert 1024 < peak < pkg.CULL_GROUP_STACK // 2, peak
        rc, off, hits, total = run_cull(pkg, ctx, b.result, vols, GROUP, guard=4)
        assert rc == 0 and total == int(ref[0][-1])
        check_answer(pkg, off, hits, ref[0], ref[1], f"2^17 algo {algo}, group")
        assert hits[: off[1]].tobytes() == order.tobytes(), "volume 0's slice is not in the schedule's emission order"
        both_walks(pkg, ctx, b.result, vols, ref, f"2^17 algo {algo}", paths=(LANE, AUTO))
