"""bvh_scene_overlap on the GPU: which triangles' leaf boxes of which active instances each world-space query box touches, against the two-level numpy
brute force (tests/test_scene_overlap.py, which also makes the inputs and checks their premises without a device) on EVERY query — there is no
well-conditioned share: sorted, unsorted and count-only calls for 1 to 64 instances over BLASes of every builder, triangle format and layout, sheared,
mirrored and far-offset instances, coincident instances, touching, inverted and NaN boxes, one identity instance against bvh_overlap, the instances seen
against bvh_overlap on the top-level tree, independence from the builders, a deep BLAS and a deep top level through the stackless pass, bvh_scene_update
after moves and after a BLAS refit, the passes and the capacity decision, rejections and buffer hygiene, the binding's input kinds."""
import ctypes as C

import numpy as np
import pytest

from test_deep_trees import combined
from test_gpu_overlap import overlap as tree_overlap
from test_gpu_scene import TLAS_ALGO, Blases
from test_gpu_scene_knn import same_root_boxes
from test_overlap import csr_of, overlap_brute_force, sorted_slices
from test_query import E_INVALID
from test_scene import identity, make_instances
from test_scene_knn import inactive_of
from test_scene_overlap import (INSTANCE_PRIM, QUERY_STACK, SCENE_OVERLAP_SORTED, check_scene_overlap, left_first_scene_need,
                                overlap_builders_inputs, overlap_coincident_inputs, overlap_deep_inputs, overlap_deep_top_inputs, overlap_exact_inputs, overlap_kinds_inputs,
                                overlap_moved_inputs, overlap_small_inputs, scene_host_sort, scene_overlap_brute_force, slice_queries, tri_leaf_boxes)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32


def call(pkg, scene, d_boxes, m, flags, d_offsets, d_prims, capacity, total=True):
    t = C.c_uint64(0xDEAD)
    rc = pkg.lib().bvh_scene_overlap(scene.handle, d_boxes, m, flags, d_offsets, d_prims, capacity, C.byref(t) if total else None)
    return rc, t.value


def search(pkg, scene, boxes, flags):
    """count-only call, then a fill with the exact capacity; returns (offsets, records).  The count-only offsets must equal the fill's."""
    ctx, m = scene.ctx, len(boxes)
    d_boxes, d_off = ctx.upload(boxes), ctx.alloc((m + 1) * 4)
    prims = None
    try:
        rc, total = call(pkg, scene, d_boxes.ptr, m, flags, d_off.ptr, None, 0)
        assert rc == 0, rc
        counted = d_off.download(np.uint32, m + 1)
        assert counted[0] == 0 and counted[-1] == total
        prims = ctx.alloc(max(total, 1) * 8)
        rc, total2 = call(pkg, scene, d_boxes.ptr, m, flags, d_off.ptr, prims.ptr, total)
        assert rc == 0 and total2 == total
        off = d_off.download(np.uint32, m + 1)
        assert off.tobytes() == counted.tobytes(), "count-only and fill calls disagree on the offsets"
        return off, prims.download(pkg.INSTANCE_PRIM, total)
    finally:
        d_boxes.free(); d_off.free()
        if prims is not None:
            prims.free()


def check_all_ways(pkg, scene, boxes, ref, what):
    """the sorted fill against the brute force on every query; the unsorted fill set-equal to the sorted one and byte-equal to itself when called twice;
    the count-only offsets equal to the fill's (search asserts it).  Returns the sorted answer"""
    off, recs = search(pkg, scene, boxes, SCENE_OVERLAP_SORTED)
    check_scene_overlap(off, recs, ref, True, what + " sorted")
    uoff, urecs = search(pkg, scene, boxes, 0)
    check_scene_overlap(uoff, urecs, ref, False, what + " unsorted")
    assert scene_host_sort(uoff, urecs).tobytes() == recs.tobytes(), f"{what}: the unsorted slices are not the sorted ones as sets"
    uoff2, urecs2 = search(pkg, scene, boxes, 0)
    assert uoff2.tobytes() == uoff.tobytes() and urecs2.tobytes() == urecs.tobytes(), f"{what}: the same unsorted call twice gives other bytes"
    return off, recs


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_inst", [1, 2, 3, 64])
def test_exact_on_every_query(pkg, n_inst):
    """1: no top-level tree; 2: a root with two leaf children; 3: the singular instance inactive; 64: all three kinds of inactive instance.  BLAS b comes
    from builder b (layouts 0 and 1) in triangle format b % 3"""
    meshes, inst, boxes, ref = overlap_exact_inputs(pkg, n_inst)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo], fmt=algo % 3) for algo in range(4)]
        same_root_boxes(pkg, blases, meshes)
        layouts = {(b[0] if isinstance(b, tuple) else b).result.layout for b in blases}
        assert layouts == {0, 1}
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[n_inst], blases, inst)
        off, recs = check_all_ways(pkg, scene, boxes, ref, f"{n_inst} instances")
        assert not set(recs["instance"].tolist()) & inactive_of(n_inst), "an inactive instance answered"
        poff, precs = scene.overlap(boxes)                                # the Python binding, host boxes
        assert poff.tobytes() == off.tobytes() and precs.tobytes() == recs.tobytes()
        d = sc_ctx.upload(boxes)                                          # ... and device boxes
        doff, drecs = scene.overlap(d)
        assert doff.tobytes() == off.tobytes() and drecs.tobytes() == recs.tobytes()
        assert scene.overlap(d, count_only=True).tobytes() == off.tobytes()
        d.free()
        if n_inst == 3:                                                   # 65 boxes: a partial last wave
            _, _, boxes65, ref65 = overlap_exact_inputs(pkg, 3, m=65)
            check_all_ways(pkg, scene, boxes65, ref65, "65 boxes")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("kind", ["shear", "mirror", "far"])
def test_sheared_mirrored_and_far_offset_instances(pkg, kind):
    """... and, in every set, two boxes that share exactly one face with a mapped leaf box (reported), two inverted boxes and two with a NaN (empty)"""
    mesh, inst, boxes, touching, ref = overlap_kinds_inputs(pkg, kind)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        same_root_boxes(pkg, [b], [mesh])
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        off, recs = check_all_ways(pkg, scene, boxes, ref, kind)
        lens = np.diff(off.astype(np.int64))
        assert (lens[touching] >= 1).all() and (lens[-4:] == 0).all()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("tlas_algo", [0, 3])
def test_coincident_instances_report_every_pair_once_per_instance(pkg, tlas_algo):
    """two instances place the same triangles identically; one BLAS also holds a far-off extra triangle that stretches its world box, so the two are not
    walked alike.  Every shared triangle that a box touches is reported for instance 0 and for instance 1, whichever BLAS is the stretched one."""
    mesh, stretched, inst, boxes = overlap_coincident_inputs(pkg, tlas_algo)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        plain, far = bl.add(3, mesh), bl.add(1, stretched)
        for order in ((plain, far), (far, plain)):
            blas_tris = [mesh, stretched] if order[0] is plain else [stretched, mesh]
            ref = scene_overlap_brute_force(boxes, [tri_leaf_boxes(t) for t in blas_tris], inst)
            scene = pkg.Scene(sc_ctx).build(tlas_algo, list(order), inst)
            off, recs = check_all_ways(pkg, scene, boxes, ref, "coincident")
            q = slice_queries(off)
            shared = recs["prim"] < len(mesh)
            a, b = shared & (recs["instance"] == 0), shared & (recs["instance"] == 1)
            assert a.sum() == b.sum() > 1000 and np.array_equal(q[a], q[b]) and np.array_equal(recs["prim"][a], recs["prim"][b])
            scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- relations --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [1, 3])
def test_one_identity_instance_equals_overlap(pkg, algo):
    """((1 x + 0 y) + 0 z) + 0 == x as a value: the prim sets are bvh_overlap's on the BLAS for every query"""
    meshes, _, boxes, _ = overlap_exact_inputs(pkg, 1)
    mesh = meshes[0]
    inst = make_instances(pkg, [identity()], [0])
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(algo, mesh)
        assert b.result.layout == (0 if algo == 1 else 1)
        foff, fprims = b.overlap(boxes)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        off, recs = scene.overlap(boxes)
        assert len(recs) > 1000 and (recs["instance"] == 0).all()
        assert off.tobytes() == foff.tobytes() and recs["prim"].tobytes() == sorted_slices(foff, fprims).tobytes()
        ref_off, ref_prims = csr_of(overlap_brute_force(boxes, tri_leaf_boxes(mesh)))
        assert off.tobytes() == ref_off.tobytes() and recs["prim"].tobytes() == ref_prims.tobytes()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_instances_seen_are_a_subset_of_overlap_on_the_top_level_tree(pkg):
    meshes, inst, boxes, ref = overlap_exact_inputs(pkg, 64)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo]) for algo in range(4)]
        scene = pkg.Scene(sc_ctx).build(2, blases, inst)
        off, recs = scene.overlap(boxes)
        rc, toff, tprims, _ = tree_overlap(pkg, sc_ctx, scene.tlas(), boxes)
        assert rc == 0
        q = slice_queries(off)
        seen = set(zip(q.tolist(), recs["instance"].tolist()))
        broad = set(zip(slice_queries(toff).tolist(), tprims[: int(toff[-1])].tolist()))
        assert seen and seen <= broad and len(seen) < len(broad)          # (a world box is touched more often than a leaf box inside it)
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- independence, depth and updates ----------------------------------------------------------------------------------------------------------------------------

def test_independent_of_builders(pkg):
    mesh, one, boxes, ref = overlap_builders_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, mesh, fmt=algo % 3) for algo in range(4)]
        same_root_boxes(pkg, blases, [mesh] * 4)
        outs = []
        for tl in range(4):                                               # top-level builders over the same BLAS
            outs.append((f"top-level builder {tl}", pkg.Scene(sc_ctx).build(tl, [blases[3]], one).overlap(boxes)))
        for b in range(3):                                                # BLAS builders (and layouts, and formats) of the same mesh
            outs.append((f"BLAS builder {b}", pkg.Scene(sc_ctx).build(3, [blases[b]], one).overlap(boxes)))
        for what, (off, recs) in outs:
            assert off.tobytes() == ref["offsets"].tobytes() and recs.tobytes() == ref["recs"].tobytes(), what
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("H,deep", [(300, True), (20, False)])
def test_deep_blas_takes_the_stackless_pass(pkg, H, deep):
    """the caterpillar under five instances: a box that covers an instance needs about H / 2 stack entries in its BLAS (tests/test_gpu_overlap.py).  H = 300
    overflows the short stack in the count AND in the fill pass, in every wave beside queries that stay in it; H = 20 is the control on the same code path"""
    tris, nodes, root, n, inst, boxes, ref, need = overlap_deep_inputs(pkg, H)
    assert ((need > QUERY_STACK).sum() >= 64) == deep and (deep or need.max() + len(inst) - 1 <= QUERY_STACK), need.max()
    c, sc_ctx = pkg.Context(0), pkg.Context(0)
    try:
        d_tris, d_nodes = c.upload(tris), c.upload(nodes)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
        sc_ctx.set_profiling(2)
        off, recs = search(pkg, scene, boxes, SCENE_OVERLAP_SORTED)           # (asserts that the count-only and the fill call agree)
        kt = sc_ctx.kernel_times()
        sc_ctx.set_profiling(0)
        assert {"k_scene_overlap_count", "k_scene_overlap_fill", "k_scene_overlap_deep", "k_overlap_scan"} <= set(kt), sorted(kt)
        launches = {k: v[1] for k, v in kt.items()}                       # (search: a count-only call, then a call that counts and fills)
        assert launches["k_scene_overlap_count"] == 2 and launches["k_scene_overlap_fill"] == 1 and launches["k_overlap_scan"] == 2, launches
        assert launches["k_scene_overlap_deep"] == 3, "k_scene_overlap_deep does not follow every pass"
        check_scene_overlap(off, recs, ref, True, f"caterpillar {H}")
        uoff, urecs = search(pkg, scene, boxes, 0)
        check_scene_overlap(uoff, urecs, ref, False, f"caterpillar {H} unsorted")
        assert scene.overlap(boxes, count_only=True).tobytes() == off.tobytes()
        scene.close(); d_nodes.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()


@pytest.mark.parametrize("tlas_algo", [2, 3])
def test_deep_top_level_takes_the_stackless_pass(pkg, tlas_algo):
    """180 instances on the staircase: the PLOC-family top-level trees chain the steps up, and a box that covers them all pushes at every chain node"""
    mesh, inst, boxes, ref = overlap_deep_top_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        scene = pkg.Scene(sc_ctx).build(tlas_algo, [b], inst)
        t = scene.tlas()
        nodes = np.empty(t.n_leaves - 1, dtype=pkg.BVH2_NODE); leaves = np.empty(t.n_leaves, dtype=pkg.PRIMREF)
        assert t.n_leaves == 180 and t.layout == 1
        assert pkg.lib().bvh_download(sc_ctx.handle, C.byref(t), nodes.ctypes.data, leaves.ctypes.data, None, None, None) == 0
        top = combined(pkg, nodes, leaves)
        q = np.concatenate([boxes["min"], boxes["max"]], axis=1)

        def top_need(i):
            with np.errstate(invalid="ignore"):
                passes = (q[i, :3] <= top["max"]).all(axis=1) & (top["min"] <= q[i, 3:]).all(axis=1) & (top["min"] <= top["max"]).all(axis=1)
            return left_first_scene_need(top, int(t.root), 180, passes, True)
        deep_need, quiet_need = top_need(0), max(top_need(i) for i in range(1, len(boxes), 2))
        print(f"tlas algo {tlas_algo}: the covering box needs {deep_need} entries at the top level, the others at most {quiet_need}")
        assert deep_need > QUERY_STACK and quiet_need + 8 <= QUERY_STACK
        check_all_ways(pkg, scene, boxes, ref, f"deep top level, algo {tlas_algo}")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_update_after_moves_and_blas_refit(pkg):
    meshes, inst, moved, boxes, refit, ref_moved, ref_refit = overlap_moved_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        before = scene.overlap(boxes, count_only=True)
        scene.update(moved)
        same_root_boxes(pkg, blases, meshes)
        off, recs = check_all_ways(pkg, scene, boxes, ref_moved, "after update")
        assert before.tobytes() != off.tobytes()
        foff, frecs = pkg.Scene(sc_ctx).build(3, blases, moved).overlap(boxes)
        assert foff.tobytes() == off.tobytes() and frecs.tobytes() == recs.tobytes(), "an updated and a freshly built scene differ"
        blases[0].refit(refit[0])
        bl.ctxs[0].synchronize()                                          # (the refit ran on the BLAS's own stream: complete before the scene reads the root box)
        scene.update(moved)
        same_root_boxes(pkg, blases, refit)
        check_all_ways(pkg, scene, boxes, ref_refit, "after BLAS refit")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- passes, capacity, argument handling and memory hygiene -------------------------------------------------------------------------------------------------------

def small_scene(pkg, bl):
    mesh, inst, boxes, ref = overlap_small_inputs(pkg)
    return mesh, bl.add(3, mesh), inst, boxes, ref


def test_passes_and_capacity(pkg):
    bl, ctx = Blases(pkg), pkg.Context(0)
    try:
        mesh, b, inst, boxes, ref = small_scene(pkg, bl)
        scene = pkg.Scene(ctx).build(2, [b], inst)
        m = len(boxes)
        want = {flags: search(pkg, scene, boxes, flags) for flags in (SCENE_OVERLAP_SORTED, 0)}
        exp_off = want[0][0]
        total = int(exp_off[-1])
        assert total > 100 and want[SCENE_OVERLAP_SORTED][0].tobytes() == exp_off.tobytes()
        check_scene_overlap(exp_off, want[SCENE_OVERLAP_SORTED][1], ref, True, "small scene")
        extra = 29
        guard_p = np.frombuffer(np.full((total + extra) * 8, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_PRIM)
        guard_o = np.full(m + 1 + extra, 0xA5A5A5A5, dtype=np.uint32)
        d_boxes, d_off, d_prims = ctx.upload(boxes), ctx.upload(guard_o), ctx.upload(guard_p)
        for flags in (SCENE_OVERLAP_SORTED, 0):
            out = {}
            # count only: d_prims untouched, offsets complete, guard words past n_boxes + 1 offsets intact
            d_off.upload(guard_o); d_prims.upload(guard_p)
            assert call(pkg, scene, d_boxes.ptr, m, flags, d_off.ptr, None, 0) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_prims.download(pkg.INSTANCE_PRIM, total + extra).tobytes() == guard_p.tobytes()
            # capacity total - 1: the fill is skipped, d_offsets still complete, *total_out set
            d_off.upload(guard_o)
            assert call(pkg, scene, d_boxes.ptr, m, flags, d_off.ptr, d_prims.ptr, total - 1) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_prims.download(pkg.INSTANCE_PRIM, total + extra).tobytes() == guard_p.tobytes()
            # the exact capacity is filled; guard records past the total intact; twice the same bytes
            for rnd in range(2):
                d_off.upload(guard_o); d_prims.upload(guard_p)
                assert call(pkg, scene, d_boxes.ptr, m, flags, d_off.ptr, d_prims.ptr, total) == (0, total)
                o, p = d_off.download(np.uint32, m + 1 + extra), d_prims.download(pkg.INSTANCE_PRIM, total + extra)
                assert o[m + 1:].tobytes() == guard_o[m + 1:].tobytes() and p[total:].tobytes() == guard_p[total:].tobytes()
                assert o[: m + 1].tobytes() == exp_off.tobytes() and p[:total].tobytes() == want[flags][1].tobytes()
                out[rnd] = (o.tobytes(), p.tobytes())
            assert out[0] == out[1], "two identical calls give different bytes"
            # total_out == NULL: the same device bytes after a synchronize
            d_off.upload(guard_o); d_prims.upload(guard_p)
            rc, t = call(pkg, scene, d_boxes.ptr, m, flags, d_off.ptr, d_prims.ptr, total + extra, total=False)
            assert rc == 0 and t == 0xDEAD
            ctx.synchronize()
            assert (d_off.download(np.uint32, m + 1 + extra).tobytes(), d_prims.download(pkg.INSTANCE_PRIM, total + extra).tobytes()) == out[0]
            assert d_boxes.download(pkg.AABB, m).tobytes() == boxes.tobytes()
        # n_boxes == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        d_off.upload(guard_o); d_prims.upload(guard_p)
        assert call(pkg, scene, d_boxes.ptr, 0, SCENE_OVERLAP_SORTED, d_off.ptr, d_prims.ptr, total) == (0, 0)
        o = d_off.download(np.uint32, m + 1 + extra)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes() and d_prims.download(pkg.INSTANCE_PRIM, total + extra).tobytes() == guard_p.tobytes()
        # the binding's capacity protocol: a capacity that is too small is re-allocated from the reported total
        qoff, qrecs = scene.overlap(boxes, sorted=False, capacity=3)
        assert qoff.tobytes() == exp_off.tobytes() and qrecs.tobytes() == want[0][1].tobytes()
        scene.close(); d_boxes.free(); d_off.free(); d_prims.free()
    finally:
        bl.close(); ctx.close()


def test_one_instance_on_a_fresh_ctx(pkg):
    """a one-instance scene builds no top-level tree, so a fresh ctx has no arena yet: the first call reserves the smallest one"""
    mesh, inst, boxes, _ = overlap_small_inputs(pkg)
    one = inst[:1].copy()
    ref = scene_overlap_brute_force(boxes, [tri_leaf_boxes(mesh)], one)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        scene = pkg.Scene(sc_ctx).build(3, [bl.add(2, mesh)], one)
        off, recs = scene.overlap(boxes)
        check_scene_overlap(off, recs, ref, True, "fresh ctx")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_errors_write_nothing(pkg):
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    L = pkg.lib()
    try:
        mesh, b, inst, boxes, ref = small_scene(pkg, bl)
        m = len(boxes)
        d_boxes = sc_ctx.upload(boxes)
        cap = int(ref["offsets"][-1]) + 64
        guard_p = np.frombuffer(np.full(cap * 8, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_PRIM)
        guard_o = np.full(m + 1, 0x5A5A5A5A, dtype=np.uint32)
        prims, offs = sc_ctx.upload(guard_p), sc_ctx.upload(guard_o)
        tot = C.c_uint64(0x77)
        unbuilt, scene = pkg.Scene(sc_ctx), pkg.Scene(sc_ctx).build(2, [b], inst)

        def go(sc=scene, p=d_boxes.ptr, n=m, flags=SCENE_OVERLAP_SORTED, o=offs.ptr, h=prims.ptr, k=cap):
            return L.bvh_scene_overlap(sc.handle if sc is not None else None, p, n, flags, o, h, k, C.byref(tot))
        cases = {
            "null scene": go(sc=None), "unbuilt scene": go(sc=unbuilt), "null boxes": go(p=None), "null offsets": go(o=None),
            "flag 2": go(flags=2), "flag 3": go(flags=3), "flag high": go(flags=0x80000000),
            "n_boxes 2^30": go(n=1 << 30),
            "offsets in boxes": go(o=d_boxes.ptr + 48), "prims in boxes": go(h=d_boxes.ptr + 24), "prims in offsets": go(h=offs.ptr + 16),
            "offsets in prims": go(o=prims.ptr + 8 * (cap - 1)), "boxes in prims": go(p=prims.ptr, h=prims.ptr + 8 * 8),
            "prims over the boxes, capacity clamped": go(h=d_boxes.ptr - 16, k=1 << 40),
            "unbuilt, n_boxes 0": go(sc=unbuilt, n=0),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        assert tot.value == 0x77
        sc_ctx.synchronize()
        assert prims.download(pkg.INSTANCE_PRIM, cap).tobytes() == guard_p.tobytes() and offs.download(np.uint32, m + 1).tobytes() == guard_o.tobytes()
        assert d_boxes.download(pkg.AABB, m).tobytes() == boxes.tobytes()
        # a count-only call ignores the capacity's range, and the scene still answers
        assert go(h=None, k=1 << 40) == 0 and tot.value == ref["offsets"][-1]
        total = tot.value
        assert offs.download(np.uint32, m + 1)[-1] == total and prims.download(pkg.INSTANCE_PRIM, cap).tobytes() == guard_p.tobytes()
        assert go() == 0 and tot.value == total
        got = prims.download(pkg.INSTANCE_PRIM, cap)
        assert got[total:].tobytes() == guard_p[total:].tobytes()
        check_scene_overlap(offs.download(np.uint32, m + 1), got[:total], ref, True, "after the errors")
        # n_boxes == 0 on a built scene: d_offsets[0] = 0 and *total_out = 0
        offs.upload(guard_o)
        assert go(n=0) == 0 and tot.value == 0
        o = offs.download(np.uint32, m + 1)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes()
        scene.close(); unbuilt.close(); d_boxes.free(); prims.free(); offs.free()
    finally:
        bl.close(); sc_ctx.close()


def test_binding_takes_every_input_kind(pkg):
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        mesh, b, inst, boxes, ref = small_scene(pkg, bl)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        want_o, want_r = scene.overlap(boxes)
        assert want_o.shape == (len(boxes) + 1,) and want_o.dtype == np.uint32 and want_r.dtype == pkg.INSTANCE_PRIM == INSTANCE_PRIM and len(want_r) == want_o[-1] > 100
        check_scene_overlap(want_o, want_r, ref, True, "binding")
        flat = np.concatenate([boxes["min"], boxes["max"]], axis=1)
        d = sc_ctx.upload(boxes)
        for o, r in (scene.overlap(flat), scene.overlap(flat.reshape(-1, 2, 3)), scene.overlap(flat.astype(np.float64)), scene.overlap(d),
                     scene.overlap(d.ptr, n_boxes=len(boxes)), scene.overlap(boxes, capacity=len(want_r) + 5), scene.overlap(boxes, capacity=1)):
            assert o.tobytes() == want_o.tobytes() and r.tobytes() == want_r.tobytes()
        assert scene.overlap(d, count_only=True).tobytes() == want_o.tobytes()
        uo, ur = scene.overlap(d, sorted=False)
        check_scene_overlap(uo, ur, ref, False, "binding, unsorted")
        d.free()
        with pytest.raises(pkg.BvhError):
            scene.overlap(np.zeros((4, 5), dtype=F32))
        with pytest.raises(pkg.BvhError):
            scene.overlap(4096)                                           # a device address without n_boxes
        eo, er = scene.overlap(boxes[:0])
        assert eo.tolist() == [0] and len(er) == 0 and er.dtype == pkg.INSTANCE_PRIM and scene.overlap(boxes[:0], count_only=True).tolist() == [0]
        scene.close()
    finally:
        bl.close(); sc_ctx.close()
