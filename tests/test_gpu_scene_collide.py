"""bvh_scene_collide on the GPU: the crossing triangle pairs of all instances at once, against the numpy brute force (tests/test_scene_collide.py, which also
makes the inputs and checks their premises without a device) on EVERY row — row_first, offsets and whole sets, sorted bytes included; the unsorted slices
equal the sorted ones as sets and the same call twice gives the same bytes.  Default and BVH_SCENE_COLLIDE_BOTH for 1 to 8 instances over BLASes of every
builder, layout and format; 64 instances against the GPU's own bvh_scene_intersect_tris(BVH_SCENE_TRIS_INSTANCE, k) for every k, byte for byte, with the three
relations of the header; coincident instances; a deep BLAS through the stackless pass, with a short-tree control; bvh_scene_update from device memory (moves,
another BLAS for an instance) and a BLAS refit; the passes, the capacity and the row-capacity decisions; asynchrony; rejections and buffer hygiene; the binding."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_scene import TLAS_ALGO, Blases
from test_gpu_scene_intersect_tris import four_blases
from test_query import E_INVALID
from test_scene_collide import (E_TOO_LARGE, QUERY_STACK, SCENE_COLLIDE_BOTH, SCENE_COLLIDE_SORTED, check_scene_collide, collide_answer, collide_coincident_inputs,
                                collide_deep_inputs, collide_exact_inputs, collide_kinds_inputs, collide_moved_inputs, scene_collide_full)
from test_scene_intersect_tris import tris_exact_inputs, tris_instance_inputs, tris_small_inputs
from test_scene_knn import inactive_of
from test_scene_overlap import scene_host_sort, slice_queries

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32


def call(pkg, scene, flags, d_first, row_capacity, d_offsets, d_prims, capacity, rows=True, total=True):
    r, t = C.c_uint64(0xBEEF), C.c_uint64(0xDEAD)
    rc = pkg.lib().bvh_scene_collide(scene.handle, flags, d_first, row_capacity, d_offsets, d_prims, capacity, C.byref(r) if rows else None, C.byref(t) if total else None)
    return rc, r.value, t.value


def search(pkg, scene, flags, row_capacity):
    """a count-only call, then a fill with the exact capacity; returns (row_first, offsets, records).  Both calls must give the same table and offsets"""
    ctx, n_inst = scene.ctx, scene.n_instances
    d_first, d_off, prims = ctx.alloc((n_inst + 1) * 4), ctx.alloc((row_capacity + 1) * 4), None
    try:
        rc, n_rows, total = call(pkg, scene, flags, d_first.ptr, row_capacity, d_off.ptr, None, 0)
        assert rc == 0, rc
        first, counted = d_first.download(np.uint32, n_inst + 1), d_off.download(np.uint32, row_capacity + 1)
        assert first[-1] == n_rows <= row_capacity and counted[0] == 0 and counted[-1] == total
        prims = ctx.alloc(max(total, 1) * 8)
        rc, n_rows2, total2 = call(pkg, scene, flags, d_first.ptr, row_capacity, d_off.ptr, prims.ptr, total)
        assert rc == 0 and (n_rows2, total2) == (n_rows, total)
        off = d_off.download(np.uint32, row_capacity + 1)
        assert off.tobytes() == counted.tobytes(), "count-only and fill calls disagree on the offsets"
        assert d_first.download(np.uint32, n_inst + 1).tobytes() == first.tobytes()
        return first, off, prims.download(pkg.INSTANCE_PRIM, total)
    finally:
        d_first.free(); d_off.free()
        if prims is not None:
            prims.free()


def check_all_ways(pkg, scene, full, what, pads=(0, 37)):
    """default and BOTH; row_capacity = n_rows and n_rows + pad (the trailing rows empty, a partial last wave, d_offsets[row_capacity] the total): the sorted
    fill against the brute force on every row; the unsorted fill set-equal to the sorted one and byte-equal to itself when called twice; the count-only
    offsets equal to the fill's (search asserts it).  Returns {both: the sorted answer at row_capacity = n_rows}"""
    n_rows, out = int(full["row_first"][-1]), {}
    for both in (False, True):
        ref, bit = collide_answer(full, both), SCENE_COLLIDE_BOTH if both else 0
        for pad in pads:
            w = f"{what}, {'both' if both else 'default'}, row_capacity n_rows + {pad}"
            first, off, recs = search(pkg, scene, bit | SCENE_COLLIDE_SORTED, n_rows + pad)
            assert len(off) == n_rows + pad + 1 and off[-1] == len(recs)
            check_scene_collide(first, off, recs, ref, both, True, w + " sorted")
            ufirst, uoff, urecs = search(pkg, scene, bit, n_rows + pad)
            check_scene_collide(ufirst, uoff, urecs, ref, both, False, w + " unsorted")
            assert scene_host_sort(uoff, urecs).tobytes() == recs.tobytes(), f"{w}: the unsorted slices are not the sorted ones as sets"
            if pad == 0:
                _, uoff2, urecs2 = search(pkg, scene, bit, n_rows)
                assert uoff2.tobytes() == uoff.tobytes() and urecs2.tobytes() == urecs.tobytes(), f"{w}: the same unsorted call twice gives other bytes"
                out[both] = (first, off, recs)
    return out


# ---- whole sets against the brute force -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_inst", [1, 2, 3])
def test_exact_on_every_row(pkg, n_inst):
    """1: no top-level tree, n_rows = n and every row empty; 2: a root with two leaf children; 3: the singular instance inactive, without rows.  The four
    BLASes come from the four builders (layouts 0 and 1, all three formats), under two top-level builders"""
    meshes, inst, full = collide_exact_inputs(pkg, n_inst)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = four_blases(pkg, bl, meshes)
        for tlas in (TLAS_ALGO[n_inst], (TLAS_ALGO[n_inst] + 2) % 4):
            scene = pkg.Scene(sc_ctx).build(tlas, blases, inst)
            got = check_all_ways(pkg, scene, full, f"{n_inst} instances, top-level builder {tlas}")
            first, off, recs = got[True]
            assert not set(recs["instance"].tolist()) & inactive_of(n_inst), "an inactive instance answered"
            if n_inst == 1:
                assert first.tolist() == [0, len(meshes[0])] and not off.any() and len(recs) == 0
            scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("kind", ["shear", "mirror", "far"])
def test_sheared_mirrored_and_far_offset_instances(pkg, kind):
    """eight instances of one mesh; the BLAS from each of the four builders in turn, the top level from two"""
    mesh, inst, full = collide_kinds_inputs(pkg, kind)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        for algo in range(4):
            scene = pkg.Scene(sc_ctx).build(3 if algo % 2 else 0, [bl.add(algo, mesh, fmt=algo % 3)], inst)
            check_all_ways(pkg, scene, full, f"{kind}, BLAS builder {algo}", pads=(0, 37) if algo == 3 else (0,))
            scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_64_instances_equal_the_instance_calls_row_for_row(pkg):
    """SORTED | BOTH: the rows of instance k are the first n_leaves slices of bvh_scene_intersect_tris(INSTANCE, k, SORTED), byte for byte, for every k;
    instance 3 also against the brute force; the default answer is the BOTH answer filtered to instance > k, half its total; the rows are symmetric"""
    meshes, inst, _, _ = tris_exact_inputs(pkg, 64)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        scene = pkg.Scene(sc_ctx).build(2, four_blases(pkg, bl, meshes), inst)
        want_first = np.zeros(65, dtype=np.int64)
        for k in range(64):
            want_first[k + 1] = want_first[k] + (0 if k in inactive_of(64) else len(meshes[k % 4]))
        n_rows = int(want_first[-1])
        assert n_rows == 44770
        first, off, recs = search(pkg, scene, SCENE_COLLIDE_SORTED | SCENE_COLLIDE_BOTH, n_rows)
        assert first.tolist() == want_first.tolist() and first[61] == first[62] == first[63] == first[64], "row_first"
        o = off.astype(np.int64)
        for k in range(64):
            ioff, irecs = scene.intersect_tris(instance=k)                # (1 280 rows: as many as the largest BLAS has leaves)
            lo, hi = int(first[k]), int(first[k + 1])
            if k in inactive_of(64):
                assert lo == hi and not ioff.any()
                continue
            n = hi - lo
            assert (o[lo:hi + 1] - o[lo]).tolist() == ioff[: n + 1].astype(np.int64).tolist(), f"instance {k}: offsets"
            assert ioff[n] == ioff[-1] and recs[o[lo]:o[hi]].tobytes() == irecs.tobytes(), f"instance {k}: records"
        _, _, _, iref = tris_instance_inputs(pkg, 64, 3)                  # the brute force of INSTANCE(3), 1 280 rows of which the BLAS has 256
        lo, hi = int(first[3]), int(first[4])
        assert hi - lo == 256 and (o[lo:hi + 1] - o[lo]).tolist() == iref["offsets"][:257].astype(np.int64).tolist()
        assert recs[o[lo]:o[hi]].tobytes() == iref["recs"].tobytes() and len(iref["recs"]) > 0
        # the three relations
        own = (np.searchsorted(want_first, slice_queries(off), side="right") - 1).astype(np.int64)
        assert (recs["instance"].astype(np.int64) != own).all() and not set(recs["instance"].tolist()) & inactive_of(64)
        keep = recs["instance"].astype(np.int64) > own
        dfirst, doff, drecs = search(pkg, scene, SCENE_COLLIDE_SORTED, n_rows)
        want_off = np.zeros(n_rows + 1, dtype=np.uint32); want_off[1:] = np.cumsum(np.bincount(slice_queries(off)[keep], minlength=n_rows))
        assert dfirst.tobytes() == first.tobytes() and doff.tobytes() == want_off.tobytes() and drecs.tobytes() == recs[keep].tobytes()
        assert len(recs) == 2 * len(drecs) == 174924
        row = slice_queries(off)
        i = row - want_first[own]
        fwd = set(zip(own.tolist(), i.tolist(), recs["instance"].tolist(), recs["prim"].tolist()))
        back = set(zip(recs["instance"].tolist(), recs["prim"].tolist(), own.tolist(), i.tolist()))
        assert fwd == back and len(fwd) == len(recs), "the rows are not symmetric"
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("tlas_algo", [0, 3])
def test_coincident_instances(pkg, tlas_algo):
    """two identities place the same triangles identically (one BLAS also holds a far-off triangle that stretches its world box): the identical, coplanar
    copies are never reported, the mesh's own crossings appear across the two instances"""
    mesh, stretched, inst = collide_coincident_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        plain, far = bl.add(3, mesh), bl.add(1, stretched)
        for order in ((plain, far), (far, plain)):
            blas_tris = [mesh, stretched] if order[0] is plain else [stretched, mesh]
            full = scene_collide_full(blas_tris, inst)
            scene = pkg.Scene(sc_ctx).build(tlas_algo, list(order), inst)
            got = check_all_ways(pkg, scene, full, "coincident", pads=(0,))
            assert len(got[True][2]) == 464 and len(got[False][2]) == 232
            scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- depth and updates ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,deep", [(300, True), (20, False)])
def test_deep_blas_takes_the_stackless_pass(pkg, H, deep):
    """instance 0's slivers run up through the hand-made caterpillar of instance 1: at H = 300 some of its rows need more than the short stack holds inside that
    BLAS, in the count AND in the fill pass; H = 20 is the control on the same code path.  k_scene_collide_deep always re-walks a marked row from the
    top-level plan, so a BLAS-level overflow covers the new code of both kernels — the row lookup, the "may enter" test and the leaf test of the stack walk
    and of the stackless walk.  Top-level overflow DETECTION is k_scene_tris_walk's code unchanged, which tests/test_gpu_scene_intersect_tris.py covers on
    its deep top level, and is not repeated here"""
    slivers, tris, nodes, root, n, inst, full, need = collide_deep_inputs(pkg, H)
    assert bool((need > QUERY_STACK).any()) == deep and (deep or need.max() + len(inst) - 1 <= QUERY_STACK), need.max()
    c, sc_ctx, bl = pkg.Context(0), pkg.Context(0), Blases(pkg)
    try:
        d_tris, d_nodes = c.upload(tris), c.upload(nodes)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        scene = pkg.Scene(sc_ctx).build(3, [bl.add(3, slivers), pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
        n_rows = int(full["row_first"][-1])
        sc_ctx.set_profiling(2)
        first, off, recs = search(pkg, scene, SCENE_COLLIDE_SORTED | SCENE_COLLIDE_BOTH, n_rows)      # (asserts that the count-only and the fill call agree)
        kt = sc_ctx.kernel_times()
        sc_ctx.set_profiling(0)
        assert {"k_scene_collide_rows", "k_scene_collide_count", "k_scene_collide_fill", "k_scene_collide_deep", "k_overlap_scan"} <= set(kt), sorted(kt)
        launches = {k: v[1] for k, v in kt.items()}                       # (search: a count-only call, then a call that counts and fills)
        assert launches["k_scene_collide_rows"] == 2 and launches["k_scene_collide_count"] == 2 and launches["k_scene_collide_fill"] == 1, launches
        assert launches["k_scene_collide_deep"] == 3 and launches["k_overlap_scan"] == 4, launches      # (a scan of the row counts and one of the counts per call)
        check_scene_collide(first, off, recs, collide_answer(full, True), True, True, f"caterpillar {H}")
        check_all_ways(pkg, scene, full, f"caterpillar {H}", pads=(0,))
        scene.close(); d_nodes.free(); d_tris.free()
    finally:
        bl.close(); sc_ctx.close(); c.close()


def test_update_from_device_memory_and_blas_refit(pkg):
    """bvh_scene_update from DEVICE memory moves every instance, then hands instance 4 the other BLAS: the host never learns which BLAS an instance places, and
    d_row_first and the sets follow; then a BLAS refit"""
    meshes, inst, moved, swapped, refit, full_moved, full_swapped, full_refit = collide_moved_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        before = search(pkg, scene, SCENE_COLLIDE_SORTED, int(full_moved["row_first"][-1]))
        d_inst = sc_ctx.upload(moved)
        scene.update((d_inst, len(moved)))
        got = check_all_ways(pkg, scene, full_moved, "after update", pads=(0,))
        assert before[0].tobytes() == got[False][0].tobytes() and before[1].tobytes() != got[False][1].tobytes()
        d_inst.upload(swapped)
        scene.update((d_inst, len(swapped)))
        sw = check_all_ways(pkg, scene, full_swapped, "instance 4 with the other BLAS", pads=(0, 37))
        assert sw[True][0].tobytes() != got[True][0].tobytes()
        first, off, recs = scene.collide(both=True)                      # the binding on device instances: an upper bound on the rows, cut to n_rows
        assert first.tobytes() == sw[True][0].tobytes() and off.tobytes() == sw[True][1].tobytes() and recs.tobytes() == sw[True][2].tobytes()
        d_inst.upload(moved)
        scene.update((d_inst, len(moved)))
        check_all_ways(pkg, scene, full_moved, "instance 4 back", pads=(0,))
        blases[0].refit(refit[0])
        bl.ctxs[0].synchronize()                                          # (the refit ran on the BLAS's own stream: complete before the scene reads the root box)
        scene.update((d_inst, len(moved)))
        check_all_ways(pkg, scene, full_refit, "after BLAS refit", pads=(0,))
        d_inst.free(); scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- passes, capacity, argument handling and memory hygiene -------------------------------------------------------------------------------------------------------

def small_scene(pkg, bl):
    """uniform_256 under an identity and a rotated, shifted instance: 512 rows"""
    mesh, inst, _, _ = tris_small_inputs(pkg)
    return mesh, bl.add(3, mesh), inst, scene_collide_full([mesh], inst)


def test_passes_capacity_and_row_capacity(pkg):
    """the count-only pass, a capacity one record short and zero (the fill is skipped, the offsets complete, d_prims untouched behind its canary), the exact
    capacity (guards intact, the same bytes twice), NULL rows_out and total_out, row_capacity = n_rows - 1 (nothing walked) and 0.  NOT tested, as for the
    siblings whose sink, scan and tail this call shares: the saturation marks, which need more than four thousand million pairs or rows"""
    bl, ctx = Blases(pkg), pkg.Context(0)
    try:
        mesh, b, inst, full = small_scene(pkg, bl)
        scene = pkg.Scene(ctx).build(2, [b], inst)
        n_inst, m = 2, int(full["row_first"][-1])
        assert m == 512
        want = {flags: search(pkg, scene, flags, m) for flags in (SCENE_COLLIDE_SORTED, 0, SCENE_COLLIDE_SORTED | SCENE_COLLIDE_BOTH, SCENE_COLLIDE_BOTH)}
        for flags, (first, off, recs) in want.items():
            both = bool(flags & SCENE_COLLIDE_BOTH)
            check_scene_collide(first, off, recs, collide_answer(full, both), both, bool(flags & SCENE_COLLIDE_SORTED), f"small scene, flags {flags}")
        exp_first = want[0][0]
        extra = 29
        for flags in (SCENE_COLLIDE_SORTED, SCENE_COLLIDE_BOTH):
            exp_off, total = want[flags][1], len(want[flags][2])
            assert total > 50
            guard_p = np.frombuffer(np.full((total + extra) * 8, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_PRIM)
            guard_o, guard_f = np.full(m + 1 + extra, 0xA5A5A5A5, dtype=np.uint32), np.full(n_inst + 1 + extra, 0xA5A5A5A5, dtype=np.uint32)
            d_off, d_prims, d_first = ctx.upload(guard_o), ctx.upload(guard_p), ctx.upload(guard_f)

            def reset():
                d_off.upload(guard_o); d_prims.upload(guard_p); d_first.upload(guard_f)

            def state():
                return d_first.download(np.uint32, n_inst + 1 + extra), d_off.download(np.uint32, m + 1 + extra), d_prims.download(pkg.INSTANCE_PRIM, total + extra)

            def table_and_offsets_complete(f, o, rows=m):
                assert f[: n_inst + 1].tobytes() == exp_first.tobytes() and f[n_inst + 1:].tobytes() == guard_f[n_inst + 1:].tobytes()
                assert o[: rows + 1].tobytes() == exp_off[: rows + 1].tobytes() and o[rows + 1:].tobytes() == guard_o[rows + 1:].tobytes()
            go = lambda prims, cap, rows=True, tot=True, row_cap=m: call(pkg, scene, flags, d_first.ptr, row_cap, d_off.ptr, prims, cap, rows=rows, total=tot)
            # count only, capacity total - 1 and capacity 0: d_prims untouched, table and offsets complete, the guard words behind them intact
            for prims, cap in ((None, 0), (d_prims.ptr, total - 1), (d_prims.ptr, 0)):
                reset()
                assert go(prims, cap) == (0, m, total)
                f, o, p = state()
                table_and_offsets_complete(f, o)
                assert p.tobytes() == guard_p.tobytes()
            # the exact capacity is filled; guard records past the total intact; twice the same bytes
            out = {}
            for rnd in range(2):
                reset()
                assert go(d_prims.ptr, total) == (0, m, total)
                f, o, p = state()
                table_and_offsets_complete(f, o)
                assert p[total:].tobytes() == guard_p[total:].tobytes() and p[:total].tobytes() == want[flags][2].tobytes()
                out[rnd] = (f.tobytes(), o.tobytes(), p.tobytes())
            assert out[0] == out[1], "two identical calls give different bytes"
            # rows_out == NULL and total_out == NULL: the same device bytes after a synchronize, the host words untouched
            reset()
            assert go(d_prims.ptr, total + extra, rows=False, tot=False) == (0, 0xBEEF, 0xDEAD)
            ctx.synchronize()
            assert tuple(x.tobytes() for x in state()) == out[0]
            # row_capacity = n_rows - 1: nothing is walked, every offset 0, d_row_first complete, *rows_out = n_rows, BVH_E_TOO_LARGE, d_prims untouched
            reset()
            assert go(d_prims.ptr, total + extra, row_cap=m - 1) == (E_TOO_LARGE, m, 0)
            f, o, p = state()
            assert f[: n_inst + 1].tobytes() == exp_first.tobytes() and not o[:m].any() and o[m:].tobytes() == guard_o[m:].tobytes() and p.tobytes() == guard_p.tobytes()
            reset()                                                       # ... and without rows_out the host is not told: the device-side caller reads d_row_first
            assert go(d_prims.ptr, total + extra, row_cap=m - 1, rows=False) == (0, 0xBEEF, 0)
            f, o, p = state()
            assert f[n_inst] == m and not o[:m].any() and p.tobytes() == guard_p.tobytes()
            # row_capacity == 0: d_offsets[0] = 0, *total_out = 0, the table all the same
            reset()
            assert go(d_prims.ptr, total, row_cap=0) == (E_TOO_LARGE, m, 0)
            f, o, p = state()
            assert f[: n_inst + 1].tobytes() == exp_first.tobytes() and o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes() and p.tobytes() == guard_p.tobytes()
            reset()
            assert go(None, 0, row_cap=0, rows=False, tot=False) == (0, 0xBEEF, 0xDEAD)
            ctx.synchronize()
            assert state()[0][: n_inst + 1].tobytes() == exp_first.tobytes()
            d_off.free(); d_prims.free(); d_first.free()
        # the binding's capacity protocol: a capacity that is too small is re-allocated from the reported total
        qfirst, qoff, qrecs = scene.collide(sorted=False, capacity=3)
        assert qfirst.tobytes() == exp_first.tobytes() and qoff.tobytes() == want[0][1].tobytes() and qrecs.tobytes() == want[0][2].tobytes()
        scene.close()
    finally:
        bl.close(); ctx.close()


def test_returns_before_the_stream_is_idle(pkg):
    """without rows_out and total_out the call enqueues and returns: a delay in front of it on the ctx's stream is still running when it does
    (tests/test_gpu_streams.py's pattern); with either word it waits, and the answers are the same"""
    import torch
    from test_gpu_streams import MIN_DELAY_MS, Delay, timed
    bl = Blases(pkg)
    s = torch.cuda.Stream()
    ctx = pkg.Context(0, s.cuda_stream)
    try:
        mesh, b, inst, full = small_scene(pkg, bl)
        scene = pkg.Scene(ctx).build(3, [b], inst)
        m, ref = int(full["row_first"][-1]), collide_answer(full, True)
        total = len(ref[2])
        d_first, d_off, d_prims = ctx.alloc(3 * 4), ctx.alloc((m + 1) * 4), ctx.alloc(total * 8)
        go = lambda waits: call(pkg, scene, SCENE_COLLIDE_SORTED | SCENE_COLLIDE_BOTH, d_first.ptr, m, d_off.ptr, d_prims.ptr, total, rows=waits, total=waits)
        step = timed(s, lambda: go(False))
        delay = Delay()
        e0, e1 = delay.put(s, max(MIN_DELAY_MS, 10.0 * step))
        assert go(False) == (0, 0xBEEF, 0xDEAD)
        pending = not e1.query()
        s.synchronize()
        assert e0.elapsed_time(e1) >= 10.0 * step
        assert pending, "declared asynchronous, but the call returned only after the delay in front of it had completed (a hidden host wait)"
        got = (d_first.download(np.uint32, 3), d_off.download(np.uint32, m + 1), d_prims.download(pkg.INSTANCE_PRIM, total))
        check_scene_collide(*got, ref, True, True, "behind a delay")
        e0, e1 = delay.put(s, MIN_DELAY_MS)
        assert go(True) == (0, m, total) and e1.query(), "rows_out and total_out are read back: the call waits for the stream"
        d_first.free(); d_off.free(); d_prims.free(); scene.close()
    finally:
        ctx.close(); bl.close()


def test_one_instance_on_a_fresh_ctx(pkg):
    """a one-instance scene builds no top-level tree, so a fresh ctx has no arena yet: the first call reserves the smallest one"""
    mesh, inst, _, _ = tris_small_inputs(pkg)
    one = inst[1:].copy()
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        scene = pkg.Scene(sc_ctx).build(3, [bl.add(2, mesh)], one)
        first, off, recs = scene.collide(both=True)
        assert first.tolist() == [0, len(mesh)] and len(off) == len(mesh) + 1 and not off.any() and len(recs) == 0
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_errors_write_nothing(pkg):
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    L = pkg.lib()
    try:
        mesh, b, inst, full = small_scene(pkg, bl)
        ref = collide_answer(full, False)
        m, cap = int(ref[0][-1]), len(ref[2]) + 64
        guard_p = np.frombuffer(np.full(cap * 8, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_PRIM)
        guard_o, guard_f = np.full(m + 1, 0x5A5A5A5A, dtype=np.uint32), np.full(3, 0x5A5A5A5A, dtype=np.uint32)
        prims, offs, firsts = sc_ctx.upload(guard_p), sc_ctx.upload(guard_o), sc_ctx.upload(guard_f)
        rows, tot = C.c_uint64(0x55), C.c_uint64(0x77)
        unbuilt, scene = pkg.Scene(sc_ctx), pkg.Scene(sc_ctx).build(2, [b], inst)

        def go(sc=scene, flags=SCENE_COLLIDE_SORTED, f=firsts.ptr, rc=m, o=offs.ptr, h=prims.ptr, c=cap):
            return L.bvh_scene_collide(sc.handle if sc is not None else None, flags, f, rc, o, h, c, C.byref(rows), C.byref(tot))
        cases = {
            "null scene": go(sc=None), "unbuilt scene": go(sc=unbuilt), "null row_first": go(f=None), "null offsets": go(o=None),
            "flag 4": go(flags=4), "flag 7": go(flags=7), "flag high": go(flags=0x80000000),
            "row_capacity 2^30": go(rc=1 << 30), "row_capacity 2^32 - 1": go(rc=0xFFFFFFFF),
            "row_first in offsets": go(f=offs.ptr + 4 * (m - 1)), "offsets in row_first": go(o=firsts.ptr + 8),
            "prims in offsets": go(h=offs.ptr + 16), "offsets in prims": go(o=prims.ptr + 8 * (cap - 1)),
            "row_first in prims": go(f=prims.ptr + 8), "prims in row_first": go(h=firsts.ptr + 4),
            "prims over offsets, capacity clamped": go(h=offs.ptr - 16, c=1 << 40),
            "row_first is offsets": go(f=offs.ptr),
            "unbuilt, row_capacity 0": go(sc=unbuilt, rc=0),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        assert rows.value == 0x55 and tot.value == 0x77
        sc_ctx.synchronize()
        assert prims.download(pkg.INSTANCE_PRIM, cap).tobytes() == guard_p.tobytes() and offs.download(np.uint32, m + 1).tobytes() == guard_o.tobytes()
        assert firsts.download(np.uint32, 3).tobytes() == guard_f.tobytes()
        # a count-only call ignores the capacity's range, and the scene still answers
        assert go(h=None, c=1 << 40) == 0 and (rows.value, tot.value) == (m, len(ref[2]))
        assert prims.download(pkg.INSTANCE_PRIM, cap).tobytes() == guard_p.tobytes()
        assert go() == 0 and (rows.value, tot.value) == (m, len(ref[2]))
        got = prims.download(pkg.INSTANCE_PRIM, cap)
        assert got[len(ref[2]):].tobytes() == guard_p[len(ref[2]):].tobytes()
        check_scene_collide(firsts.download(np.uint32, 3), offs.download(np.uint32, m + 1), got[: len(ref[2])], ref, False, True, "after the errors")
        scene.close(); unbuilt.close(); prims.free(); offs.free(); firsts.free()
    finally:
        bl.close(); sc_ctx.close()


def test_binding_with_host_and_device_instances(pkg):
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        mesh, b, inst, full = small_scene(pkg, bl)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)                     # host instances: the binding computes the rows from them
        for both in (False, True):
            ref = collide_answer(full, both)
            first, off, recs = scene.collide(both=both)
            assert first.dtype == off.dtype == np.uint32 and recs.dtype == pkg.INSTANCE_PRIM and off.shape == (int(first[-1]) + 1,)
            check_scene_collide(first, off, recs, ref, both, True, "binding")
            ufirst, uoff, urecs = scene.collide(both=both, sorted=False)
            check_scene_collide(ufirst, uoff, urecs, ref, both, False, "binding, unsorted")
            cfirst, coff = scene.collide(both=both, count_only=True)
            assert cfirst.tobytes() == first.tobytes() and coff.tobytes() == off.tobytes()
            for o in (scene.collide(both=both, capacity=len(recs) + 5), scene.collide(both=both, capacity=1)):
                assert o[0].tobytes() == first.tobytes() and o[1].tobytes() == off.tobytes() and o[2].tobytes() == recs.tobytes()
            pfirst, poff, precs = scene.collide(both=both, row_capacity=len(off) - 1 + 37)     # a given row_capacity returns all its rows
            assert len(poff) == len(off) + 37 and (poff[len(off) - 1:] == off[-1]).all() and precs.tobytes() == recs.tobytes()
        with pytest.raises(pkg.BvhError):
            scene.collide(row_capacity=int(first[-1]) - 1)
        d_inst = sc_ctx.upload(inst)                                      # device instances: an upper bound on the rows, cut to n_rows
        scene.update((d_inst, len(inst)))
        dfirst, doff, drecs = scene.collide(both=True)
        assert dfirst.tobytes() == first.tobytes() and doff.tobytes() == off.tobytes() and drecs.tobytes() == recs.tobytes()
        d_inst.free(); scene.close()
    finally:
        bl.close(); sc_ctx.close()
