"""bvh_scene_radius_search on the GPU: every triangle of every active instance within each query's radius against the two-level numpy brute force
(tests/test_scene_radius.py, which also makes the inputs and checks their premises without a device): sorted, unsorted and count-only calls for 1 to 64
instances over BLASes of every builder and triangle format, the sorted prefix against bvh_scene_knn, one identity instance against bvh_radius_search,
coincident instances, independence from the builders, sheared and far-offset instances, deep BLASes through the stackless pass, bvh_scene_update after moves
and after a BLAS refit, the passes and the capacity decision, rejections and buffer hygiene, the binding's input kinds."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_scene import TLAS_ALGO, Blases, root_boxes, world_tris
from test_gpu_scene_knn import same_root_boxes
from test_query import E_INVALID
from test_radius import slice_queries
from test_scene_point import scene_points
from test_scene_radius import (QUERY_STACK, RADIUS_SORTED, check_scene_radius, mixed_wave, radius_builders_inputs, radius_coincident_inputs,
                               radius_deep_inputs, radius_exact_inputs, radius_kinds_inputs, radius_moved_inputs, radius_small_inputs, radius_sponza_inputs,
                               scene_host_sort, scene_radius_brute_force, scene_radius_needs)
from test_scene_knn import inactive_of

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]


def call(pkg, scene, d_points, m, flags, d_offsets, d_hits, capacity, total=True):
    t = C.c_uint64(0xDEAD)
    rc = pkg.lib().bvh_scene_radius_search(scene.handle, d_points, m, flags, d_offsets, d_hits, capacity, C.byref(t) if total else None)
    return rc, t.value


def search(pkg, scene, pts, flags):
    """count-only call, then a fill with the exact capacity; returns (offsets, hits).  The count-only offsets must equal the fill's."""
    ctx, m = scene.ctx, len(pts)
    d_pts, d_off = ctx.upload(pts), ctx.alloc((m + 1) * 4)
    hits = None
    try:
        rc, total = call(pkg, scene, d_pts.ptr, m, flags, d_off.ptr, None, 0)
        assert rc == 0, rc
        counted = d_off.download(np.uint32, m + 1)
        assert counted[0] == 0 and counted[-1] == total
        hits = ctx.alloc(max(total, 1) * 16)
        rc, total2 = call(pkg, scene, d_pts.ptr, m, flags, d_off.ptr, hits.ptr, total)
        assert rc == 0 and total2 == total
        off = d_off.download(np.uint32, m + 1)
        assert off.tobytes() == counted.tobytes(), "count-only and fill calls disagree on the offsets"
        return off, hits.download(pkg.INSTANCE_KNN_HIT, total)
    finally:
        d_pts.free(); d_off.free()
        if hits is not None:
            hits.free()


def check_all_ways(pkg, scene, pts, blas_tris, inst, ref, what):
    """the sorted fill against the brute force; the unsorted fill set-equal to the sorted one on every query and byte-equal to itself when called twice; the
    count-only offsets equal to the fill's (search asserts it).  Returns the sorted answer"""
    off, hits = search(pkg, scene, pts, RADIUS_SORTED)
    check_scene_radius(pkg, pts, blas_tris, inst, ref, off, hits, True, what + " sorted")
    uoff, uhits = search(pkg, scene, pts, 0)
    assert uoff.tobytes() == off.tobytes(), f"{what}: sorted and unsorted calls count differently"
    assert scene_host_sort(uoff, uhits).tobytes() == hits.tobytes(), f"{what}: the unsorted slices are not the sorted ones as sets"
    uoff2, uhits2 = search(pkg, scene, pts, 0)
    assert uoff2.tobytes() == uoff.tobytes() and uhits2.tobytes() == uhits.tobytes(), f"{what}: the same unsorted call twice gives other bytes"
    return off, hits


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_inst", [1, 2, 3, 64])
def test_exact_against_brute_force(pkg, n_inst):
    """1: no top-level tree; 2: a root with two leaf children; 3: the singular instance inactive; 64: all three kinds of inactive instance"""
    meshes, inst, pts, ref = radius_exact_inputs(pkg, n_inst)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo], fmt=algo % 3) for algo in range(4)]
        same_root_boxes(pkg, blases, meshes)
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[n_inst], blases, inst)
        off, hits = check_all_ways(pkg, scene, pts, meshes, inst, ref, f"{n_inst} instances")
        assert not set(hits["instance"].tolist()) & inactive_of(n_inst), "an inactive instance answered"
        poff, phits = scene.radius_search(pts)                            # the Python binding, host points
        assert poff.tobytes() == off.tobytes() and phits.tobytes() == hits.tobytes()
        assert scene.radius_search(pts, count_only=True).tobytes() == off.tobytes()
        if n_inst == 3:                                               # 65 points: a partial last wave
            _, _, pts65, ref65 = radius_exact_inputs(pkg, 3, m=65)
            check_all_ways(pkg, scene, pts65, meshes, inst, ref65, "65 points")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("kind", ["shear", "far"])
def test_anisotropic_and_far_offset_instances(pkg, kind):
    mesh, inst, pts, ref = radius_kinds_inputs(pkg, kind)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        same_root_boxes(pkg, [b], [mesh])
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        check_all_ways(pkg, scene, pts, [mesh], inst, ref, kind)
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_sorted_prefix_equals_scene_knn(pkg):
    meshes, inst, pts, ref = radius_exact_inputs(pkg, 64)
    well = ref["well"]
    assert well.mean() >= 0.99
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo], fmt=algo % 3) for algo in range(4)]
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[64], blases, inst)
        off, hits = scene.radius_search(pts)
        o = off.astype(np.int64)
        lens = np.diff(o)
        assert (lens > 32).sum() > 50 and (lens == 0).sum() > 50
        for k in (1, 8, 32):
            lists, counts = scene.knn(pts, k)
            want = np.minimum(lens, k)
            assert np.array_equal(counts[well], want[well]), f"k = {k}: counts differ from min(k, slice length)"
            for i in np.nonzero(well)[0]:
                assert hits[o[i]: o[i] + want[i]].tobytes() == lists[i, : want[i]].tobytes(), f"k = {k}, query {i}: the sorted prefix is not bvh_scene_knn's list"
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("algo", [1, 3])
def test_one_identity_instance_equals_radius_search(pkg, algo):
    mesh, inst, pts, ref, flat_well = radius_sponza_inputs(pkg)
    both = ref["well"] & flat_well                                    # well-conditioned for both queries
    assert both.mean() >= 0.99
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(algo, mesh)
        assert b.result.layout == (0 if algo == 1 else 1)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        for sorted_ in (True, False):
            foff, fhits = b.radius_search(pts, sorted=sorted_)
            off, hits = scene.radius_search(pts, sorted=sorted_)
            assert len(hits) > 1000 and (hits["instance"] == 0).all() and (hits["reserved"] == 0).all()
            assert np.array_equal(np.diff(off.astype(np.int64))[both], np.diff(foff.astype(np.int64))[both]), f"sorted {sorted_}: the counts differ from bvh_radius_search's"
            if not sorted_:
                hits = scene_host_sort(off, hits)
                fhits = fhits[np.lexsort((fhits["prim"], np.ascontiguousarray(fhits["dist2"]).view(np.uint32), slice_queries(foff)))]
            mine, theirs = hits[both[slice_queries(off)]], fhits[both[slice_queries(foff)]]
            assert mine["dist2"].tobytes() == theirs["dist2"].tobytes() and np.array_equal(mine["prim"], theirs["prim"]), f"sorted {sorted_}"
        check_all_ways(pkg, scene, pts, [mesh], inst, ref, f"sponza, algo {algo}")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("tlas_algo", [0, 3])
def test_coincident_instances_interleave(pkg, tlas_algo):
    """two instances place the same triangles identically, so every record comes twice; one BLAS also holds a far-off extra triangle that stretches its world
    box, so the two are not walked alike.  Every sorted slice is (d, 0, p), (d, 1, p), ... whichever BLAS is the stretched one."""
    mesh, stretched, inst, pts = radius_coincident_inputs(pkg, tlas_algo)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        plain, far = bl.add(3, mesh), bl.add(1, stretched)
        for order in ((plain, far), (far, plain)):
            blas_tris = [mesh, stretched] if order[0] is plain else [stretched, mesh]
            ref = scene_radius_brute_force(pkg, pts, blas_tris, inst, root_boxes(pkg, list(order)))
            assert ref["well"].all()
            scene = pkg.Scene(sc_ctx).build(tlas_algo, list(order), inst)
            off, hits = check_all_ways(pkg, scene, pts, blas_tris, inst, ref, "coincident")
            assert off.tobytes() == ref["offsets"].tobytes() and hits.tobytes() == ref["hits"].tobytes()
            q = slice_queries(off)
            pair = (q[1:] == q[:-1]) & (hits["dist2"][1:] == hits["dist2"][:-1]) & (hits["prim"][1:] == hits["prim"][:-1])
            assert pair.sum() > 1000 and (hits["instance"][:-1][pair] == 0).all() and (hits["instance"][1:][pair] == 1).all(), "a tie went to the higher instance first"
            scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- independence, depth and updates ----------------------------------------------------------------------------------------------------------------------------

def test_independent_of_builders(pkg):
    mesh, inst, pts, ref, _ = radius_builders_inputs(pkg)
    assert ref["well"].all()
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, mesh) for algo in range(4)]
        same_root_boxes(pkg, blases, [mesh] * 4)
        outs = []
        for tl in range(4):                                       # top-level builders over the same BLAS
            outs.append((f"top-level builder {tl}", pkg.Scene(sc_ctx).build(tl, [blases[3]], inst).radius_search(pts)))
        for b in range(3):                                        # BLAS builders of the same mesh
            outs.append((f"BLAS builder {b}", pkg.Scene(sc_ctx).build(3, [blases[b]], inst).radius_search(pts)))
        for what, (off, hits) in outs:
            assert off.tobytes() == ref["offsets"].tobytes() and hits.tobytes() == ref["hits"].tobytes(), what
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("H", [70, 250])
def test_deep_blas_takes_the_stackless_pass(pkg, H):
    tris, nodes, left, root, n, inst, pts, ref = radius_deep_inputs(pkg, H)
    lower, upper = scene_radius_needs(left, root, n, inst, pts)
    assert (lower > QUERY_STACK).sum() >= 64 and (upper <= QUERY_STACK).sum() >= 64 and mixed_wave(lower, upper), "no wave mixes overflowing and quiet queries"
    assert ref["well"].all()
    c, sc_ctx = pkg.Context(0), pkg.Context(0)
    try:
        d_tris = c.upload(tris)
        for label, arr in (("chain left", left), ("as made", nodes)):
            d_nodes = c.upload(arr)
            r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
            scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
            sc_ctx.set_profiling(2)
            off, hits = search(pkg, scene, pts, RADIUS_SORTED)            # (asserts that the count-only and the fill call agree)
            kt = sc_ctx.kernel_times()
            sc_ctx.set_profiling(0)
            assert {"k_scene_radius_count", "k_scene_radius_fill", "k_scene_radius_deep", "k_overlap_scan"} <= set(kt), sorted(kt)
            launches = {k: v[1] for k, v in kt.items()}                   # (search: a count-only call, then a call that counts and fills)
            assert launches["k_scene_radius_count"] == 2 and launches["k_scene_radius_fill"] == 1 and launches["k_overlap_scan"] == 2, launches
            assert launches["k_scene_radius_deep"] == 3, "k_scene_radius_deep does not follow every pass"
            assert off.tobytes() == ref["offsets"].tobytes() and hits.tobytes() == ref["hits"].tobytes(), f"H {H} {label}"
            uoff, uhits = search(pkg, scene, pts, 0)
            assert uoff.tobytes() == off.tobytes() and scene_host_sort(uoff, uhits).tobytes() == hits.tobytes(), f"H {H} {label} unsorted"
            assert scene.radius_search(pts, count_only=True).tobytes() == off.tobytes()
            scene.close(); d_nodes.free()
        d_tris.free()
    finally:
        sc_ctx.close(); c.close()


def test_deep_kernel_is_launched_after_both_passes(pkg):
    """bvh_ctx_kernel_times keeps one entry per name: a count-only call reports k_scene_radius_deep without a fill, a filling call reports the fill as well"""
    tris, nodes, left, root, n, inst, pts, ref = radius_deep_inputs(pkg, 70)
    c, sc_ctx = pkg.Context(0), pkg.Context(0)
    try:
        d_tris, d_nodes = c.upload(tris), c.upload(left)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
        sc_ctx.set_profiling(2)
        off = scene.radius_search(pts, count_only=True)
        kt = sc_ctx.kernel_times()
        counted = set(kt)
        sc_ctx.set_profiling(0)
        assert {"k_scene_radius_count", "k_scene_radius_deep", "k_overlap_scan"} <= counted and "k_scene_radius_fill" not in counted, sorted(counted)
        assert kt["k_scene_radius_count"][1] == 1 and kt["k_scene_radius_deep"][1] == 1
        assert off.tobytes() == ref["offsets"].tobytes()
        scene.close(); d_nodes.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()


def test_update_after_moves_and_blas_refit(pkg):
    meshes, inst, moved, pts, refit, ref_moved, ref_refit = radius_moved_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        scene.radius_search(pts, count_only=True)
        scene.update(moved)
        same_root_boxes(pkg, blases, meshes)
        off, hits = check_all_ways(pkg, scene, pts, meshes, moved, ref_moved, "after update")
        foff, fhits = pkg.Scene(sc_ctx).build(3, blases, moved).radius_search(pts)
        assert foff.tobytes() == off.tobytes() and fhits.tobytes() == hits.tobytes(), "an updated and a freshly built scene differ"
        blases[0].refit(refit[0])
        bl.ctxs[0].synchronize()                                  # (the refit ran on the BLAS's own stream: complete before the scene reads the root box)
        scene.update(moved)
        same_root_boxes(pkg, blases, refit)
        check_all_ways(pkg, scene, pts, refit, moved, ref_refit, "after BLAS refit")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- passes, capacity, argument handling and memory hygiene -------------------------------------------------------------------------------------------------------

def small_scene(pkg, bl):
    mesh, inst, pts, ref = radius_small_inputs(pkg)
    return mesh, bl.add(3, mesh), inst, pts, ref


def test_passes_and_capacity(pkg):
    bl, ctx = Blases(pkg), pkg.Context(0)
    try:
        mesh, b, inst, pts, ref = small_scene(pkg, bl)
        scene = pkg.Scene(ctx).build(2, [b], inst)
        m = len(pts)
        want = {flags: search(pkg, scene, pts, flags) for flags in (RADIUS_SORTED, 0)}
        exp_off = want[0][0]
        total = int(exp_off[-1])
        assert total > 100 and want[RADIUS_SORTED][0].tobytes() == exp_off.tobytes()
        check_scene_radius(pkg, pts, [mesh], inst, ref, exp_off, want[RADIUS_SORTED][1], True, "small scene")
        extra = 29
        guard_h = np.frombuffer(np.full((total + extra) * 16, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_KNN_HIT)
        guard_o = np.full(m + 1 + extra, 0xA5A5A5A5, dtype=np.uint32)
        d_pts, d_off, d_hits = ctx.upload(pts), ctx.upload(guard_o), ctx.upload(guard_h)
        for flags in (RADIUS_SORTED, 0):
            out = {}
            # count only: d_hits untouched, offsets complete, guard words past n_points + 1 offsets intact
            d_off.upload(guard_o); d_hits.upload(guard_h)
            assert call(pkg, scene, d_pts.ptr, m, flags, d_off.ptr, None, 0) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_hits.download(pkg.INSTANCE_KNN_HIT, total + extra).tobytes() == guard_h.tobytes()
            # capacity total - 1: the fill is skipped, d_offsets still complete, *total_out set
            d_off.upload(guard_o)
            assert call(pkg, scene, d_pts.ptr, m, flags, d_off.ptr, d_hits.ptr, total - 1) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_hits.download(pkg.INSTANCE_KNN_HIT, total + extra).tobytes() == guard_h.tobytes()
            # the exact capacity is filled; guard records past the total intact; twice the same bytes
            for rnd in range(2):
                d_off.upload(guard_o); d_hits.upload(guard_h)
                assert call(pkg, scene, d_pts.ptr, m, flags, d_off.ptr, d_hits.ptr, total) == (0, total)
                o, h = d_off.download(np.uint32, m + 1 + extra), d_hits.download(pkg.INSTANCE_KNN_HIT, total + extra)
                assert o[m + 1:].tobytes() == guard_o[m + 1:].tobytes() and h[total:].tobytes() == guard_h[total:].tobytes()
                assert o[: m + 1].tobytes() == exp_off.tobytes() and h[:total].tobytes() == want[flags][1].tobytes()
                out[rnd] = (o.tobytes(), h.tobytes())
            assert out[0] == out[1], "two identical calls give different bytes"
            # total_out == NULL: the same device bytes after a synchronize
            d_off.upload(guard_o); d_hits.upload(guard_h)
            rc, t = call(pkg, scene, d_pts.ptr, m, flags, d_off.ptr, d_hits.ptr, total + extra, total=False)
            assert rc == 0 and t == 0xDEAD
            ctx.synchronize()
            assert (d_off.download(np.uint32, m + 1 + extra).tobytes(), d_hits.download(pkg.INSTANCE_KNN_HIT, total + extra).tobytes()) == out[0]
            assert d_pts.download(pkg.POINT_QUERY, m).tobytes() == pts.tobytes()
        # n_points == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        d_off.upload(guard_o); d_hits.upload(guard_h)
        assert call(pkg, scene, d_pts.ptr, 0, RADIUS_SORTED, d_off.ptr, d_hits.ptr, total) == (0, 0)
        o = d_off.download(np.uint32, m + 1 + extra)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes() and d_hits.download(pkg.INSTANCE_KNN_HIT, total + extra).tobytes() == guard_h.tobytes()
        # the binding's capacity protocol: a capacity that is too small is re-allocated from the reported total
        qoff, qhits = scene.radius_search(pts, sorted=False, capacity=3)
        assert qoff.tobytes() == exp_off.tobytes() and qhits.tobytes() == want[0][1].tobytes()
        scene.close(); d_pts.free(); d_off.free(); d_hits.free()
    finally:
        bl.close(); ctx.close()


def test_errors_write_nothing(pkg):
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    L = pkg.lib()
    try:
        mesh, b, inst, pts, ref = small_scene(pkg, bl)
        m = len(pts)
        d_pts = sc_ctx.upload(pts)
        cap = int(ref["offsets"][-1]) + 64
        guard_h = np.frombuffer(np.full(cap * 16, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_KNN_HIT)
        guard_o = np.full(m + 1, 0x5A5A5A5A, dtype=np.uint32)
        hits, offs = sc_ctx.upload(guard_h), sc_ctx.upload(guard_o)
        tot = C.c_uint64(0x77)
        unbuilt, scene = pkg.Scene(sc_ctx), pkg.Scene(sc_ctx).build(2, [b], inst)

        def go(sc=scene, p=d_pts.ptr, n=m, flags=RADIUS_SORTED, o=offs.ptr, h=hits.ptr, k=cap):
            return L.bvh_scene_radius_search(sc.handle if sc is not None else None, p, n, flags, o, h, k, C.byref(tot))
        cases = {
            "null scene": go(sc=None), "unbuilt scene": go(sc=unbuilt), "null points": go(p=None), "null offsets": go(o=None),
            "flag 2": go(flags=2), "flag 3": go(flags=3), "flag high": go(flags=0x80000000),
            "n_points 2^30": go(n=1 << 30),
            "offsets in points": go(o=d_pts.ptr + 32), "hits in points": go(h=d_pts.ptr + 16), "hits in offsets": go(h=offs.ptr + 16),
            "offsets in hits": go(o=hits.ptr + 16 * (cap - 1)), "points in hits": go(p=hits.ptr, h=hits.ptr + 16 * 8),
            "hits over the points, capacity clamped": go(h=d_pts.ptr - 16, k=1 << 40),
            "unbuilt, n_points 0": go(sc=unbuilt, n=0),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        assert tot.value == 0x77
        sc_ctx.synchronize()
        assert hits.download(pkg.INSTANCE_KNN_HIT, cap).tobytes() == guard_h.tobytes() and offs.download(np.uint32, m + 1).tobytes() == guard_o.tobytes()
        assert d_pts.download(pkg.POINT_QUERY, m).tobytes() == pts.tobytes()
        # a count-only call ignores the capacity's range, and the scene still answers
        assert go(h=None, k=1 << 40) == 0 and tot.value == ref["offsets"][-1]
        total = tot.value
        assert offs.download(np.uint32, m + 1)[-1] == total and hits.download(pkg.INSTANCE_KNN_HIT, cap).tobytes() == guard_h.tobytes()
        assert go() == 0 and tot.value == total
        got = hits.download(pkg.INSTANCE_KNN_HIT, cap)
        assert got[total:].tobytes() == guard_h[total:].tobytes()
        check_scene_radius(pkg, pts, [mesh], inst, ref, offs.download(np.uint32, m + 1), got[:total], True, "after the errors")
        scene.close(); unbuilt.close(); d_pts.free(); hits.free(); offs.free()
    finally:
        bl.close(); sc_ctx.close()


def test_dead_zero_and_infinite_radii_and_inactive_instances(pkg):
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        mesh, b, inst, pts, ref = small_scene(pkg, bl)
        scene = pkg.Scene(sc_ctx).build(2, [b], inst)
        off, hits = check_all_ways(pkg, scene, pts, [mesh], inst, ref, "small scene")
        lens = np.diff(off.astype(np.int64))
        with np.errstate(invalid="ignore"):
            dead = np.isnan(pts["point"]).any(axis=1) | np.isnan(pts["radius"]) | (pts["radius"] < 0)
        assert dead.sum() == 6 and (lens[dead] == 0).all(), "a dead query has records"
        zero = ~dead & (pts["radius"] == 0)
        assert zero.sum() == 2 and (hits["dist2"][np.isin(slice_queries(off), np.nonzero(zero)[0])] == 0).all()
        unbounded = ~dead & np.isinf(pts["radius"])
        assert unbounded.sum() > 100 and (lens[unbounded] == 2 * len(mesh)).all(), "an infinite radius takes every triangle of both instances"
        # an inactive instance (singular, NaN, a BLAS out of range) never answers: the answer is the other instance's alone
        for what, edit in (("singular", lambda i: i["object_to_world"].__setitem__(1, 0.0)), ("NaN", lambda i: i["object_to_world"][1].__setitem__(5, np.nan)),
                           ("no BLAS", lambda i: i["blas"].__setitem__(1, 7))):
            off_inst = inst.copy(); edit(off_inst)
            scene.update(off_inst)
            ref1 = scene_radius_brute_force(pkg, pts, [mesh], off_inst)
            o1, h1 = check_all_ways(pkg, scene, pts, [mesh], off_inst, ref1, what)
            assert len(h1) > 100 and (h1["instance"] == 0).all(), what
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_binding_takes_every_input_kind(pkg):
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        mesh, b, inst, _, _ = small_scene(pkg, bl)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        xyz = np.ascontiguousarray(scene_points(pkg, world_tris(pkg, [mesh], inst), 256, 4, bounded=False)["point"])
        rec = np.zeros(256, dtype=pkg.POINT_QUERY); rec["point"] = xyz; rec["radius"] = 0.5
        want_o, want_h = scene.radius_search(rec)
        assert want_o.shape == (257,) and want_o.dtype == np.uint32 and want_h.dtype == pkg.INSTANCE_KNN_HIT and len(want_h) == want_o[-1] > 100
        check_scene_radius(pkg, rec, [mesh], inst, scene_radius_brute_force(pkg, rec, [mesh], inst), want_o, want_h, True, "binding")
        d = sc_ctx.upload(rec)
        for o, h in (scene.radius_search(xyz, radius=0.5), scene.radius_search(d), scene.radius_search(d.ptr, n_points=256),
                     scene.radius_search(rec, capacity=len(want_h) + 5), scene.radius_search(rec, capacity=1)):
            assert o.tobytes() == want_o.tobytes() and h.tobytes() == want_h.tobytes()
        assert scene.radius_search(d, count_only=True).tobytes() == want_o.tobytes()
        uo, uh = scene.radius_search(d, sorted=False)
        assert uo.tobytes() == want_o.tobytes() and scene_host_sort(uo, uh).tobytes() == want_h.tobytes()
        d.free()
        with pytest.raises(pkg.BvhError):
            scene.radius_search(rec, radius=1.0)
        with pytest.raises(pkg.BvhError):
            scene.radius_search(4096)                                 # a device address without n_points
        eo, eh = scene.radius_search(rec[:0])
        assert eo.tolist() == [0] and len(eh) == 0 and eh.dtype == pkg.INSTANCE_KNN_HIT and scene.radius_search(rec[:0], count_only=True).tolist() == [0]
        uo, uh = scene.radius_search(xyz)                             # radius None: unbounded, every triangle of both instances
        assert (np.diff(uo.astype(np.int64)) == 2 * len(mesh)).all()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()
