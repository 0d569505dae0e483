"""bvh_scene_cull on the GPU: which triangles' leaf boxes of which active instances pass each world-space convex volume, against the two-level numpy brute
force (pkg.scene_cull_brute_force; tests/test_scene_cull.py makes the inputs and checks their premises without a device) on EVERY volume, through the lane
walk, the group walk and the AUTO rule: 1 to 64 instances over BLASes of every builder, triangle format and layout and over bvh_build_many slices, 1 to 8
planes per volume, coincident instances, one identity instance against bvh_cull, the instances seen against bvh_cull on the top-level tree, the group walk's
bytes against the host restatement of its schedule, bvh_scene_update after moves and after a BLAS refit, the passes and the capacity decision, rejections and
buffer hygiene, a deep BLAS, a deep top level and a full work stack through the stackless pass (the overflow words read back), and the instance ladder of
tests/test_scene_extremes.py."""
import ctypes as C

import numpy as np
import pytest

from test_cull import Tree
from test_deep_trees import QUERY_STACK
from test_gpu_scene import Blases
from test_gpu_scene_knn import same_root_boxes
from test_query import E_INVALID
from test_scene import identity, make_instances
from test_scene_cull import (N_VOLUMES, PLANE_COUNTS, HostScene, check_scene_cull, cull_coincident_inputs, cull_deep_inputs, cull_deep_top_inputs,
                             cull_fat_inputs, cull_moved_inputs, cull_scene_inputs, cull_small_inputs, ladder_inputs, reference, scene_cull_host_sort,
                             scene_group_walk, scene_lane_walk)
from test_scene_extremes import RUNGS, meshes as ladder_meshes
from test_scene_knn import inactive_of
from test_scene_overlap import slice_queries, tri_leaf_boxes

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32
AUTO, LANE, GROUP = 0, 1, 2
PATHS = (LANE, GROUP, AUTO)
TLAS_ALGO = {1: 3, 2: 0, 7: 1, 64: 2}
REC = 16                                                                # bytes of a bvh_scene_cull_hit


def call(pkg, scene, d_planes, m, per, path, d_offsets, d_hits, capacity, total=True):
    t = C.c_uint64(0xDEAD)
    rc = pkg.lib().bvh_scene_cull(scene.handle, d_planes, m, per, path, d_offsets, d_hits, capacity, C.byref(t) if total else None)
    return rc, t.value


def search(pkg, scene, vols, path):
    """a count-only call, then a call with the exact capacity; returns (offsets, records, the overflow words of the second call).  The count-only offsets
    must equal the fill's."""
    ctx, (m, per, _) = scene.ctx, vols.shape
    d_planes, d_off = ctx.upload(vols), ctx.alloc((m + 1) * 4)
    hits = None
    try:
        rc, total = call(pkg, scene, d_planes.ptr, m, per, path, d_off.ptr, None, 0)
        assert rc == 0, rc
        counted = d_off.download(np.uint32, m + 1)
        assert counted[0] == 0 and counted[-1] == total
        hits = ctx.alloc(max(total, 1) * REC)
        rc, total2 = call(pkg, scene, d_planes.ptr, m, per, path, d_off.ptr, hits.ptr, total)
        assert rc == 0 and total2 == total
        words = ctx.query_overflow()
        off = d_off.download(np.uint32, m + 1)
        assert off.tobytes() == counted.tobytes(), "count-only and fill calls disagree on the offsets"
        return off, hits.download(pkg.SCENE_CULL_HIT, total), words
    finally:
        d_planes.free(); d_off.free()
        if hits is not None:
            hits.free()


def check_all_paths(pkg, scene, vols, ref, what, paths=PATHS):
    """every path against the brute force on every volume, and byte-equal to itself when called twice.  Returns {path: (offsets, records, overflow words)}"""
    out = {}
    for path in paths:
        off, recs, words = search(pkg, scene, vols, path)
        check_scene_cull(pkg, off, recs, ref, f"{what}, path {path}")
        off2, recs2, _ = search(pkg, scene, vols, path)
        assert off2.tobytes() == off.tobytes() and recs2.tobytes() == recs.tobytes(), f"{what}, path {path}: the same call twice gives other bytes"
        out[path] = (off, recs, words)
    return out


# ---- exactness ----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", PLANE_COUNTS)
@pytest.mark.parametrize("n_inst", [1, 2, 7, 64])
def test_exact_on_every_volume(pkg, n_inst, per):
    """1: no top-level tree; 2: a root with two leaf children; 7: the singular instance inactive, a sheared one; 64: all three kinds of inactive instance.
    BLAS b comes from builder b (layouts 0 and 1) in triangle format b % 3; the last BLAS has two triangles"""
    meshes, inst, vols, ref = cull_scene_inputs(pkg, n_inst, per)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo], fmt=algo % 3) for algo in range(4)]
        same_root_boxes(pkg, blases, meshes)
        assert {(b[0] if isinstance(b, tuple) else b).result.layout for b in blases} == {0, 1}
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[n_inst], blases, inst)
        got = check_all_paths(pkg, scene, vols, ref, f"{n_inst} instances x {per} planes")
        assert not set(got[LANE][1]["instance"].tolist()) & inactive_of(n_inst), "an inactive instance answered"
        if per == 6:                                                      # the Python binding
            for path, name in ((LANE, "lane"), (GROUP, "group"), (AUTO, "auto")):
                poff, precs = scene.cull(vols, path=name)
                assert poff.tobytes() == got[path][0].tobytes() and precs.tobytes() == got[path][1].tobytes()
            assert scene.cull(vols, count_only=True).tobytes() == ref["offsets"].tobytes()
            one_off, one_recs = scene.cull(vols[1])                       # (planes, 4): one volume
            check_scene_cull(pkg, one_off, one_recs, reference(pkg, vols[1:2], [tri_leaf_boxes(t) for t in meshes], inst), "one volume")
            if n_inst == 7:                                               # 65 volumes: a partial last wave of the lane walk
                ref65 = reference(pkg, vols[:65], [tri_leaf_boxes(t) for t in meshes], inst)
                check_all_paths(pkg, scene, vols[:65], ref65, "65 volumes", paths=(LANE,))
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("ploc", [False, True])
def test_build_many_slices_as_blases(pkg, ploc):
    """the four meshes built by one bvh_build_many (layout 0) or bvh_build_many_ploc (layout 1) call, each slice a BLAS of the 7-instance scene"""
    meshes, inst, vols, ref = cull_scene_inputs(pkg, 7, 6)
    ctx = pkg.Context(0)
    try:
        mt = ctx.build_many_ploc(meshes) if ploc else ctx.build_many(meshes)
        ctx.synchronize()
        scene = pkg.Scene(ctx).build(3, [mt.blas(m) for m in range(len(meshes))], inst)
        check_all_paths(pkg, scene, vols, ref, "build_many_ploc slices" if ploc else "build_many slices")
        scene.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("tlas_algo", [0, 3])
def test_coincident_instances_report_every_pair_once_per_instance(pkg, tlas_algo):
    """two instances place the same triangles identically; one BLAS also holds a far-off extra triangle that stretches its world box, so the two are not
    walked alike.  Every shared triangle whose box passes is reported for instance 0 and for instance 1 with the same mask, whichever BLAS is stretched"""
    mesh, stretched, inst, vols = cull_coincident_inputs(pkg, tlas_algo)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        plain, far = bl.add(3, mesh), bl.add(1, stretched)
        for order in ((plain, far), (far, plain)):
            blas_tris = [mesh, stretched] if order[0] is plain else [stretched, mesh]
            ref = reference(pkg, vols, [tri_leaf_boxes(t) for t in blas_tris], inst)
            scene = pkg.Scene(sc_ctx).build(tlas_algo, list(order), inst)
            got = check_all_paths(pkg, scene, vols, ref, "coincident")
            off, recs, _ = got[GROUP]
            recs = scene_cull_host_sort(off, recs); q = slice_queries(off)
            shared = recs["prim"] < len(mesh)
            a, b = shared & (recs["instance"] == 0), shared & (recs["instance"] == 1)
            assert a.sum() == b.sum() > 1000 and np.array_equal(q[a], q[b]) and np.array_equal(recs["prim"][a], recs["prim"][b])
            assert np.array_equal(recs["straddle"][a], recs["straddle"][b])
            scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- relations ------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [1, 3])
def test_one_identity_instance_equals_cull_on_the_blas(pkg, algo):
    """((a 1 + b 0) + c 0) == a as a value: the {prim, straddle} sets are bvh_cull's on the BLAS for every volume and every path"""
    meshes, _, vols, _ = cull_scene_inputs(pkg, 1, 6)
    mesh = meshes[0]
    inst = make_instances(pkg, [identity()], [0])
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(algo, mesh)
        assert b.result.layout == (0 if algo == 1 else 1)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        ref_off, ref_hits = pkg.cull_brute_force(vols, tri_leaf_boxes(mesh))
        for name in ("lane", "group", "auto"):
            foff, fhits = b.cull(vols, path=name)
            off, recs = scene.cull(vols, path=name)
            recs = scene_cull_host_sort(off, recs)
            fhits = fhits[np.lexsort((fhits["prim"], slice_queries(foff)))]
            assert len(recs) > 1000 and (recs["instance"] == 0).all() and (recs["zero"] == 0).all()
            assert off.tobytes() == foff.tobytes() == ref_off.tobytes()
            assert recs["prim"].tobytes() == fhits["prim"].tobytes() == ref_hits["prim"].tobytes(), name
            assert recs["straddle"].tobytes() == fhits["straddle"].tobytes() == ref_hits["straddle"].tobytes(), name
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_instances_seen_are_a_subset_of_cull_on_the_top_level_tree(pkg):
    meshes, inst, vols, ref = cull_scene_inputs(pkg, 64, 6)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo]) for algo in range(4)]
        scene = pkg.Scene(sc_ctx).build(2, blases, inst)
        off, recs = scene.cull(vols)
        toff, thits = scene.cull_instances(vols)
        seen = set(zip(slice_queries(off).tolist(), recs["instance"].tolist()))
        broad = set(zip(slice_queries(toff).tolist(), thits["prim"].tolist()))
        assert seen and seen <= broad and len(seen) < len(broad)          # (a world box passes more often than a leaf box inside it)
        assert not {k for _, k in seen} & inactive_of(64)
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def download_tlas(pkg, ctx, scene):
    t = scene.tlas()
    n = t.n_leaves
    assert t.layout == 1
    nodes = np.empty(n - 1, dtype=pkg.BVH2_NODE); leaves = np.empty(n, dtype=pkg.PRIMREF)
    assert pkg.lib().bvh_download(ctx.handle, C.byref(t), nodes.ctypes.data, leaves.ctypes.data, None, None, None) == 0
    return Tree(nodes, leaves, int(t.root), n, 1)


def test_group_walk_bytes_equal_the_host_restatement(pkg):
    """the 7-instance scene with the trees downloaded from the device: every slice of the group walk is the restated schedule's emission order, byte for
    byte, and the lane walk's slices are the restated lane walk's"""
    meshes, inst, vols, ref = cull_scene_inputs(pkg, 7, 6)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo]) for algo in range(4)]
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        trees = []
        for b, tris in zip(blases, meshes):
            d = b.download()
            trees.append(Tree(d["nodes"], d["leaves"], int(b.result.root), len(tris), int(b.result.layout)))
        sc = HostScene(pkg, download_tlas(pkg, sc_ctx, scene), trees, inst, [tri_leaf_boxes(t) for t in meshes])
        stored = np.concatenate([sc.top.leaf_boxes["min"], sc.top.leaf_boxes["max"]], axis=1)
        assert stored[sc.active].tobytes() == sc.wb[sc.active].tobytes(), "the stored world boxes of the active instances are not the restated ones"
        goff, grecs, gw = search(pkg, scene, vols, GROUP)
        loff, lrecs, lw = search(pkg, scene, vols, LANE)
        assert gw == (0, 0) and lw == (0, 0)
        peak = 0
        for i in range(N_VOLUMES):
            want, p = scene_group_walk(sc, vols[i])
            peak = max(peak, p)
            assert grecs[goff[i]:goff[i + 1]].tobytes() == want.tobytes(), f"volume {i}: the group walk's slice is not in the schedule's emission order"
            want, _ = scene_lane_walk(sc, vols[i])
            assert lrecs[loff[i]:loff[i + 1]].tobytes() == want.tobytes(), f"volume {i}: the lane walk's slice is not in the walk's order"
        print(f"group stack occupancy up to {peak} of {pkg.SCENE_CULL_GROUP_STACK}")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_auto_takes_the_walk_the_rule_names(pkg):
    """BVH_CULL_AUTO: the group walk iff n_volumes <= 65536 and n_instances + the largest BLAS's n_leaves >= 1024"""
    meshes, inst, vols, _ = cull_scene_inputs(pkg, 7, 6)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        big, small = bl.add(3, meshes[0]), bl.add(3, meshes[2])          # 2000 and 700 leaves
        for blases, count, walk in (([big, small], 256, "k_scene_cull_group"), ([small], 256, "k_scene_cull_walk"),
                                    ([big, small], 65536, "k_scene_cull_group"), ([big, small], 65537, "k_scene_cull_walk")):
            ins = inst.copy(); ins["blas"] = np.minimum(inst["blas"], len(blases) - 1)
            scene = pkg.Scene(sc_ctx).build(3, blases, ins)
            v = np.ascontiguousarray(np.tile(vols[2::8], (count // 32 + 1, 1, 1))[:count])      # volumes that hold nothing
            sc_ctx.set_profiling(2)
            off = scene.cull(v, path="auto", count_only=True)
            kt = sc_ctx.kernel_times()
            sc_ctx.set_profiling(0)
            other = "k_scene_cull_walk" if walk == "k_scene_cull_group" else "k_scene_cull_group"
            assert walk in kt and other not in kt and {"k_scene_cull_deep", "k_overlap_scan"} <= set(kt), (count, sorted(kt))
            assert off[-1] == 0
            scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- updates ----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_update_after_moves_and_blas_refit(pkg):
    meshes, inst, moved, vols, refit, ref_moved, ref_refit = cull_moved_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        before = scene.cull(vols, count_only=True)
        scene.update(moved)                                               # moved and toggled instances, no rebuild
        same_root_boxes(pkg, blases, meshes)
        got = check_all_paths(pkg, scene, vols, ref_moved, "after update")
        assert before.tobytes() != got[LANE][0].tobytes()
        assert not set(got[GROUP][1]["instance"].tolist()) & {61, 62, 63}
        fresh = pkg.Scene(sc_ctx).build(3, blases, moved)
        foff, frecs, _ = search(pkg, fresh, vols, LANE)
        assert foff.tobytes() == got[LANE][0].tobytes() and scene_cull_host_sort(foff, frecs).tobytes() == scene_cull_host_sort(*got[LANE][:2]).tobytes()
        fresh.close()
        blases[0].refit(refit[0])
        bl.ctxs[0].synchronize()                                          # (the refit ran on the BLAS's own stream: complete before the scene reads the root box)
        scene.update(moved)
        same_root_boxes(pkg, blases, refit)
        check_all_paths(pkg, scene, vols, ref_refit, "after BLAS refit")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- passes, capacity, argument handling and memory hygiene -----------------------------------------------------------------------------------------------------------

def small_scene(pkg, bl):
    mesh, inst, vols, ref = cull_small_inputs(pkg)
    return mesh, bl.add(3, mesh), inst, vols, ref


@pytest.mark.parametrize("path", [LANE, GROUP])
def test_passes_and_capacity(pkg, path):
    bl, ctx = Blases(pkg), pkg.Context(0)
    try:
        mesh, b, inst, vols, ref = small_scene(pkg, bl)
        scene = pkg.Scene(ctx).build(2, [b], inst)
        m, per = len(vols), vols.shape[1]
        exp_off, exp_recs, _ = search(pkg, scene, vols, path)
        total = int(exp_off[-1])
        assert total > 100
        check_scene_cull(pkg, exp_off, exp_recs, ref, "small scene")
        extra = 29
        guard_h = np.frombuffer(np.full((total + extra) * REC, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.SCENE_CULL_HIT)
        guard_o = np.full(m + 1 + extra, 0xA5A5A5A5, dtype=np.uint32)
        d_planes, d_off, d_hits = ctx.upload(vols), ctx.upload(guard_o), ctx.upload(guard_h)
        # count only: d_hits untouched, offsets complete, guard words past n_volumes + 1 offsets intact
        assert call(pkg, scene, d_planes.ptr, m, per, path, d_off.ptr, None, 0) == (0, total)
        o = d_off.download(np.uint32, m + 1 + extra)
        assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
        assert d_hits.download(pkg.SCENE_CULL_HIT, total + extra).tobytes() == guard_h.tobytes()
        # capacity one short: the fill is skipped, d_hits untouched, d_offsets still complete, *total_out set
        d_off.upload(guard_o)
        assert call(pkg, scene, d_planes.ptr, m, per, path, d_off.ptr, d_hits.ptr, total - 1) == (0, total)
        o = d_off.download(np.uint32, m + 1 + extra)
        assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
        assert d_hits.download(pkg.SCENE_CULL_HIT, total + extra).tobytes() == guard_h.tobytes()
        # the exact capacity is filled; guard records past the total intact; twice the same bytes
        out = {}
        for rnd in range(2):
            d_off.upload(guard_o); d_hits.upload(guard_h)
            assert call(pkg, scene, d_planes.ptr, m, per, path, d_off.ptr, d_hits.ptr, total) == (0, total)
            o, h = d_off.download(np.uint32, m + 1 + extra), d_hits.download(pkg.SCENE_CULL_HIT, total + extra)
            assert o[m + 1:].tobytes() == guard_o[m + 1:].tobytes() and h[total:].tobytes() == guard_h[total:].tobytes()
            assert o[: m + 1].tobytes() == exp_off.tobytes() and h[:total].tobytes() == exp_recs.tobytes()
            out[rnd] = (o.tobytes(), h.tobytes())
        assert out[0] == out[1], "two identical calls give different bytes"
        # total_out == NULL: the same device bytes after a synchronize
        d_off.upload(guard_o); d_hits.upload(guard_h)
        rc, t = call(pkg, scene, d_planes.ptr, m, per, path, d_off.ptr, d_hits.ptr, total + extra, total=False)
        assert rc == 0 and t == 0xDEAD
        ctx.synchronize()
        assert (d_off.download(np.uint32, m + 1 + extra).tobytes(), d_hits.download(pkg.SCENE_CULL_HIT, total + extra).tobytes()) == out[0]
        assert d_planes.download(F32, vols.size).tobytes() == vols.tobytes()
        # n_volumes == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        d_off.upload(guard_o); d_hits.upload(guard_h)
        assert call(pkg, scene, d_planes.ptr, 0, per, path, d_off.ptr, d_hits.ptr, total) == (0, 0)
        o = d_off.download(np.uint32, m + 1 + extra)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes() and d_hits.download(pkg.SCENE_CULL_HIT, total + extra).tobytes() == guard_h.tobytes()
        # the binding's capacity protocol: a capacity that is too small is re-allocated from the reported total
        qoff, qrecs = scene.cull(vols, path=path, capacity=3)
        assert qoff.tobytes() == exp_off.tobytes() and qrecs.tobytes() == exp_recs.tobytes()
        eo, er = scene.cull(vols[:0])
        assert eo.tolist() == [0] and len(er) == 0 and er.dtype == pkg.SCENE_CULL_HIT and scene.cull(vols[:0], count_only=True).tolist() == [0]
        with pytest.raises(pkg.BvhError):
            scene.cull(np.zeros((4, 9, 4), dtype=F32))
        with pytest.raises(pkg.BvhError):
            scene.cull(vols, path="wave")
        scene.close(); d_planes.free(); d_off.free(); d_hits.free()
    finally:
        bl.close(); ctx.close()


def test_one_instance_on_a_fresh_ctx(pkg):
    """a one-instance scene builds no top-level tree, so a fresh ctx has no arena yet: the first call reserves the smallest one"""
    mesh, inst, vols, _ = cull_small_inputs(pkg)
    one = inst[:1].copy()
    ref = reference(pkg, vols, [tri_leaf_boxes(mesh)], one)
    for path in ("lane", "group"):
        bl, sc_ctx = Blases(pkg), pkg.Context(0)
        try:
            scene = pkg.Scene(sc_ctx).build(3, [bl.add(2, mesh)], one)
            off, recs = scene.cull(vols, path=path)
            check_scene_cull(pkg, off, recs, ref, "fresh ctx")
            scene.close()
        finally:
            bl.close(); sc_ctx.close()


def test_errors_write_nothing(pkg):
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    L = pkg.lib()
    try:
        mesh, b, inst, vols, ref = small_scene(pkg, bl)
        m, per = len(vols), vols.shape[1]
        d_planes = sc_ctx.upload(vols)
        cap = int(ref["offsets"][-1]) + 64
        guard_h = np.frombuffer(np.full(cap * REC, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.SCENE_CULL_HIT)
        guard_o = np.full(m + 1, 0x5A5A5A5A, dtype=np.uint32)
        hits, offs = sc_ctx.upload(guard_h), sc_ctx.upload(guard_o)
        tot = C.c_uint64(0x77)
        unbuilt, scene = pkg.Scene(sc_ctx), pkg.Scene(sc_ctx).build(2, [b], inst)

        def go(sc=scene, p=d_planes.ptr, n=m, k=per, path=AUTO, o=offs.ptr, h=hits.ptr, c=cap):
            return L.bvh_scene_cull(sc.handle if sc is not None else None, p, n, k, path, o, h, c, C.byref(tot))
        cases = {
            "null scene": go(sc=None), "unbuilt scene": go(sc=unbuilt), "null planes": go(p=None), "null offsets": go(o=None),
            "0 planes": go(k=0), "9 planes": go(k=9), "path 3": go(path=3), "path -1": go(path=-1),
            "n_volumes 2^30": go(n=1 << 30),
            "offsets in planes": go(o=d_planes.ptr + 48), "hits in planes": go(h=d_planes.ptr + 32), "hits in offsets": go(h=offs.ptr + 16),
            "offsets in hits": go(o=hits.ptr + REC * (cap - 1)), "planes in hits": go(p=hits.ptr, h=hits.ptr + REC * 8),
            "hits over the planes, capacity clamped": go(h=d_planes.ptr - 16, c=1 << 40),
            "unbuilt, n_volumes 0": go(sc=unbuilt, n=0),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        assert tot.value == 0x77
        sc_ctx.synchronize()
        assert hits.download(pkg.SCENE_CULL_HIT, cap).tobytes() == guard_h.tobytes() and offs.download(np.uint32, m + 1).tobytes() == guard_o.tobytes()
        assert d_planes.download(F32, vols.size).tobytes() == vols.tobytes()
        # a count-only call ignores the capacity's range, and the scene still answers
        assert go(h=None, c=1 << 40) == 0 and tot.value == ref["offsets"][-1]
        total = tot.value
        assert offs.download(np.uint32, m + 1)[-1] == total and hits.download(pkg.SCENE_CULL_HIT, cap).tobytes() == guard_h.tobytes()
        assert go() == 0 and tot.value == total
        got = hits.download(pkg.SCENE_CULL_HIT, cap)
        assert got[total:].tobytes() == guard_h[total:].tobytes()
        check_scene_cull(pkg, offs.download(np.uint32, m + 1), got[:total], ref, "after the errors")
        # n_volumes == 0 on a built scene: d_offsets[0] = 0 and *total_out = 0
        offs.upload(guard_o)
        assert go(n=0) == 0 and tot.value == 0
        o = offs.download(np.uint32, m + 1)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes()
        scene.close(); unbuilt.close(); d_planes.free(); hits.free(); offs.free()
    finally:
        bl.close(); sc_ctx.close()


# ---- depth ------------------------------------------------------------------------------------------------------------------------------------------------------------

def box_tris(pkg, leaf):
    """triangles whose fminf / fmaxf boxes are the given leaf boxes (a BLAS descriptor names triangles; bvh_scene_cull never reads them)"""
    t = np.zeros(len(leaf), dtype=pkg.meshgen.TRIANGLE)
    t["v1"], t["v2"], t["v3"] = leaf["min"], leaf["max"], leaf["min"]
    return t


def arrays_scene(pkg, c, sc_ctx, tris, nodes, root, n, inst, algo=3):
    """a scene over one caller-filled layout-0 BLAS"""
    d_tris, d_nodes = c.upload(tris), c.upload(nodes)
    r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
    return pkg.Scene(sc_ctx).build(algo, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst), (d_tris, d_nodes)


@pytest.mark.parametrize("H,deep", [(300, True), (20, False)])
def test_deep_blas_takes_the_stackless_pass(pkg, H, deep):
    """the caterpillar under five instances: a volume that holds an instance needs about H / 2 entries of the lane walk's stack in its BLAS (the host
    restatement: tests/test_scene_cull.py).  H = 300 overflows the short stack in the count AND in the fill pass — the overflow words say so —, H = 20 is the
    control on the same code path"""
    tris, nodes, root, n, inst, vols, ref = cull_deep_inputs(pkg, H)
    c, sc_ctx = pkg.Context(0), pkg.Context(0)
    try:
        scene, bufs = arrays_scene(pkg, c, sc_ctx, tris, nodes, root, n, inst)
        sc_ctx.set_profiling(2)
        off, recs, words = search(pkg, scene, vols, LANE)
        kt = sc_ctx.kernel_times()
        sc_ctx.set_profiling(0)
        assert {"k_scene_cull_walk", "k_scene_cull_deep", "k_overlap_scan"} <= set(kt) and "k_scene_cull_group" not in kt, sorted(kt)
        launches = {k: v[1] for k, v in kt.items()}                       # (search: a count-only call, then a call that counts and fills)
        assert launches["k_scene_cull_walk"] == 3 and launches["k_scene_cull_deep"] == 3 and launches["k_overlap_scan"] == 2, launches
        print(f"caterpillar {H}: {words[0]} volumes left to the stackless pass by the count pass, {words[1]} by the fill pass")
        assert (words[0] >= 64 and words[1] >= 64) if deep else words == (0, 0), words
        check_scene_cull(pkg, off, recs, ref, f"caterpillar {H}, lane")
        check_all_paths(pkg, scene, vols, ref, f"caterpillar {H}", paths=(GROUP, AUTO))
        scene.close()
        for b in bufs:
            b.free()
    finally:
        sc_ctx.close(); c.close()


@pytest.mark.parametrize("tlas_algo", [2, 3])
def test_deep_top_level_takes_the_stackless_pass(pkg, tlas_algo):
    """180 instances on the staircase: the PLOC-family top-level trees chain the steps up, and a volume that holds them all pushes at every chain node of the
    lane walk (the need is the host restatement's on the downloaded top-level tree)"""
    mesh, inst, vols, ref = cull_deep_top_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        scene = pkg.Scene(sc_ctx).build(tlas_algo, [b], inst)
        d = b.download()
        sc = HostScene(pkg, download_tlas(pkg, sc_ctx, scene), [Tree(d["nodes"], d["leaves"], int(b.result.root), len(mesh), int(b.result.layout))], inst,
                       [tri_leaf_boxes(mesh)])
        deep_need, quiet_need = scene_lane_walk(sc, vols[0])[1], max(scene_lane_walk(sc, vols[i])[1] for i in range(1, len(vols), 2))
        print(f"tlas algo {tlas_algo}: the covering volume needs {deep_need} entries, the others at most {quiet_need}")
        assert deep_need > QUERY_STACK and quiet_need + 8 <= QUERY_STACK
        got = check_all_paths(pkg, scene, vols, ref, f"deep top level, algo {tlas_algo}")
        assert got[LANE][2][0] >= len(vols) // 2 and got[LANE][2][1] >= len(vols) // 2, got[LANE][2]
        assert got[GROUP][2] == (0, 0), got[GROUP][2]
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("levels,over", [(32, True), (31, False)])
def test_group_stack_overflow_hands_over_to_the_stackless_pass(pkg, levels, over):
    """a one-instance scene over test_cull.fat_caterpillar: by the host restatement an all-containing volume reaches 8448 entries at 32 levels — above
    BVH_SCENE_CULL_GROUP_STACK — and exactly 8192 at 31, the control that stays in the group walk.  Beside it: volumes that stay far below the capacity, so
    marked and unmarked volumes share a launch.  The overflow words say which walk served them; the answers equal the brute force either way"""
    leaf, nodes, root, n, inst, vols, ref = cull_fat_inputs(pkg, levels)
    sc = HostScene(pkg, None, [Tree(nodes, None, root, n, 0)], inst, [leaf])
    peaks = [scene_group_walk(sc, v)[1] for v in (vols[0], vols[2], vols[6])]
    assert (peaks[0] > pkg.SCENE_CULL_GROUP_STACK) == over and peaks[0] == 256 * (levels - 1) + 512 and max(peaks[1:]) < pkg.SCENE_CULL_GROUP_STACK // 2, peaks
    c, sc_ctx = pkg.Context(0), pkg.Context(0)
    try:
        scene, bufs = arrays_scene(pkg, c, sc_ctx, box_tris(pkg, leaf), nodes, root, n, inst)
        sc_ctx.set_profiling(2)
        off, recs, words = search(pkg, scene, vols, GROUP)
        kt = sc_ctx.kernel_times()
        sc_ctx.set_profiling(0)
        assert {"k_scene_cull_group", "k_scene_cull_deep", "k_overlap_scan"} <= set(kt) and "k_scene_cull_walk" not in kt, sorted(kt)
        print(f"fat caterpillar {levels}: overflow words {words}")
        assert (words[0] >= 3 and words[1] >= 3) if over else words == (0, 0), words          # volumes 0, 1 and 11 hold everything
        check_scene_cull(pkg, off, recs, ref, f"fat caterpillar {levels}, group")
        off2, recs2, _ = search(pkg, scene, vols, GROUP)
        assert off2.tobytes() == off.tobytes() and recs2.tobytes() == recs.tobytes()          # the same bytes, served by either walk
        check_all_paths(pkg, scene, vols, ref, f"fat caterpillar {levels}", paths=(LANE, AUTO))
        scene.close()
        for b in bufs:
            b.free()
    finally:
        sc_ctx.close(); c.close()


# ---- extreme transforms -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", RUNGS)
def test_instance_ladder(pkg, name):
    """a rung of tests/test_scene_extremes.py's ladder: where the brute force meets no NaN in any s or s' the sets are equal on every path; elsewhere every
    slice is a subset of the brute force's — every record passes its own test — without duplicates (tests/test_scene_cull.py asserts which rungs must be in
    the first class)"""
    inst, vols, ref, nan = ladder_inputs(pkg, name)
    meshes = ladder_meshes(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1])]
        same_root_boxes(pkg, blases, meshes)
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        if not nan:
            check_all_paths(pkg, scene, vols, ref, name)
        else:
            want = set(zip(slice_queries(ref["offsets"]).tolist(), ref["recs"]["instance"].tolist(), ref["recs"]["prim"].tolist(), ref["recs"]["straddle"].tolist()))
            for path in PATHS:
                off, recs, _ = search(pkg, scene, vols, path)
                got = list(zip(slice_queries(off).tolist(), recs["instance"].tolist(), recs["prim"].tolist(), recs["straddle"].tolist()))
                assert len(set(got)) == len(got) and set(got) <= want and (recs["zero"] == 0).all(), f"{name}, path {path}"
        scene.close()
    finally:
        bl.close(); sc_ctx.close()
