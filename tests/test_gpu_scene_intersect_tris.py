"""bvh_scene_intersect_tris on the GPU: which triangles of which active instances each query triangle properly crosses, against the two-level numpy brute
force (tests/test_scene_intersect_tris.py, which also makes the inputs and checks their premises without a device) on EVERY query — whole sets, sorted bytes
included; the unsorted slices equal the sorted ones as sets and the same call twice gives the same bytes.  Both modes (a world-space query mesh in each
triangle format; the triangles of one instance, looked up on the device) for 1 to 64 instances over BLASes of every builder, layout and format; sheared,
mirrored and far-offset instances; coincident instances; the relations to bvh_intersect_tris, bvh_scene_overlap and between the instance rows; independence
from the builders; a deep BLAS and a deep top level through the stackless pass, with a short-tree control; bvh_scene_update after moves (from host and from
device memory) and after a BLAS refit; the passes and the capacity decision; rejections and buffer hygiene; the binding's input kinds."""
import ctypes as C

import numpy as np
import pytest

from test_deep_trees import combined
from test_gpu_intersect_tris import DeviceMesh
from test_gpu_scene import TLAS_ALGO, Blases
from test_intersect_tris import as_triangles, stage_e_boxes, tris_brute_force, xyz
from test_overlap import csr_of, sorted_slices
from test_query import E_INVALID
from test_scene import identity, make_instances
from test_scene_knn import inactive_of
from test_scene_intersect_tris import (INSTANCE_PRIM, QUERY_STACK, SCENE_TRIS_INSTANCE, SCENE_TRIS_QUERY, SCENE_TRIS_SORTED, check_scene_tris, instance_queries,
                                       left_first_scene_need, scene_tris_brute_force, tris_builders_inputs, tris_coincident_inputs, tris_deep_inputs,
                                       tris_deep_top_inputs, tris_exact_inputs, tris_instance_inputs, tris_kinds_inputs, tris_moved_inputs, tris_small_inputs)
from test_scene_overlap import scene_host_sort, slice_queries

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32


def call(pkg, scene, qin, m, mode, k, flags, d_offsets, d_prims, capacity, total=True):
    t = C.c_uint64(0xDEAD)
    rc = pkg.lib().bvh_scene_intersect_tris(scene.handle, C.byref(qin) if qin is not None else None, m, mode, k, flags, d_offsets, d_prims, capacity,
                                            C.byref(t) if total else None)
    return rc, t.value


def search(pkg, scene, qin, m, mode, k, flags):
    """count-only call, then a fill with the exact capacity; returns (offsets, records).  The count-only offsets must equal the fill's."""
    ctx = scene.ctx
    d_off, prims = ctx.alloc((m + 1) * 4), None
    try:
        rc, total = call(pkg, scene, qin, m, mode, k, flags, d_off.ptr, None, 0)
        assert rc == 0, rc
        counted = d_off.download(np.uint32, m + 1)
        assert counted[0] == 0 and counted[-1] == total
        prims = ctx.alloc(max(total, 1) * 8)
        rc, total2 = call(pkg, scene, qin, m, mode, k, flags, d_off.ptr, prims.ptr, total)
        assert rc == 0 and total2 == total
        off = d_off.download(np.uint32, m + 1)
        assert off.tobytes() == counted.tobytes(), "count-only and fill calls disagree on the offsets"
        return off, prims.download(pkg.INSTANCE_PRIM, total)
    finally:
        d_off.free()
        if prims is not None:
            prims.free()


def check_all_ways(pkg, scene, queries, ref, what, fmt=0, instance=None, rows=None):
    """the sorted fill against the brute force on every query; the unsorted fill set-equal to the sorted one and byte-equal to itself when called twice;
    the count-only offsets equal to the fill's (search asserts it).  queries: (m, 3, 3) world triangles, uploaded in format fmt — or None with
    instance=k and rows: BVH_SCENE_TRIS_INSTANCE.  Returns the sorted answer"""
    mesh = DeviceMesh(pkg, scene.ctx, as_triangles(pkg, queries), fmt) if instance is None else None
    qin, m, mode, k = (mesh.inp, mesh.n, SCENE_TRIS_QUERY, 0) if mesh is not None else (None, rows, SCENE_TRIS_INSTANCE, instance)
    try:
        off, recs = search(pkg, scene, qin, m, mode, k, SCENE_TRIS_SORTED)
        check_scene_tris(off, recs, ref, True, what + " sorted")
        uoff, urecs = search(pkg, scene, qin, m, mode, k, 0)
        check_scene_tris(uoff, urecs, ref, False, what + " unsorted")
        assert scene_host_sort(uoff, urecs).tobytes() == recs.tobytes(), f"{what}: the unsorted slices are not the sorted ones as sets"
        uoff2, urecs2 = search(pkg, scene, qin, m, mode, k, 0)
        assert uoff2.tobytes() == uoff.tobytes() and urecs2.tobytes() == urecs.tobytes(), f"{what}: the same unsorted call twice gives other bytes"
        return off, recs
    finally:
        if mesh is not None:
            mesh.free()


def four_blases(pkg, bl, meshes):
    """BLAS b from builder b (layouts 0 and 1) in triangle format b % 3; the leaf boxes are stage E's, so the root box is the triangles' bound"""
    blases = [bl.add(algo, meshes[algo], fmt=algo % 3) for algo in range(4)]
    assert {(b[0] if isinstance(b, tuple) else b).result.layout for b in blases} == {0, 1}
    return blases


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------------------------

INSTANCE_CASES = {1: [0], 2: [0, 1], 3: [1, 2], 64: [3, 62]}         # (3, 2) and (64, 62): an inactive query instance


@pytest.mark.parametrize("n_inst", [1, 2, 3, 64])
def test_exact_on_every_query_in_both_modes(pkg, n_inst):
    """1: no top-level tree; 2: a root with two leaf children; 3: the singular instance inactive; 64: all three kinds of inactive instance"""
    meshes, inst, q, ref = tris_exact_inputs(pkg, n_inst)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[n_inst], four_blases(pkg, bl, meshes), inst)
        off, recs = check_all_ways(pkg, scene, q, ref, f"{n_inst} instances", fmt=n_inst % 3)
        assert not set(recs["instance"].tolist()) & inactive_of(n_inst), "an inactive instance answered"
        poff, precs = scene.intersect_tris(as_triangles(pkg, q))         # the Python binding, a host mesh
        assert poff.tobytes() == off.tobytes() and precs.tobytes() == recs.tobytes()
        if n_inst == 3:                                                   # 65 queries: a partial last wave
            _, _, q65, ref65 = tris_exact_inputs(pkg, 3, m=65)
            check_all_ways(pkg, scene, q65, ref65, "65 queries", fmt=1)
        for k in INSTANCE_CASES[n_inst]:
            _, _, rows, iref = tris_instance_inputs(pkg, n_inst, k)
            ioff, irecs = check_all_ways(pkg, scene, None, iref, f"{n_inst} instances, instance {k}", instance=k, rows=len(rows))
            assert k not in irecs["instance"] and not set(irecs["instance"].tolist()) & inactive_of(n_inst)
            boff, brecs = scene.intersect_tris(instance=k)                # the binding: as many rows as the largest BLAS has leaves
            assert boff.tobytes() == ioff.tobytes() and brecs.tobytes() == irecs.tobytes()
            if n_inst == 3 and k == 1:                                    # 65 rows: a partial last wave, and fewer rows than the BLAS has leaves
                cut = scene_tris_brute_force(rows[:65], meshes, inst, skip=k)
                check_all_ways(pkg, scene, None, cut, "65 rows", instance=k, rows=65)
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("kind", ["shear", "mirror", "far"])
def test_sheared_mirrored_and_far_offset_instances(pkg, kind):
    mesh, inst, q, ref = tris_kinds_inputs(pkg, kind)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        scene = pkg.Scene(sc_ctx).build(3, [bl.add(3, mesh)], inst)
        check_all_ways(pkg, scene, q, ref, kind, fmt=2)
        iref = scene_tris_brute_force(instance_queries([mesh], inst, 5, len(mesh)), [mesh], inst, skip=5)
        assert iref["offsets"][-1] > 0
        check_all_ways(pkg, scene, None, iref, kind + ", instance 5", instance=5, rows=len(mesh))
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("tlas_algo", [0, 3])
def test_coincident_instances_report_every_pair_once_per_instance(pkg, tlas_algo):
    """two instances place the same triangles identically; one BLAS also holds a far-off extra triangle that stretches its world box, so the two are not
    walked alike.  Every shared triangle that a query crosses is reported for instance 0 and for instance 1, whichever BLAS is the stretched one; and in
    instance mode the coincident copy is a different instance: coplanar, so it is not crossed, and the call reports nothing"""
    mesh, stretched, inst, q = tris_coincident_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        plain, far = bl.add(3, mesh), bl.add(1, stretched)
        for order in ((plain, far), (far, plain)):
            blas_tris = [mesh, stretched] if order[0] is plain else [stretched, mesh]
            ref = scene_tris_brute_force(q, blas_tris, inst)
            scene = pkg.Scene(sc_ctx).build(tlas_algo, list(order), inst)
            off, recs = check_all_ways(pkg, scene, q, ref, "coincident")
            qq = slice_queries(off)
            a, b = recs["instance"] == 0, recs["instance"] == 1
            assert a.sum() == b.sum() > 100 and np.array_equal(qq[a], qq[b]) and np.array_equal(recs["prim"][a], recs["prim"][b])
            rows = len(stretched)
            iref = scene_tris_brute_force(instance_queries(blas_tris, inst, 0, rows), blas_tris, inst, skip=0)
            ioff, irecs = check_all_ways(pkg, scene, None, iref, "coincident, instance 0", instance=0, rows=rows)
            self_sets = tris_brute_force(blas_tris[0], blas_tris[1])      # the copy is skipped by INDEX only: instance 1 answers with the mesh's self-crossings
            assert (irecs["instance"] == 1).all() and ioff[-1] == sum(len(s) for s in self_sets) > 0
            scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- relations --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [1, 3])
def test_one_identity_instance_equals_intersect_tris(pkg, algo):
    """((1 x + 0 y) + 0 z) + 0 == x as a value: the prim sets are bvh_intersect_tris's on the BLAS for every query"""
    meshes, _, _, _ = tris_exact_inputs(pkg, 1)
    mesh, other = meshes[0], meshes[3]
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(algo, mesh)
        assert b.result.layout == (0 if algo == 1 else 1)
        foff, fprims = b.intersect_tris(other)
        scene = pkg.Scene(sc_ctx).build(3, [b], make_instances(pkg, [identity()], [0]))
        off, recs = scene.intersect_tris(other)
        assert len(recs) > 100 and (recs["instance"] == 0).all()
        assert off.tobytes() == foff.tobytes() and recs["prim"].tobytes() == sorted_slices(foff, fprims).tobytes()
        ref_off, ref_prims = csr_of(tris_brute_force(other, mesh))
        assert off.tobytes() == ref_off.tobytes() and recs["prim"].tobytes() == ref_prims.tobytes()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_slices_are_a_subset_of_scene_overlap_and_instance_rows_are_symmetric(pkg):
    meshes, inst, q, ref = tris_exact_inputs(pkg, 64)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        scene = pkg.Scene(sc_ctx).build(2, four_blases(pkg, bl, meshes), inst)
        off, recs = scene.intersect_tris(as_triangles(pkg, q))
        boff, brecs = scene.overlap(stage_e_boxes(q))
        narrow = set(zip(slice_queries(off).tolist(), recs["instance"].tolist(), recs["prim"].tolist()))
        broad = set(zip(slice_queries(boff).tolist(), brecs["instance"].tolist(), brecs["prim"].tolist()))
        assert len(narrow) == ref["offsets"][-1] > 0 and narrow < broad and len(broad) == ref["box_pairs"]
        # (l, j) is in row i of INSTANCE(k) iff (k, i) is in row j of INSTANCE(l), over every instance l that INSTANCE(k) names
        k = 3
        koff, krecs = scene.intersect_tris(instance=k)
        fwd = set(zip(slice_queries(koff).tolist(), krecs["instance"].tolist(), krecs["prim"].tolist()))
        back = set()
        for l in sorted(set(krecs["instance"].tolist())):
            loff, lrecs = scene.intersect_tris(instance=l)
            sel = lrecs["instance"] == k
            back |= set(zip(lrecs["prim"][sel].tolist(), [l] * int(sel.sum()), slice_queries(loff)[sel].tolist()))
        assert fwd == back and len(fwd) >= 50 and len(set(krecs["instance"].tolist())) >= 2
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- independence, depth and updates ----------------------------------------------------------------------------------------------------------------------------

def test_independent_of_builders(pkg):
    mesh, one, q, ref = tris_builders_inputs(pkg)
    tq = as_triangles(pkg, q)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, mesh, fmt=algo % 3) for algo in range(4)]
        outs = []
        for tl in range(4):                                               # top-level builders over the same BLAS
            outs.append((f"top-level builder {tl}", pkg.Scene(sc_ctx).build(tl, [blases[3]], one).intersect_tris(tq)))
        for b in range(3):                                                # BLAS builders (and layouts, and formats) of the same mesh
            outs.append((f"BLAS builder {b}", pkg.Scene(sc_ctx).build(3, [blases[b]], one).intersect_tris(tq)))
        for what, (off, recs) in outs:
            assert off.tobytes() == ref["offsets"].tobytes() and recs.tobytes() == ref["recs"].tobytes(), what
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("H,deep", [(300, True), (20, False)])
def test_deep_blas_takes_the_stackless_pass(pkg, H, deep):
    """the caterpillar under five instances: a sliver up through an instance needs about H / 2 stack entries in its BLAS.  H = 300 overflows the short stack in
    the count AND in the fill pass, in every wave beside queries that stay in it; H = 20 is the control on the same code path"""
    tris, nodes, root, n, inst, q, ref, need = tris_deep_inputs(pkg, H)
    assert ((need > QUERY_STACK).sum() >= 4) == deep and (deep or need.max() + len(inst) - 1 <= QUERY_STACK), need.max()
    c, sc_ctx = pkg.Context(0), pkg.Context(0)
    try:
        d_tris, d_nodes = c.upload(tris), c.upload(nodes)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
        mesh = DeviceMesh(pkg, sc_ctx, as_triangles(pkg, q))
        sc_ctx.set_profiling(2)
        off, recs = search(pkg, scene, mesh.inp, mesh.n, SCENE_TRIS_QUERY, 0, SCENE_TRIS_SORTED)   # (asserts that the count-only and the fill call agree)
        kt = sc_ctx.kernel_times()
        sc_ctx.set_profiling(0)
        mesh.free()
        assert {"k_scene_tris_count", "k_scene_tris_fill", "k_scene_tris_deep", "k_overlap_scan"} <= set(kt), sorted(kt)
        launches = {k: v[1] for k, v in kt.items()}                       # (search: a count-only call, then a call that counts and fills)
        assert launches["k_scene_tris_count"] == 2 and launches["k_scene_tris_fill"] == 1 and launches["k_overlap_scan"] == 2, launches
        assert launches["k_scene_tris_deep"] == 3, "k_scene_tris_deep does not follow every pass"
        check_scene_tris(off, recs, ref, True, f"caterpillar {H}")
        check_all_ways(pkg, scene, q, ref, f"caterpillar {H}", fmt=1)
        iref = scene_tris_brute_force(instance_queries([tris], inst, 2, n), [tris], inst, skip=2)     # (parallel copies 100 apart: nothing crosses)
        check_all_ways(pkg, scene, None, iref, f"caterpillar {H}, instance 2", instance=2, rows=n)
        scene.close(); d_nodes.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()


@pytest.mark.parametrize("tlas_algo", [2, 3])
def test_deep_top_level_takes_the_stackless_pass(pkg, tlas_algo):
    """180 instances on the staircase: the PLOC-family top-level trees chain the steps up, and a triangle whose box covers them all pushes at every chain node"""
    mesh, inst, q, ref = tris_deep_top_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        scene = pkg.Scene(sc_ctx).build(tlas_algo, [bl.add(3, mesh)], inst)
        t = scene.tlas()
        nodes = np.empty(t.n_leaves - 1, dtype=pkg.BVH2_NODE); leaves = np.empty(t.n_leaves, dtype=pkg.PRIMREF)
        assert t.n_leaves == 180 and t.layout == 1
        assert pkg.lib().bvh_download(sc_ctx.handle, C.byref(t), nodes.ctypes.data, leaves.ctypes.data, None, None, None) == 0
        top = combined(pkg, nodes, leaves)
        qb = stage_e_boxes(q)

        def top_need(i):
            with np.errstate(invalid="ignore"):
                passes = (qb["min"][i] <= top["max"]).all(axis=1) & (top["min"] <= qb["max"][i]).all(axis=1) & (top["min"] <= top["max"]).all(axis=1)
            return left_first_scene_need(top, int(t.root), 180, passes, True)
        deep_need, quiet_need = top_need(0), max(top_need(i) for i in range(len(q)) if i % 32)
        print(f"tlas algo {tlas_algo}: a covering triangle needs {deep_need} entries at the top level, the others at most {quiet_need}")
        assert deep_need > QUERY_STACK and quiet_need + 8 <= QUERY_STACK
        check_all_ways(pkg, scene, q, ref, f"deep top level, algo {tlas_algo}")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_update_after_moves_and_blas_refit(pkg):
    meshes, inst, moved, q, refit, ref_moved, ref_refit = tris_moved_inputs(pkg)
    tq = as_triangles(pkg, q)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        before = scene.intersect_tris(tq, count_only=True)
        scene.update(moved)
        off, recs = check_all_ways(pkg, scene, q, ref_moved, "after update")
        assert before.tobytes() != off.tobytes()
        foff, frecs = pkg.Scene(sc_ctx).build(3, blases, moved).intersect_tris(tq)
        assert foff.tobytes() == off.tobytes() and frecs.tobytes() == recs.tobytes(), "an updated and a freshly built scene differ"
        # an update from DEVICE memory that hands instance 4 the other BLAS: instance mode reads the BLAS index on the device, so its rows follow
        swapped = moved.copy(); swapped["blas"][4] = 1 - swapped["blas"][4]
        d_inst = sc_ctx.upload(swapped)
        scene.update((d_inst, len(swapped)))
        rows = max(len(t) for t in meshes)
        for what, arr in (("instance 4 with the other BLAS", swapped), ("instance 4 back", moved)):
            iref = scene_tris_brute_force(instance_queries(meshes, arr, 4, rows), meshes, arr, skip=4)
            assert iref["offsets"][-1] > 0
            check_all_ways(pkg, scene, None, iref, what, instance=4, rows=rows)
            d_inst.upload(moved)
            scene.update((d_inst, len(moved)))
        d_inst.free()
        blases[0].refit(refit[0])
        bl.ctxs[0].synchronize()                                          # (the refit ran on the BLAS's own stream: complete before the scene reads the root box)
        scene.update(moved)
        check_all_ways(pkg, scene, q, ref_refit, "after BLAS refit")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- passes, capacity, argument handling and memory hygiene -------------------------------------------------------------------------------------------------------

def small_scene(pkg, bl):
    mesh, inst, q, ref = tris_small_inputs(pkg)
    return mesh, bl.add(3, mesh), inst, q, ref


def test_passes_and_capacity(pkg):
    """the count-only pass, a capacity one record short (the fill is skipped, the offsets complete), the exact capacity (guards intact, the same bytes
    twice), a NULL total_out and n == 0.  NOT tested, here or for bvh_scene_overlap, whose sink, scan and tail this call shares: the saturation marks — the
    per-query counter stopping at 0xFFFFFFFD and a total of 2^32 or more saturating d_offsets and returning BVH_E_TOO_LARGE.  Either needs more than four
    thousand million crossing pairs in one call, each a leaf test in f64, which no test of a few seconds can make"""
    bl, ctx = Blases(pkg), pkg.Context(0)
    try:
        mesh, b, inst, q, ref = small_scene(pkg, bl)
        scene = pkg.Scene(ctx).build(2, [b], inst)
        dm = DeviceMesh(pkg, ctx, as_triangles(pkg, q))
        m = dm.n
        want = {flags: search(pkg, scene, dm.inp, m, SCENE_TRIS_QUERY, 0, flags) for flags in (SCENE_TRIS_SORTED, 0)}
        exp_off = want[0][0]
        total = int(exp_off[-1])
        assert total > 50 and want[SCENE_TRIS_SORTED][0].tobytes() == exp_off.tobytes()
        check_scene_tris(exp_off, want[SCENE_TRIS_SORTED][1], ref, True, "small scene")
        extra = 29
        guard_p = np.frombuffer(np.full((total + extra) * 8, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_PRIM)
        guard_o = np.full(m + 1 + extra, 0xA5A5A5A5, dtype=np.uint32)
        d_off, d_prims = ctx.upload(guard_o), ctx.upload(guard_p)
        go = lambda flags, prims, cap, tot=True: call(pkg, scene, dm.inp, m, SCENE_TRIS_QUERY, 0, flags, d_off.ptr, prims, cap, total=tot)
        for flags in (SCENE_TRIS_SORTED, 0):
            out = {}
            # count only: d_prims untouched, offsets complete, guard words past n_queries + 1 offsets intact
            d_off.upload(guard_o); d_prims.upload(guard_p)
            assert go(flags, None, 0) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_prims.download(pkg.INSTANCE_PRIM, total + extra).tobytes() == guard_p.tobytes()
            # capacity total - 1: the fill is skipped, d_offsets still complete, *total_out set
            d_off.upload(guard_o)
            assert go(flags, d_prims.ptr, total - 1) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_prims.download(pkg.INSTANCE_PRIM, total + extra).tobytes() == guard_p.tobytes()
            # the exact capacity is filled; guard records past the total intact; twice the same bytes
            for rnd in range(2):
                d_off.upload(guard_o); d_prims.upload(guard_p)
                assert go(flags, d_prims.ptr, total) == (0, total)
                o, p = d_off.download(np.uint32, m + 1 + extra), d_prims.download(pkg.INSTANCE_PRIM, total + extra)
                assert o[m + 1:].tobytes() == guard_o[m + 1:].tobytes() and p[total:].tobytes() == guard_p[total:].tobytes()
                assert o[: m + 1].tobytes() == exp_off.tobytes() and p[:total].tobytes() == want[flags][1].tobytes()
                out[rnd] = (o.tobytes(), p.tobytes())
            assert out[0] == out[1], "two identical calls give different bytes"
            # total_out == NULL: the same device bytes after a synchronize
            d_off.upload(guard_o); d_prims.upload(guard_p)
            rc, t = go(flags, d_prims.ptr, total + extra, tot=False)
            assert rc == 0 and t == 0xDEAD
            ctx.synchronize()
            assert (d_off.download(np.uint32, m + 1 + extra).tobytes(), d_prims.download(pkg.INSTANCE_PRIM, total + extra).tobytes()) == out[0]
        # n_queries == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        d_off.upload(guard_o); d_prims.upload(guard_p)
        assert call(pkg, scene, dm.inp, 0, SCENE_TRIS_QUERY, 0, SCENE_TRIS_SORTED, d_off.ptr, d_prims.ptr, total) == (0, 0)
        o = d_off.download(np.uint32, m + 1 + extra)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes() and d_prims.download(pkg.INSTANCE_PRIM, total + extra).tobytes() == guard_p.tobytes()
        # the binding's capacity protocol: a capacity that is too small is re-allocated from the reported total
        qoff, qrecs = scene.intersect_tris(as_triangles(pkg, q), sorted=False, capacity=3)
        assert qoff.tobytes() == exp_off.tobytes() and qrecs.tobytes() == want[0][1].tobytes()
        scene.close(); dm.free(); d_off.free(); d_prims.free()
    finally:
        bl.close(); ctx.close()


def test_one_instance_on_a_fresh_ctx(pkg):
    """a one-instance scene builds no top-level tree, so a fresh ctx has no arena yet: the first call reserves the smallest one"""
    mesh, inst, q, _ = tris_small_inputs(pkg)
    one = inst[1:].copy()
    ref = scene_tris_brute_force(q, [mesh], one)
    assert ref["offsets"][-1] > 0
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        scene = pkg.Scene(sc_ctx).build(3, [bl.add(2, mesh)], one)
        off, recs = scene.intersect_tris(as_triangles(pkg, q))
        check_scene_tris(off, recs, ref, True, "fresh ctx")
        ioff = scene.intersect_tris(instance=0, count_only=True)         # nobody else to cross: every row empty
        assert len(ioff) == len(mesh) + 1 and not ioff.any()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_errors_write_nothing(pkg):
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    L = pkg.lib()
    try:
        mesh, b, inst, q, ref = small_scene(pkg, bl)
        tq = as_triangles(pkg, q)
        dm = {fmt: DeviceMesh(pkg, sc_ctx, tq, fmt) for fmt in (0, 1, 2)}
        m = len(q)
        cap = int(ref["offsets"][-1]) + 64
        guard_p = np.frombuffer(np.full(cap * 8, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_PRIM)
        guard_o = np.full(m + 1, 0x5A5A5A5A, dtype=np.uint32)
        prims, offs = sc_ctx.upload(guard_p), sc_ctx.upload(guard_o)
        tot = C.c_uint64(0x77)
        unbuilt, scene = pkg.Scene(sc_ctx), pkg.Scene(sc_ctx).build(2, [b], inst)
        NONE = object()

        def go(sc=scene, qin=dm[0].inp, n=m, mode=SCENE_TRIS_QUERY, k=0, flags=SCENE_TRIS_SORTED, o=offs.ptr, h=prims.ptr, c=cap):
            return L.bvh_scene_intersect_tris(sc.handle if sc is not None else None, C.byref(qin) if qin is not NONE else None, n, mode, k, flags, o, h, c, C.byref(tot))

        def inp(fmt, tris=None, verts=None, idx=None, nv=0):
            return pkg.BuildInput(fmt, 30, tris, verts, idx, nv, 0)
        tris_ptr, (v_ptr, i_ptr), nv = dm[0].bufs[0].ptr, (dm[2].bufs[0].ptr, dm[2].bufs[1].ptr), dm[2].inp.n_vertices
        cases = {
            "null scene": go(sc=None), "unbuilt scene": go(sc=unbuilt), "null offsets": go(o=None),
            "flag 2": go(flags=2), "flag 3": go(flags=3), "flag high": go(flags=0x80000000),
            "n_queries 2^30": go(n=1 << 30),
            "mode 2": go(mode=2), "mode -1": go(mode=-1),
            "query mode without queries": go(qin=NONE), "instance mode with queries": go(mode=SCENE_TRIS_INSTANCE),
            "query_instance = n_instances": go(qin=NONE, mode=SCENE_TRIS_INSTANCE, k=len(inst)), "query_instance huge": go(qin=NONE, mode=SCENE_TRIS_INSTANCE, k=0xFFFFFFFF),
            "query mode with query_instance 1": go(k=1),
            "unknown format": go(qin=inp(7, tris_ptr)), "padded without triangles": go(qin=inp(0)), "packed misaligned": go(qin=inp(1, dm[1].bufs[0].ptr + 4)),
            "indexed without vertices": go(qin=inp(2, None, None, i_ptr, nv)), "indexed without indices": go(qin=inp(2, None, v_ptr, None, nv)),
            "indexed with no vertices": go(qin=inp(2, None, v_ptr, i_ptr, 0)),
            "offsets in the triangles": go(o=tris_ptr + 64), "prims in the triangles": go(h=tris_ptr + 64 * (m - 1)),
            "prims in the packed triangles": go(qin=dm[1].inp, h=dm[1].bufs[0].ptr + 8), "prims in the vertices": go(qin=dm[2].inp, h=v_ptr + 8),
            "offsets in the indices": go(qin=dm[2].inp, o=i_ptr + 12 * (m - 1)),
            "prims in offsets": go(h=offs.ptr + 16), "offsets in prims": go(o=prims.ptr + 8 * (cap - 1)),
            "prims over the triangles, capacity clamped": go(h=tris_ptr - 16, c=1 << 40),
            "unbuilt, n_queries 0": go(sc=unbuilt, n=0),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        assert tot.value == 0x77
        sc_ctx.synchronize()
        assert prims.download(pkg.INSTANCE_PRIM, cap).tobytes() == guard_p.tobytes() and offs.download(np.uint32, m + 1).tobytes() == guard_o.tobytes()
        assert dm[0].bufs[0].download(pkg.meshgen.TRIANGLE, m).tobytes() == np.ascontiguousarray(tq).tobytes()
        # a count-only call ignores the capacity's range, and the scene still answers — in every query format
        assert go(h=None, c=1 << 40) == 0 and tot.value == ref["offsets"][-1]
        total = tot.value
        assert offs.download(np.uint32, m + 1)[-1] == total and prims.download(pkg.INSTANCE_PRIM, cap).tobytes() == guard_p.tobytes()
        for fmt in (0, 1, 2):
            prims.upload(guard_p)
            assert go(qin=dm[fmt].inp) == 0 and tot.value == total
            got = prims.download(pkg.INSTANCE_PRIM, cap)
            assert got[total:].tobytes() == guard_p[total:].tobytes()
            check_scene_tris(offs.download(np.uint32, m + 1), got[:total], ref, True, f"after the errors, format {fmt}")
        # n_queries == 0 on a built scene: d_offsets[0] = 0 and *total_out = 0
        offs.upload(guard_o)
        assert go(n=0) == 0 and tot.value == 0
        o = offs.download(np.uint32, m + 1)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes()
        scene.close(); unbuilt.close(); prims.free(); offs.free()
        for d in dm.values():
            d.free()
    finally:
        bl.close(); sc_ctx.close()


def test_binding_takes_every_input_kind(pkg):
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        mesh, b, inst, q, ref = small_scene(pkg, bl)
        tq = as_triangles(pkg, q)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        want_o, want_r = scene.intersect_tris(tq)
        assert want_o.shape == (len(q) + 1,) and want_o.dtype == np.uint32 and want_r.dtype == pkg.INSTANCE_PRIM == INSTANCE_PRIM and len(want_r) == want_o[-1] > 50
        check_scene_tris(want_o, want_r, ref, True, "binding")
        dm = {fmt: DeviceMesh(pkg, sc_ctx, tq, fmt) for fmt in (0, 1, 2)}
        for o, r in (scene.intersect_tris(q), scene.intersect_tris(q.reshape(-1, 9)), scene.intersect_tris(q.astype(np.float64)),
                     scene.intersect_tris(dm[0].bufs[0]), scene.intersect_tris(dm[0].bufs[0].ptr, n=len(q)),
                     scene.intersect_tris(dm[1].bufs[0], tri_format=pkg.TRI_PACKED36),
                     scene.intersect_tris(vertices=dm[2].bufs[0], indices=dm[2].bufs[1], n_vertices=dm[2].inp.n_vertices, tri_format=pkg.TRI_INDEXED),
                     scene.intersect_tris(tq, capacity=len(want_r) + 5), scene.intersect_tris(tq, capacity=1)):
            assert o.tobytes() == want_o.tobytes() and r.tobytes() == want_r.tobytes()
        assert scene.intersect_tris(dm[0].bufs[0], count_only=True).tobytes() == want_o.tobytes()
        uo, ur = scene.intersect_tris(dm[0].bufs[0], sorted=False)
        check_scene_tris(uo, ur, ref, False, "binding, unsorted")
        iref = scene_tris_brute_force(instance_queries([mesh], inst, 1, len(mesh)), [mesh], inst, skip=1)
        io, ir = scene.intersect_tris(instance=1)
        check_scene_tris(io, ir, iref, True, "binding, instance 1")
        assert scene.intersect_tris(instance=1, n=40, count_only=True).tobytes() == io[:41].tobytes()
        for d in dm.values():
            d.free()
        for bad in (lambda: scene.intersect_tris(np.zeros((4, 5), dtype=F32)), lambda: scene.intersect_tris(4096), lambda: scene.intersect_tris(),
                    lambda: scene.intersect_tris(tq, instance=0), lambda: scene.intersect_tris(instance=2)):
            with pytest.raises(pkg.BvhError):
                bad()
        eo, er = scene.intersect_tris(tq[:0])
        assert eo.tolist() == [0] and len(er) == 0 and er.dtype == pkg.INSTANCE_PRIM and scene.intersect_tris(tq[:0], count_only=True).tolist() == [0]
        scene.close()
    finally:
        bl.close(); sc_ctx.close()
