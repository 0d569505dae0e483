"""bvh_scene_knn on the GPU: the k nearest (dist2, instance, prim) lists against the two-level numpy brute force (tests/test_scene_knn.py, which also makes the
inputs and checks their premises without a device) for 1 to 64 instances over BLASes of every builder and triangle format, sheared and far-offset instances,
k = 1 against bvh_scene_closest_point, one identity instance against bvh_knn, coincident instances, independence from the builders, deep BLASes through the
stackless pass, bvh_scene_update after moves and after a BLAS refit, the binding's input kinds, rejections and buffer hygiene."""
import numpy as np
import pytest

from test_gpu_point_query import first_descent_pushes
from test_gpu_scene import TLAS_ALGO, Blases, root_boxes, world_tris
from test_query import E_INVALID
from test_scene import tris_root_box
from test_scene_knn import (DEEP_OFFSETS, EXACT_KS, MAX_K, builders_inputs, coincident_inputs, deep_inputs, exact_inputs, flat_entries_well, inactive_of,
                            kinds_inputs, moved_inputs, scene_knn_below, scene_knn_brute_force, scene_knn_recompute, scene_knn_truncate, small_inputs,
                            sponza_inputs)
from test_scene_point import scene_points

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]


def cut(pkg, bf, k):
    return bf if k == bf["hits"].shape[1] else scene_knn_truncate(pkg, bf, k)


def same_root_boxes(pkg, blases, blas_tris):
    """the brute force's world boxes come from the triangles' bounds: the built trees' root boxes must be those, bit for bit"""
    for got, t in zip(root_boxes(pkg, blases), blas_tris):
        assert got.tobytes() == tris_root_box(t).tobytes()


def check_exact(pkg, pts, blas_tris, inst, bf, hits, counts, what):
    """byte-equal lists and equal counts on the well-conditioned queries (at least 99 % of them); on every query each entry is an accepted candidate with
    bit-equal dist2 in strictly ascending order with the right padding, and no list is below the brute force's"""
    k = hits.shape[1]
    well = bf["well"]
    print(f"{what}, k = {k}: {well.sum()} of {len(well)} well-conditioned, {np.count_nonzero(bf['counts'] < k)} partial lists, {bf['kth_tie'].sum()} ties at place k")
    assert well.mean() >= 0.99, f"{what}: only {well.mean():.4f} of the queries are well-conditioned"
    same = (hits.view(np.uint8).reshape(len(pts), -1) == bf["hits"].view(np.uint8).reshape(len(pts), -1)).all(axis=1)
    bad = np.nonzero(~same & well)[0]
    assert bad.size == 0, f"{what}, k = {k}: {bad.size} well-conditioned lists differ, e.g. query {bad[0]}: got {hits[bad[0]]} want {bf['hits'][bad[0]]}"
    assert np.array_equal(counts[well], bf["counts"][well]), f"{what}, k = {k}: counts differ"
    assert scene_knn_recompute(pkg, pts, blas_tris, inst, hits, counts).all(), f"{what}, k = {k}: an entry is not an accepted candidate, or order / padding / count is wrong"
    assert not scene_knn_below(pkg, hits, bf["hits"]).any(), f"{what}, k = {k}: a list below the brute force"


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_inst", [1, 2, 3, 64])
def test_exact_against_brute_force(pkg, n_inst):
    meshes, inst, pts, bf32 = exact_inputs(pkg, n_inst)
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo], fmt=algo % 3) for algo in range(4)]
        same_root_boxes(pkg, blases, meshes)
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[n_inst], blases, inst)
        partial = ties = 0
        for k in EXACT_KS:
            bf = cut(pkg, bf32, k)
            hits, counts = scene.knn(pts, k)
            check_exact(pkg, pts, meshes, inst, bf, hits, counts, f"{n_inst} instances")
            assert not set(hits["instance"][hits["prim"] != pkg.INVALID].tolist()) & inactive_of(n_inst), "an inactive instance answered"
            partial += np.count_nonzero((counts > 0) & (counts < k)); ties += np.count_nonzero(bf["kth_tie"] & bf["well"])
        assert partial > 0, "no partial list"
        if n_inst == 64:                                          # (instances 0, 20 and 40 coincide: lists end inside their ties; the meshes of
                                                                  # the smaller scenes have no two candidates at one distance)
            assert ties > 0, "no list has its k-th entry tied on dist2"
        if n_inst == 3:                                           # 65 points: a partial last wave
            _, _, pts65, bf65 = exact_inputs(pkg, 3, m=65)
            for k in (5, 32):
                hits, counts = scene.knn(pts65, k)
                check_exact(pkg, pts65, meshes, inst, cut(pkg, bf65, k), hits, counts, "65 points")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("kind", ["shear", "far"])
def test_anisotropic_and_far_offset_instances(pkg, kind):
    """every instance is rotation x diag(0.25 .. 4) x shear x rotation ("shear": object-space distances are off by up to 16x either way), or rigid with
    translations up to 4096 ("far": the mapped point carries an absolute error that dwarfs a near-surface distance); the bound comes from the list's last
    entry, not from the best candidate"""
    mesh, inst, pts, bf32 = kinds_inputs(pkg, kind)
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        same_root_boxes(pkg, [b], [mesh])
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        hits, counts = scene.knn(pts, 8)
        assert (counts == 8).all()
        check_exact(pkg, pts, [mesh], inst, cut(pkg, bf32, 8), hits, counts, kind)
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_k1_equals_scene_closest_point(pkg):
    """(dist2, prim, instance) of every query, well-conditioned or not: the walk is k_scene_closest_point's"""
    meshes, inst, pts, _ = exact_inputs(pkg, 64)
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo], fmt=algo % 3) for algo in range(4)]
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[64], blases, inst)
        ref = scene.closest_point(pts, query="closest")
        hits, counts = scene.knn(pts, 1)
        got = hits[:, 0]
        assert got["dist2"].tobytes() == ref["dist2"].tobytes() and np.array_equal(got["prim"], ref["prim"]) and np.array_equal(got["instance"], ref["instance"])
        assert np.array_equal(counts, (ref["prim"] != pkg.INVALID).astype(np.uint32)) and 20 < counts.sum() < len(pts) - 20
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("algo", [1, 3])
def test_one_identity_instance_equals_knn(pkg, algo):
    mesh, inst, pts, bf32 = sponza_inputs(pkg)
    bf = cut(pkg, bf32, 8)
    well = bf["well"] & flat_entries_well(pkg, pts, mesh, bf["hits"])             # well-conditioned for both queries
    assert well.mean() >= 0.99
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        b = bl.add(algo, mesh)
        assert b.result.layout == (0 if algo == 1 else 1)
        ref, ref_counts = b.knn(pts, 8)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        hits, counts = scene.knn(pts, 8)
        for f in ("dist2", "prim"):
            bad = np.nonzero((hits[f].view(np.uint32) != ref[f].view(np.uint32)).any(axis=1) & well)[0]
            assert bad.size == 0, f"{f} differs on {bad.size} well-conditioned queries, e.g. {bad[:4]}: scene {hits[bad[:4]]} knn {ref[bad[:4]]}"
        assert np.array_equal(counts[well], ref_counts[well])
        valid = hits["prim"] != pkg.INVALID
        assert (hits["instance"][valid] == 0).all() and (hits["instance"][~valid] == pkg.INVALID).all()
        check_exact(pkg, pts, [mesh], inst, bf, hits, counts, f"sponza, algo {algo}")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("tlas_algo", [0, 3])
def test_coincident_instances_alternate(pkg, tlas_algo):
    """two instances place the same triangles identically, so every dist2 comes twice; one BLAS also holds a far-off extra triangle that stretches its world
    box, so the two are not walked alike.  Every list is (d, 0, p), (d, 1, p), ... whichever BLAS is the stretched one."""
    mesh, stretched, inst, pts = coincident_inputs(pkg, tlas_algo)
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        plain, far = bl.add(3, mesh), bl.add(1, stretched)
        for order in ((plain, far), (far, plain)):
            blas_tris = [mesh, stretched] if order[0] is plain else [stretched, mesh]
            hits, counts = pkg.Scene(sc_ctx).build(tlas_algo, list(order), inst).knn(pts, 6)
            bf = scene_knn_brute_force(pkg, pts, blas_tris, inst, 6, root_boxes(pkg, list(order)))
            assert (counts == 6).all() and bf["well"].all()
            assert (hits["instance"] == np.array([0, 1, 0, 1, 0, 1])[None]).all(), "a tie went to the higher instance first"
            assert np.array_equal(hits["prim"][:, 0::2], hits["prim"][:, 1::2]) and hits["dist2"][:, 0::2].tobytes() == hits["dist2"][:, 1::2].tobytes()
            assert hits.tobytes() == bf["hits"].tobytes()
    finally:
        bl.close(); sc_ctx.close()


# ---- independence, depth and updates ----------------------------------------------------------------------------------------------------------------------------

def test_independent_of_builders(pkg):
    mesh, inst, pts, bf, _ = builders_inputs(pkg)
    assert bf["well"].all()
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(algo, mesh) for algo in range(4)]
        same_root_boxes(pkg, blases, [mesh] * 4)
        outs = []
        for tl in range(4):                                   # top-level builders over the same BLAS
            outs.append(pkg.Scene(sc_ctx).build(tl, [blases[3]], inst).knn(pts, 16))
        for b in range(3):                                    # BLAS builders of the same mesh
            outs.append(pkg.Scene(sc_ctx).build(3, [blases[b]], inst).knn(pts, 16))
        assert outs[0][0].tobytes() == bf["hits"].tobytes() and np.array_equal(outs[0][1], bf["counts"])
        for h, c in outs[1:]:
            assert h.tobytes() == outs[0][0].tobytes() and np.array_equal(c, outs[0][1])
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("H", [70, 250])
def test_deep_blas_takes_the_stackless_pass(pkg, H):
    tris, nodes, root, n, inst, pts, bf8 = deep_inputs(pkg, H)
    offs = np.array(DEEP_OFFSETS, dtype=np.float64)
    m = len(pts)
    # an unbounded query passes every box until its list is full, so whichever instance it enters first its first descent there pushes one entry per chain
    # node: more than the short stack holds
    pushes = [min(first_descent_pushes(nodes, root, n - 1, pts["point"][j].astype(np.float64) - t) for t in offs) for j in range(m // 2)]
    assert max(pushes) > 64
    c = pkg.Context(0)
    sc_ctx = pkg.Context(0)
    try:
        d_nodes, d_tris = c.upload(nodes), c.upload(tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
        for k in (1, 8):
            bf = cut(pkg, bf8, k)
            assert bf["well"].all()
            sc_ctx.set_profiling(2)
            hits, counts = scene.knn(pts, k)
            kt = sc_ctx.kernel_times()
            sc_ctx.set_profiling(0)
            assert {"k_scene_knn", "k_scene_knn_deep"} <= set(kt)
            assert hits.tobytes() == bf["hits"].tobytes() and np.array_equal(counts, bf["counts"]), f"k = {k}"
        scene.close(); d_nodes.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()


def test_update_after_moves_and_blas_refit(pkg):
    meshes, inst, moved, pts, refit, bf_moved, bf_refit = moved_inputs(pkg)
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        scene.update(moved)
        same_root_boxes(pkg, blases, meshes)
        hits, counts = scene.knn(pts, 8)
        check_exact(pkg, pts, meshes, moved, cut(pkg, bf_moved, 8), hits, counts, "after update")
        fresh, fresh_counts = pkg.Scene(sc_ctx).build(3, blases, moved).knn(pts, 8)
        assert fresh.tobytes() == hits.tobytes() and np.array_equal(fresh_counts, counts)
        blases[0].refit(refit[0])
        bl.ctxs[0].synchronize()                              # (the refit ran on the BLAS's own stream: complete before the scene reads the root box)
        scene.update(moved)
        same_root_boxes(pkg, blases, refit)
        hits, counts = scene.knn(pts, 8)
        check_exact(pkg, pts, refit, moved, cut(pkg, bf_refit, 8), hits, counts, "after BLAS refit")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- argument handling and memory hygiene -------------------------------------------------------------------------------------------------------------------------

def small_scene(pkg, bl):
    mesh, inst, pts, bf32 = small_inputs(pkg)
    return mesh, bl.add(3, mesh), inst, pts, bf32


def test_binding_takes_every_input_kind(pkg):
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        mesh, b, inst, _, _ = small_scene(pkg, bl)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        xyz = np.ascontiguousarray(scene_points(pkg, world_tris(pkg, [mesh], inst), 256, 4, bounded=False)["point"])
        rec = np.zeros(256, dtype=pkg.POINT_QUERY); rec["point"] = xyz; rec["radius"] = 0.5
        want_h, want_c = scene.knn(rec, 5)
        assert want_h.shape == (256, 5) and want_h.dtype == pkg.INSTANCE_KNN_HIT and want_c.shape == (256,) and 0 < (want_c < 5).sum() < 256
        assert scene_knn_recompute(pkg, rec, [mesh], inst, want_h, want_c).all()
        d = sc_ctx.upload(rec)
        for h, c in (scene.knn(xyz, 5, radius=0.5), scene.knn(d, 5), scene.knn(d.ptr, 5, n_points=256)):
            assert h.tobytes() == want_h.tobytes() and np.array_equal(c, want_c)
        d.free()
        with pytest.raises(pkg.BvhError):
            scene.knn(rec, 5, radius=1.0)
        for k in (0, 33):
            with pytest.raises(pkg.BvhError):
                scene.knn(rec, k)
        unbounded, _ = scene.knn(xyz, 3)
        assert (unbounded["prim"] != pkg.INVALID).all()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_rejections_and_hygiene(pkg):
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    L = pkg.lib()
    try:
        mesh, b, inst, pts, bf32 = small_scene(pkg, bl)
        scene = pkg.Scene(sc_ctx)
        n, k = len(pts), 5
        d_pts = sc_ctx.upload(pts)
        pad = 32
        hb, cb = (n * k + 2 * pad) * 16, (n + 2 * pad) * 4
        hits, counts = sc_ctx.alloc(hb), sc_ctx.alloc(cb)
        pat_h, pat_c = np.full(hb, 0xAB, dtype=np.uint8), np.full(cb, 0xCD, dtype=np.uint8)
        hits.upload(pat_h); counts.upload(pat_c)
        h, c = hits.ptr + pad * 16, counts.ptr + pad * 4
        assert L.bvh_scene_knn(scene.handle, d_pts.ptr, n, k, h, c) == E_INVALID                       # not built
        scene.build(2, [b], inst)
        assert L.bvh_scene_knn(None, d_pts.ptr, n, k, h, c) == E_INVALID
        assert L.bvh_scene_knn(scene.handle, None, n, k, h, c) == E_INVALID
        assert L.bvh_scene_knn(scene.handle, d_pts.ptr, n, k, None, c) == E_INVALID
        assert L.bvh_scene_knn(scene.handle, d_pts.ptr, n, 0, h, c) == E_INVALID
        assert L.bvh_scene_knn(scene.handle, d_pts.ptr, n, MAX_K + 1, h, c) == E_INVALID
        assert L.bvh_scene_knn(scene.handle, d_pts.ptr, 1 << 28, 16, h, c) == E_INVALID                # n_points * k == 2^32
        assert L.bvh_scene_knn(scene.handle, d_pts.ptr, 0xFFFFFFFF, 2, h, c) == E_INVALID
        assert L.bvh_scene_knn(scene.handle, d_pts.ptr, n, k, d_pts.ptr + 16, c) == E_INVALID          # hits over the points
        assert L.bvh_scene_knn(scene.handle, h + 16 * (n * k - 1), n, k, h, c) == E_INVALID            # points inside the last record
        assert L.bvh_scene_knn(scene.handle, d_pts.ptr, n, k, h, d_pts.ptr + 16 * (n - 1) + 12) == E_INVALID   # counts over the last point
        assert L.bvh_scene_knn(scene.handle, d_pts.ptr, n, k, h, h + 16 * n * k - 4) == E_INVALID      # counts over the last record
        assert L.bvh_scene_knn(scene.handle, d_pts.ptr, n, k, c - 16 * n * k + 4, c) == E_INVALID      # the last record over the first count
        assert L.bvh_scene_knn(scene.handle, d_pts.ptr, 0, k, h, c) == 0
        sc_ctx.synchronize()
        assert np.array_equal(hits.download(np.uint8, hb), pat_h), "an error or n_points == 0 wrote to the hits"
        assert np.array_equal(counts.download(np.uint8, cb), pat_c), "an error or n_points == 0 wrote to the counts"
        same_root_boxes(pkg, [b], [mesh])
        bf = cut(pkg, bf32, k)
        assert bf["well"].mean() >= 0.99
        runs = []
        for use_counts in (True, True, False):
            hits.upload(pat_h); counts.upload(pat_c)
            assert L.bvh_scene_knn(scene.handle, d_pts.ptr, n, k, h, c if use_counts else None) == 0
            sc_ctx.synchronize()
            got_h, got_c = hits.download(np.uint8, hb), counts.download(np.uint8, cb)
            assert np.array_equal(got_h[: pad * 16], pat_h[: pad * 16]) and np.array_equal(got_h[-pad * 16:], pat_h[-pad * 16:]), "a guard word of d_hits"
            assert np.array_equal(got_c[: pad * 4], pat_c[: pad * 4]) and np.array_equal(got_c[-pad * 4:], pat_c[-pad * 4:]), "a guard word of d_counts"
            rec = np.frombuffer(got_h[pad * 16: -pad * 16].tobytes(), dtype=pkg.INSTANCE_KNN_HIT).reshape(n, k)
            cnt = np.frombuffer(got_c[pad * 4: -pad * 4].tobytes(), dtype=np.uint32)
            if not use_counts:
                assert np.array_equal(got_c, pat_c), "d_counts == NULL wrote counts"
            assert (rec["reserved"] == 0).all()
            assert scene_knn_recompute(pkg, pts, [mesh], inst, rec, cnt if use_counts else None).all()
            assert rec[bf["well"]].tobytes() == bf["hits"][bf["well"]].tobytes()
            if use_counts:
                assert np.array_equal(cnt[bf["well"]], bf["counts"][bf["well"]])
            assert d_pts.download(pkg.POINT_QUERY, n).tobytes() == pts.tobytes()
            runs.append(rec.tobytes())
        assert runs[0] == runs[1] == runs[2], "the same call twice gives other bytes"
        scene.close(); d_pts.free(); hits.free(); counts.free()
    finally:
        bl.close(); sc_ctx.close()
