"""bvh_scene_closest_tris on the GPU: nearest-triangle and any-within-radius answers on instanced scenes against the two-level numpy brute force
(tests/test_scene_closest_tris.py): 1 to 64 instances over BLASes of every builder, layout and format, in both modes (a world-space query mesh; the triangles
of one instance, looked up on the device); sheared, far-offset and mirrored instances; one identity instance against bvh_closest_tris; consistency with
bvh_scene_intersect_tris; independence from the builders; a deep BLAS and a deep top level through the stackless pass, each with a short-tree control;
bvh_scene_update after moves (from host and from device memory) and after a BLAS refit; coincident instances; rejections, buffer hygiene and the binding.
The pair matrix of an input (every query triangle against every world triangle, 15 terms each) is computed once and shared across radii, kinds and builders."""
import ctypes as C

import numpy as np
import pytest

from test_closest_tris import CROSSING, E_INVALID
from test_deep_trees import QUERY_STACK, combined
from test_gpu_closest_tris import NAN_QUERIES, make_queries, raw as flat_raw
from test_gpu_intersect_tris import DeviceMesh
from test_gpu_point_query import first_descent_pushes
from test_gpu_query import caterpillar, mesh as named_mesh
from test_gpu_refit import jitter, no_negzero
from test_gpu_scene import MESH_SIZES, TLAS_ALGO, Blases, root_boxes, scene_instances
from test_gpu_scene_intersect_tris import INSTANCE_CASES, four_blases
from test_gpu_scene_point import with_shear
from test_intersect_tris import as_triangles, stage_e_boxes, xyz
from test_scene import identity, make_instances, mat34, rot
from test_scene_closest_tris import (SCENE_TRIS_INSTANCE, SCENE_TRIS_QUERY, scene_pair_matrix, scene_tri_miss_records, scene_tris_dist_brute_force,
                                     scene_tris_dist_recompute, tris_dist_below)
from test_scene_intersect_tris import instance_queries, left_first_scene_need, tris_deep_top_inputs, tris_exact_inputs
from test_scene_knn import DEEP_OFFSETS, cached, inactive_of
from test_scene_point import flat_world_tris, instance_set

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32
BAND = 0.05
RADII = {"inf": np.inf, "band": BAND, "zero": 0.0, "negative": -1.0, "nan": np.nan}


def call(pkg, scene, qin, m, mode, k, radius, d_hits, kind):
    return pkg.lib().bvh_scene_closest_tris(scene.handle, C.byref(qin) if qin is not None else None, m, mode, k, radius, d_hits, kind)


def raw(pkg, scene, qin, m, mode, k, radius, kind):
    hits = scene.ctx.alloc(m * 16)
    try:
        rc = call(pkg, scene, qin, m, mode, k, radius, hits.ptr, kind)
        assert rc == 0, rc
        return hits.download(pkg.INSTANCE_TRI_HIT, m)
    finally:
        hits.free()


def check_exact(pkg, q, blas_tris, inst, radius, bf, closest, anyhit, what, skip=None, inactive=()):
    """test_gpu_closest_tris.check_exact on scene records: bytes equal on well-conditioned queries, any-hit hit / miss equal on them, recompute and not-below
    on every query, no inactive (or skipped) instance answers"""
    well = bf["well"]
    print(f"{what}: {well.sum()} of {len(well)} well-conditioned, {bf['hit'].sum()} hits, {(bf['closest']['feature'] == CROSSING).sum()} crossings, "
          f"{len(set(bf['closest']['instance'][bf['hit']].tolist()))} instances answer")
    assert well.mean() >= 0.99, f"{what}: only {well.mean():.4f} of the queries are well-conditioned"
    ref = bf["closest"]
    diff = (closest.view(np.uint8).reshape(-1, 16) != ref.view(np.uint8).reshape(-1, 16)).any(axis=1)
    assert not (diff & well).any(), (f"{what}: closest differs on {np.count_nonzero(diff & well)} well-conditioned queries (first {np.nonzero(diff & well)[0][:6]}: "
                                     f"got {closest[diff & well][:3]} want {ref[diff & well][:3]})")
    hit_any = anyhit["prim"] != pkg.INVALID
    assert (hit_any == bf["hit"])[well].all(), f"{what}: any hit/miss differs"
    for name, out in (("closest", closest), ("any", anyhit)):
        assert scene_tris_dist_recompute(pkg, q, blas_tris, inst, radius, out, skip=skip).all(), \
            f"{what}: a {name} record is not an accepted candidate of its (instance, prim) (or not the miss record)"
        answered = set(out["instance"][out["prim"] != pkg.INVALID].tolist())
        assert not answered & set(inactive), f"{what}: an inactive instance answered"
        assert skip is None or skip not in answered, f"{what}: the query instance answered"
    assert not tris_dist_below(pkg, closest, ref).any(), f"{what}: closest below the brute force"


def check_all_radii(pkg, scene, q, blas_tris, inst, pairs, rb, what, qin=None, mode=SCENE_TRIS_QUERY, k=0, radii=RADII, inactive=()):
    """both kinds at every radius against the brute force cut from one pair matrix; returns {label: (brute force, closest records)}"""
    skip = k if mode == SCENE_TRIS_INSTANCE else None
    out = {}
    for label, radius in radii.items():
        bf = scene_tris_dist_brute_force(pkg, q, blas_tris, inst, radius, skip=skip, pairs=pairs, root_boxes=rb)
        c = raw(pkg, scene, qin, len(q), mode, k, radius, pkg.QUERY_CLOSEST)
        a = raw(pkg, scene, qin, len(q), mode, k, radius, pkg.QUERY_ANY)
        check_exact(pkg, q, blas_tris, inst, radius, bf, c, a, f"{what} radius {label}", skip=skip, inactive=inactive)
        out[label] = (bf, c)
    return out


# ---- inputs (host side, computed once) --------------------------------------------------------------------------------------------------------------------------

def exact_inputs(pkg, n_inst, spacing=1.5):
    """test_gpu_scene_point.test_exact_against_brute_force's scene (four meshes of MESH_SIZES, every kind of instance, every sixth sheared, the trailing ones
    inactive) and test_gpu_closest_tris.make_queries' 768 triangles over its flattened world triangles -> (meshes, inst, queries, pair matrix)"""
    def make():
        rng = np.random.default_rng(n_inst)
        meshes = [no_negzero(pkg.meshgen.uniform(n, 31 + n)) for n in MESH_SIZES[n_inst]]
        inst = with_shear(pkg, rng, scene_instances(pkg, rng, n_inst, 4, spacing), n_inst - len(inactive_of(n_inst)))
        flat, _, _ = flat_world_tris(pkg, meshes, inst)
        q = make_queries(pkg, flat, 300 + n_inst)
        return meshes, inst, q, scene_pair_matrix(pkg, q, meshes, inst)
    return cached(("closest tris exact", n_inst, spacing), make)


def instance_inputs(pkg, n_inst, k, spacing):
    """INSTANCE(k) on exact_inputs' scene: rows up to the largest BLAS -> (meshes, inst, the rows as explicit triangles, pair matrix)"""
    def make():
        meshes, inst, _, _ = exact_inputs(pkg, n_inst, spacing)
        rows = as_triangles(pkg, instance_queries(meshes, inst, k, max(len(t) for t in meshes)))
        return meshes, inst, rows, scene_pair_matrix(pkg, rows, meshes, inst)
    return cached(("closest tris instance", n_inst, k, spacing), make)


def mirrored_set(pkg, rng, n_inst):
    mats = []
    for k in range(n_inst):
        R = rot(rng.integers(3), rng.uniform(0, 2 * np.pi)) @ rot(rng.integers(3), rng.uniform(0, 2 * np.pi))
        D = np.diag([-1.0, 1.0, 1.0]) if k % 2 else np.diag(-rng.uniform(0.5, 2.0, 3))
        mats.append(mat34(R @ D, rng.uniform(-3.0, 3.0, 3)))
    inst = make_instances(pkg, mats, [0] * n_inst)
    assert (np.linalg.det(inst["object_to_world"].reshape(-1, 3, 4)[:, :, :3].astype(np.float64)) < 0).all()
    return inst


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_inst", [1, 2, 3, 64])
def test_exact_against_brute_force_in_both_modes(pkg, n_inst):
    """1: no top-level tree; 2: a root with two leaf children; 3: the singular instance inactive; 64: all three kinds of inactive instance.  QUERY mode at
    spacing 1.5; INSTANCE mode at spacing 0.6 for 2 and 3 instances (at 1.5 hardly a pair lies inside the band and nothing crosses)"""
    meshes, inst, q, pairs = exact_inputs(pkg, n_inst)
    inactive = inactive_of(n_inst)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = four_blases(pkg, bl, meshes)
        rb = root_boxes(pkg, blases)
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[n_inst], blases, inst)
        dm = DeviceMesh(pkg, sc_ctx, q, n_inst % 3)
        got = check_all_radii(pkg, scene, q, meshes, inst, pairs, rb, f"{n_inst} instances", qin=dm.inp, inactive=inactive)
        dm.free()
        inf, band = got["inf"][0], got["band"][0]
        assert inf["hit"][:-NAN_QUERIES].all() and not inf["hit"][-NAN_QUERIES:].any()
        assert not got["negative"][0]["hit"].any() and not got["nan"][0]["hit"].any() and got["zero"][0]["hit"].any() and band["hit"].any() and not band["hit"].all()
        assert (inf["closest"]["feature"] == CROSSING).any()
        assert scene.closest_tris(q).tobytes() == got["inf"][1].tobytes()                       # the Python binding, a host mesh
        assert scene_tris_dist_recompute(pkg, q, meshes, inst, BAND, scene.closest_tris(q, radius=BAND, query="any")).all()
        if n_inst in (2, 3):                                                                    # the interpenetrating scene of the instance mode
            scene.close()
            meshes, inst, _, _ = exact_inputs(pkg, n_inst, 0.6)
            scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[n_inst], blases, inst)
        for k in INSTANCE_CASES[n_inst]:
            _, _, rows, ipairs = instance_inputs(pkg, n_inst, k, 0.6 if n_inst in (2, 3) else 1.5)
            igot = check_all_radii(pkg, scene, rows, meshes, inst, ipairs, rb, f"{n_inst} instances, instance {k}", mode=SCENE_TRIS_INSTANCE, k=k,
                                   radii={"inf": np.inf, "band": BAND, "negative": -1.0}, inactive=inactive)
            ibf = igot["inf"][0]
            if k in inactive or n_inst == 1:
                assert not ibf["hit"].any()                                                     # an inactive query instance, or nobody else to answer
            else:
                assert ibf["hit"][: len(meshes[int(inst["blas"][k])])].all() and not ibf["hit"][len(meshes[int(inst["blas"][k])]):].any()
            if n_inst in (2, 3) and k not in inactive:
                bh = igot["band"][0]["hit"][: len(meshes[int(inst["blas"][k])])]
                assert (ibf["closest"]["feature"] == CROSSING).any() and bh.any() and not bh.all(), "the instance rows lack a crossing, a band hit or a band miss"
            assert scene.closest_tris(instance=k).tobytes() == igot["inf"][1].tobytes()          # the binding: as many rows as the largest BLAS has leaves
            if n_inst == 3 and k == 1:                                                           # 65 rows: a partial last wave, fewer rows than the BLAS has leaves
                cut = raw(pkg, scene, None, 65, SCENE_TRIS_INSTANCE, k, np.inf, pkg.QUERY_CLOSEST)
                assert cut.tobytes() == igot["inf"][1][:65].tobytes()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("kind", ["shear", "far", "mirror"])
def test_sheared_far_offset_and_mirrored_instances(pkg, kind):
    """every instance is rotation x diag(0.25 .. 4) x shear x rotation ("shear": object-space distances are off by up to 16x either way), rigid with
    translations up to 4096 ("far": the mapped vertices carry an absolute error that dwarfs a near-contact distance) or a reflection ("mirror")"""
    rng = np.random.default_rng({"shear": 7, "far": 8, "mirror": 9}[kind])
    mesh = no_negzero(pkg.meshgen.uniform(300, 41))
    inst = mirrored_set(pkg, rng, 8) if kind == "mirror" else instance_set(pkg, rng, kind, 8)
    flat, _, _ = flat_world_tris(pkg, [mesh], inst)
    q = make_queries(pkg, flat, 9)
    pairs = scene_pair_matrix(pkg, q, [mesh], inst)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        dm = DeviceMesh(pkg, sc_ctx, q, 2)
        got = check_all_radii(pkg, scene, q, [mesh], inst, pairs, root_boxes(pkg, [b]), kind, qin=dm.inp, radii={"inf": np.inf})
        assert got["inf"][0]["hit"][:-NAN_QUERIES].all() and len(set(got["inf"][1]["instance"][:-NAN_QUERIES].tolist())) >= 4
        rows = as_triangles(pkg, instance_queries([mesh], inst, 5, len(mesh)))
        check_all_radii(pkg, scene, rows, [mesh], inst, scene_pair_matrix(pkg, rows, [mesh], inst), root_boxes(pkg, [b]), kind + ", instance 5",
                        mode=SCENE_TRIS_INSTANCE, k=5, radii={"inf": np.inf})
        dm.free(); scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- relations --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [1, 3])
def test_one_identity_instance_equals_closest_tris(pkg, algo):
    """((1 x + 0 y) + 0 z) + 0 == x as a value and W = identity maps the query onto itself: hit records byte for byte (the flat record's reserved 0 is
    instance 0), misses equal but for the last word"""
    tris = named_mesh(pkg, "uniform_1000")
    q = make_queries(pkg, tris, 1017)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(algo, tris)
        assert b.result.layout == (0 if algo == 1 else 1)
        scene = pkg.Scene(sc_ctx).build(3, [b], make_instances(pkg, [identity()], [0]))
        d_q = bl.ctxs[0].upload(q)
        for radius in (np.inf, 2e-3, 0.0):
            for kind in (pkg.QUERY_CLOSEST, pkg.QUERY_ANY):
                flat = flat_raw(pkg, bl.ctxs[0], b.result, d_q, len(q), radius, kind)
                got = scene.closest_tris(q, radius=radius, query=kind)
                hit = flat["prim"] != pkg.INVALID
                assert hit.any() and (~hit).any()
                assert got[hit].tobytes() == flat[hit].tobytes(), f"radius {radius} kind {kind}: hit records differ"
                assert got[~hit].view(np.uint32).reshape(-1, 4)[:, :3].tobytes() == flat[~hit].view(np.uint32).reshape(-1, 4)[:, :3].tobytes()
                assert (got["instance"][~hit] == pkg.INVALID).all()
        d_q.free(); scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_feature_15_rows_are_the_nonempty_rows_of_scene_intersect_tris(pkg):
    """on test_gpu_scene_intersect_tris' interpenetrating 64-instance scene, in both modes: a closest answer is a crossing iff the query crosses something
    (a row that crosses always answers dist2 0; its feature is 15 unless a candidate that TOUCHES it at exactly 0 has the lower key)"""
    meshes, inst, q, ref = tris_exact_inputs(pkg, 64)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        scene = pkg.Scene(sc_ctx).build(2, four_blases(pkg, bl, meshes), inst)
        tq = as_triangles(pkg, q)
        got = scene.closest_tris(tq)
        counts = np.diff(scene.intersect_tris(tq, count_only=True).astype(np.int64))
        # (every eighth query, and the last, is a copy of a world triangle: it touches its original at dist2 exactly 0 by a vertex term, and that candidate
        # wins the tie where its (instance, prim) is below the crossed triangle's — there, and only there, a crossing row may answer with another feature)
        cross, touching = got["feature"] == CROSSING, np.arange(len(q)) % 8 == 7
        touching[-1] = True
        assert np.array_equal(counts > 0, ref["counts"] > 0) and 50 < (counts > 0).sum() < len(q) - 50
        assert np.array_equal(cross[~touching], (counts > 0)[~touching])
        assert (counts[cross] > 0).all() and (got["dist2"][counts > 0] == 0).all() and (got["prim"][counts > 0] != pkg.INVALID).all()
        for k in (3, 62):                                                 # (62 is inactive: every row misses and every slice is empty)
            igot = scene.closest_tris(instance=k)
            icounts = np.diff(scene.intersect_tris(instance=k, count_only=True).astype(np.int64))
            assert len(igot) == len(icounts) and np.array_equal(igot["feature"] == CROSSING, icounts > 0)
            assert ((icounts > 0).sum() > 20) == (k == 3) and (k == 3 or (igot["prim"] == pkg.INVALID).all())
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- independence, depth and updates ----------------------------------------------------------------------------------------------------------------------------

def test_independent_of_builders(pkg):
    rng = np.random.default_rng(9)
    mesh = no_negzero(pkg.meshgen.uniform(200, 77))
    inst = with_shear(pkg, rng, scene_instances(pkg, rng, 64, 1, 1.2), 61)
    flat, _, _ = flat_world_tris(pkg, [mesh], inst)
    q = make_queries(pkg, flat, 5)[::3]
    pairs = scene_pair_matrix(pkg, q, [mesh], inst)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, mesh, fmt=algo % 3) for algo in range(4)]
        rb = root_boxes(pkg, blases[:1])
        for label, radius in (("inf", np.inf), ("band", BAND)):
            bf = scene_tris_dist_brute_force(pkg, q, [mesh], inst, radius, pairs=pairs, root_boxes=rb)
            well = bf["well"]
            assert well.mean() >= 0.99 and bf["hit"].sum() > 50
            outs = []
            for tl in range(4):                                           # top-level builders over the same BLAS
                outs.append((f"top-level builder {tl}", pkg.Scene(sc_ctx).build(tl, [blases[3]], inst).closest_tris(q, radius=radius)))
            for b in range(3):                                            # BLAS builders (and layouts, and formats) of the same mesh
                outs.append((f"BLAS builder {b}", pkg.Scene(sc_ctx).build(3, [blases[b]], inst).closest_tris(q, radius=radius)))
            for what, o in outs:
                assert o[well].tobytes() == bf["closest"][well].tobytes(), f"{what}, radius {label}"
    finally:
        bl.close(); sc_ctx.close()


def deep_queries(pkg, H, m=256):
    """test_gpu_closest_tris.caterpillar_queries' kinds, each aimed at one of the five instances: small triangles below the face at z = 0 (every box passes an
    unbounded query: the first descent pushes at every chain node), between the two near faces, coplanar with the face, through both near faces, and
    among the far triangles"""
    rng = np.random.default_rng(H)
    offs = np.array(DEEP_OFFSETS, dtype=np.float64)
    aimed = np.arange(m) % len(offs)
    c = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-3, -0.5, m)], axis=1)
    c[: m // 6, 2] = 0.25
    c[3 * m // 4:, 2] = rng.uniform(1000, 1000 + 2 * H, m - 3 * m // 4)
    q = c[:, None, :] + rng.normal(0, 0.05, (m, 3, 3))
    q[m // 6: m // 3, :, 2] = 0.0
    q[m // 3: m // 2, 0, 2] = 0.75; q[m // 3: m // 2, 1:, 2] = -0.5
    return no_negzero(as_triangles(pkg, (q + offs[aimed][:, None, :]).astype(F32))), aimed, offs


def tree_depth(nodes, root, ni):
    """the number of internal nodes on the longest path from the root: no walk holds more stack entries than that"""
    deepest, todo = 0, [(int(root), 1)]
    while todo:
        v, d = todo.pop()
        deepest = max(deepest, d)
        todo += [(c, d + 1) for c in (int(nodes["left"][v]), int(nodes["right"][v])) if c < ni]
    return deepest


@pytest.mark.parametrize("H,deep", [(250, True), (20, False)])
def test_deep_blas_takes_the_stackless_pass(pkg, H, deep):
    """the caterpillar under five translated instances.  An unbounded query below the faces passes every box until its first candidate, so its first descent in
    the instance it enters first pushes one entry per chain node: with H = 250 more than the short stack holds (the deep kernel must finish those queries,
    beside quiet ones in the same wave), with H = 20 never (the control on the same code path)"""
    tris, nodes, root, n = caterpillar(pkg, H, 3 + H)
    q, aimed, offs = deep_queries(pkg, H)
    m = len(q)
    cen = xyz(q).astype(np.float64).mean(axis=1)
    pushes = [min(first_descent_pushes(nodes, root, n - 1, cen[j] - t) for t in offs) for j in range(m // 2, 3 * m // 4)]
    assert (max(pushes) > QUERY_STACK) if deep else (tree_depth(nodes, root, n - 1) + len(offs) <= QUERY_STACK), (max(pushes), n)
    inst = make_instances(pkg, [mat34(np.eye(3), t) for t in offs], [0] * len(offs))
    pairs = scene_pair_matrix(pkg, q, [tris], inst)
    c, sc_ctx = pkg.Context(0), pkg.Context(0)
    try:
        d_tris, d_nodes = c.upload(tris), c.upload(nodes)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
        dm = DeviceMesh(pkg, sc_ctx, q, 1)
        for radius in (np.inf, 5.0):
            bf = scene_tris_dist_brute_force(pkg, q, [tris], inst, radius, pairs=pairs)
            assert bf["well"].all() and bf["hit"].any() and (bf["closest"]["feature"] == CROSSING).any()
            sc_ctx.set_profiling(2)
            closest = raw(pkg, scene, dm.inp, m, SCENE_TRIS_QUERY, 0, radius, pkg.QUERY_CLOSEST)
            anyhit = raw(pkg, scene, dm.inp, m, SCENE_TRIS_QUERY, 0, radius, pkg.QUERY_ANY)
            kt = sc_ctx.kernel_times()
            sc_ctx.set_profiling(0)
            assert {"k_scene_closest_tris", "k_scene_closest_tris_deep"} <= set(kt), sorted(kt)
            assert closest.tobytes() == bf["closest"].tobytes(), f"caterpillar {H} radius {radius}"
            assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"]).all() and scene_tris_dist_recompute(pkg, q, [tris], inst, radius, anyhit).all()
        rows = as_triangles(pkg, instance_queries([tris], inst, 2, n))     # (parallel copies 100 apart: every row's answer is the same primitive of a neighbour)
        ibf = scene_tris_dist_brute_force(pkg, rows, [tris], inst, np.inf, skip=2)
        igot = raw(pkg, scene, None, n, SCENE_TRIS_INSTANCE, 2, np.inf, pkg.QUERY_CLOSEST)
        assert ibf["well"].all() and igot.tobytes() == ibf["closest"].tobytes()
        dm.free(); scene.close(); d_nodes.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()


@pytest.mark.parametrize("tlas_algo,deep", [(2, True), (3, True), (0, False)])
def test_deep_top_level_takes_the_stackless_pass(pkg, tlas_algo, deep):
    """180 instances on the staircase: the PLOC-family top-level trees chain the steps up, and a triangle whose box covers them all has a zero lower bound
    at every node, so it enters the left child and pushes the right one at every chain node — more than the short stack holds.  The LBVH top level over
    the same instances is the control: a balanced tree, the same code path, the same answers"""
    mesh, inst, q, _ = tris_deep_top_inputs(pkg)
    tq = as_triangles(pkg, q)
    pairs = cached(("closest tris deep top",), lambda: scene_pair_matrix(pkg, tq, [mesh], inst))
    bf = scene_tris_dist_brute_force(pkg, tq, [mesh], inst, np.inf, pairs=pairs)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        scene = pkg.Scene(sc_ctx).build(tlas_algo, [b], inst)
        t = scene.tlas()
        assert t.n_leaves == 180
        nodes = np.empty(2 * t.n_leaves - 1 if t.layout == 0 else t.n_leaves - 1, dtype=pkg.BVH2_NODE)
        leaves = np.empty(t.n_leaves, dtype=pkg.PRIMREF) if t.layout == 1 else None
        assert pkg.lib().bvh_download(sc_ctx.handle, C.byref(t), nodes.ctypes.data, leaves.ctypes.data if leaves is not None else None, None, None, None) == 0
        top = combined(pkg, nodes, leaves) if leaves is not None else nodes
        need = left_first_scene_need(top, int(t.root), 180, np.ones(len(top), dtype=bool), True)     # the covering triangle: every box passes, left first
        print(f"tlas algo {tlas_algo}: a covering triangle needs {need} entries at the top level")
        assert (need > QUERY_STACK) == deep, need
        sc_ctx.set_profiling(2)
        closest = scene.closest_tris(tq)
        kt = sc_ctx.kernel_times()
        sc_ctx.set_profiling(0)
        assert {"k_scene_closest_tris", "k_scene_closest_tris_deep"} <= set(kt), sorted(kt)
        check_exact(pkg, tq, [mesh], inst, np.inf, bf, closest, scene.closest_tris(tq, query="any"), f"deep top level, algo {tlas_algo}")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_update_after_moves_and_blas_refit(pkg):
    rng = np.random.default_rng(21)
    meshes = [no_negzero(pkg.meshgen.uniform(n, 5 + n)) for n in (150, 120)]
    inst = scene_instances(pkg, rng, 64, 2, 1.5)
    rng2 = np.random.default_rng(22)
    moved = with_shear(pkg, rng2, scene_instances(pkg, rng2, 64, 2, 1.0), 61)      # (the matrices change kind too: s2 is refreshed by the update)
    moved["blas"][:8] = 1 - np.minimum(moved["blas"][:8], 1)
    flat, _, _ = flat_world_tris(pkg, meshes, moved)
    q = make_queries(pkg, flat, 23)[::3]
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        before = scene.closest_tris(q)
        scene.update(moved)
        dm = DeviceMesh(pkg, sc_ctx, q)
        radii = {"inf": np.inf, "band": BAND}
        got = check_all_radii(pkg, scene, q, meshes, moved, scene_pair_matrix(pkg, q, meshes, moved), root_boxes(pkg, blases), "after update", qin=dm.inp,
                              radii=radii, inactive=inactive_of(64))
        assert before.tobytes() != got["inf"][1].tobytes()
        assert pkg.Scene(sc_ctx).build(3, blases, moved).closest_tris(q).tobytes() == got["inf"][1].tobytes(), "an updated and a freshly built scene differ"
        # an update from DEVICE memory that hands instance 4 the other BLAS: instance mode reads the BLAS index on the device, so its rows follow
        swapped = moved.copy(); swapped["blas"][4] = 1 - swapped["blas"][4]
        d_inst = sc_ctx.upload(swapped)
        scene.update((d_inst, len(swapped)))
        n_rows = max(len(t) for t in meshes)
        for what, arr in (("instance 4 with the other BLAS", swapped), ("instance 4 back", moved)):
            rows = as_triangles(pkg, instance_queries(meshes, arr, 4, n_rows))
            igot = check_all_radii(pkg, scene, rows, meshes, arr, scene_pair_matrix(pkg, rows, meshes, arr), root_boxes(pkg, blases), what,
                                   mode=SCENE_TRIS_INSTANCE, k=4, radii=radii, inactive=inactive_of(64))
            assert igot["inf"][0]["hit"].sum() == len(meshes[int(arr["blas"][4])])
            d_inst.upload(moved)
            scene.update((d_inst, len(moved)))
        d_inst.free()
        m0 = jitter(meshes[0], 3, 2e-2)
        blases[0].refit(m0)
        bl.ctxs[0].synchronize()                                          # (the refit ran on the BLAS's own stream: complete before the scene reads the root box)
        scene.update(moved)
        meshes2 = [m0, meshes[1]]
        check_all_radii(pkg, scene, q, meshes2, moved, scene_pair_matrix(pkg, q, meshes2, moved), root_boxes(pkg, blases), "after BLAS refit", qin=dm.inp,
                        radii=radii, inactive=inactive_of(64))
        dm.free(); scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("tlas_algo", [0, 1, 2, 3])
def test_coincident_instances_tie_to_the_lower_index(pkg, tlas_algo):
    """two instances place the same triangles identically, so every answer ties on dist2; one BLAS also holds a far-off extra triangle that stretches its world
    box, so the two are not walked alike.  The lower instance index must win whichever of them that is"""
    mesh = no_negzero(pkg.meshgen.uniform(120, 12))
    v = np.concatenate([mesh["v1"], mesh["v2"], mesh["v3"]])
    lo, hi = v.min(axis=0), v.max(axis=0)
    extra = np.zeros(1, dtype=pkg.meshgen.TRIANGLE)                       # (appended: the prim indices of the shared triangles are the same in both BLASes)
    extra["v1"] = (hi[0] + 50, lo[1], lo[2] - 5); extra["v2"] = (hi[0] + 51, lo[1], lo[2] - 5); extra["v3"] = (hi[0] + 50, lo[1] + 1, lo[2] - 5)
    stretched = no_negzero(np.concatenate([mesh, extra]))
    q = make_queries(pkg, mesh, 40 + tlas_algo)[:-NAN_QUERIES:2]
    inst = make_instances(pkg, [identity(), identity()], [0, 1])
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        plain, far = bl.add(3, mesh), bl.add(1, stretched)
        for order in ((plain, far), (far, plain)):
            blas_tris = [mesh, stretched] if order[0] is plain else [stretched, mesh]
            got = pkg.Scene(sc_ctx).build(tlas_algo, list(order), inst).closest_tris(q)
            bf = cached(("closest tris coincident", tlas_algo, order[0] is plain),
                        lambda: scene_tris_dist_brute_force(pkg, q, blas_tris, inst, np.inf, root_boxes=root_boxes(pkg, list(order))))
            assert (got["prim"] != pkg.INVALID).all()
            assert (got["instance"] == 0).all(), f"stretched BLAS at index {1 if order[0] is plain else 0}: {np.count_nonzero(got['instance'])} ties went to instance 1"
            assert bf["well"].mean() >= 0.99
            assert got[bf["well"]].tobytes() == bf["closest"][bf["well"]].tobytes()
    finally:
        bl.close(); sc_ctx.close()


# ---- argument handling, memory hygiene and the binding ----------------------------------------------------------------------------------------------------------

def small_scene(pkg):
    def make():
        mesh = no_negzero(pkg.meshgen.uniform(100, 3))
        inst = make_instances(pkg, [identity(), mat34(rot(1, 0.7), (0.6, 0.05, -0.1))], [0, 0])
        flat, _, _ = flat_world_tris(pkg, [mesh], inst)
        q = make_queries(pkg, flat, 4)[::3]
        return mesh, inst, q, scene_pair_matrix(pkg, q, [mesh], inst)
    return cached(("closest tris small",), make)


def test_errors_write_nothing_and_guards_stay(pkg):
    mesh, inst, q, pairs = small_scene(pkg)
    m = len(q)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    L = pkg.lib()
    try:
        b = bl.add(3, mesh)
        dm = {fmt: DeviceMesh(pkg, sc_ctx, q, fmt) for fmt in (0, 1, 2)}
        pad = 32
        pattern = np.full((m + 2 * pad) * 16, 0xAB, dtype=np.uint8)
        hits = sc_ctx.upload(pattern)
        h = hits.ptr + pad * 16
        unbuilt, scene = pkg.Scene(sc_ctx), pkg.Scene(sc_ctx).build(2, [b], inst)
        d_inst_before = inst.copy()
        NONE = object()

        def go(sc=scene, qin=dm[0].inp, n=m, mode=SCENE_TRIS_QUERY, k=0, radius=np.inf, out=h, kind=0):
            return L.bvh_scene_closest_tris(sc.handle if sc is not None else None, C.byref(qin) if qin is not NONE else None, n, mode, k, radius, out, kind)

        def inp(fmt, tris=None, verts=None, idx=None, nv=0):
            return pkg.BuildInput(fmt, 30, tris, verts, idx, nv, 0)
        tris_ptr, (v_ptr, i_ptr), nv = dm[0].bufs[0].ptr, (dm[2].bufs[0].ptr, dm[2].bufs[1].ptr), dm[2].inp.n_vertices
        cases = {
            "null scene": go(sc=None), "unbuilt scene": go(sc=unbuilt), "null hits": go(out=None),
            "mode 2": go(mode=2), "mode -1": go(mode=-1), "kind 2": go(kind=2), "kind -1": go(kind=-1),
            "query mode without queries": go(qin=NONE), "instance mode with queries": go(mode=SCENE_TRIS_INSTANCE),
            "query_instance = n_instances": go(qin=NONE, mode=SCENE_TRIS_INSTANCE, k=len(inst)), "query_instance huge": go(qin=NONE, mode=SCENE_TRIS_INSTANCE, k=0xFFFFFFFF),
            "query mode with query_instance 1": go(k=1),
            "unknown format": go(qin=inp(7, tris_ptr)), "padded without triangles": go(qin=inp(0)), "packed misaligned": go(qin=inp(1, dm[1].bufs[0].ptr + 4)),
            "indexed without vertices": go(qin=inp(2, None, None, i_ptr, nv)), "indexed without indices": go(qin=inp(2, None, v_ptr, None, nv)),
            "indexed with no vertices": go(qin=inp(2, None, v_ptr, i_ptr, 0)),
            "n_queries 2^30": go(n=1 << 30),
            "hits in the triangles": go(out=tris_ptr + 64 * (m - 1)), "triangles in the hits": go(qin=inp(0, h + 16 * (m - 1))),
            "hits in the packed triangles": go(qin=dm[1].inp, out=dm[1].bufs[0].ptr + 8), "hits in the vertices": go(qin=dm[2].inp, out=v_ptr + 8),
            "hits in the indices": go(qin=dm[2].inp, out=i_ptr + 12 * (m - 1)),
            "unbuilt, n_queries 0": go(sc=unbuilt, n=0),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        assert go(n=0) == 0 and go(qin=NONE, mode=SCENE_TRIS_INSTANCE, n=0) == 0           # n_queries == 0: nothing is touched
        sc_ctx.synchronize()
        assert np.array_equal(hits.download(np.uint8, pattern.size), pattern), "an error or n_queries == 0 wrote to the hits"
        # the scene still answers, in every query format, inside the guards; the queries, the BLAS's arrays and the instances are unchanged
        rb = root_boxes(pkg, [b])
        tree_before = b.download()
        for radius in (np.inf, BAND):
            bf = scene_tris_dist_brute_force(pkg, q, [mesh], inst, radius, pairs=pairs, root_boxes=rb)
            for fmt in (0, 1, 2):
                for kind in (0, 1):
                    hits.upload(pattern)
                    assert go(qin=dm[fmt].inp, radius=radius, kind=kind) == 0
                    sc_ctx.synchronize()
                    got = hits.download(np.uint8, pattern.size)
                    assert np.array_equal(got[: pad * 16], pattern[: pad * 16]) and np.array_equal(got[-pad * 16:], pattern[-pad * 16:]), "a guard byte changed"
                    rec = np.frombuffer(got[pad * 16: -pad * 16].tobytes(), dtype=pkg.INSTANCE_TRI_HIT)
                    assert scene_tris_dist_recompute(pkg, q, [mesh], inst, radius, rec).all()
                    if kind == 0:
                        assert rec[bf["well"]].tobytes() == bf["closest"][bf["well"]].tobytes()
        assert dm[0].bufs[0].download(pkg.meshgen.TRIANGLE, m).tobytes() == np.ascontiguousarray(q).tobytes()
        tree_after = b.download()
        assert tree_after["nodes"].tobytes() == tree_before["nodes"].tobytes()
        assert inst.tobytes() == d_inst_before.tobytes()
        # instance mode inside the guards: rows beyond the BLAS miss with the exact miss record
        hits.upload(pattern)
        rows = m                                                            # (more rows than the BLAS has leaves)
        assert go(qin=NONE, mode=SCENE_TRIS_INSTANCE, k=1, n=rows, radius=0.25) == 0
        sc_ctx.synchronize()
        got = hits.download(np.uint8, pattern.size)
        assert np.array_equal(got[: pad * 16], pattern[: pad * 16]) and np.array_equal(got[-pad * 16:], pattern[-pad * 16:])
        rec = np.frombuffer(got[pad * 16: -pad * 16].tobytes(), dtype=pkg.INSTANCE_TRI_HIT)
        assert rec[len(mesh):].tobytes() == scene_tri_miss_records(pkg, rows - len(mesh), 0.25).tobytes() and set(rec["instance"][: len(mesh)].tolist()) <= {0, pkg.INVALID}
        scene.close(); unbuilt.close(); hits.free()
        for d in dm.values():
            d.free()
    finally:
        bl.close(); sc_ctx.close()


def test_one_instance_on_a_fresh_ctx(pkg):
    """a one-instance scene builds no top-level tree, so a fresh ctx has made no arena: the call needs none"""
    mesh, inst, q, _ = small_scene(pkg)
    one = inst[1:].copy()
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(2, mesh)
        scene = pkg.Scene(sc_ctx).build(3, [b], one)
        bf = scene_tris_dist_brute_force(pkg, q, [mesh], one, np.inf, root_boxes=root_boxes(pkg, [b]))
        got = scene.closest_tris(q)
        assert bf["well"].mean() >= 0.99 and got[bf["well"]].tobytes() == bf["closest"][bf["well"]].tobytes()
        assert scene_tris_dist_recompute(pkg, q, [mesh], one, np.inf, got).all()
        alone = scene.closest_tris(instance=0)                             # nobody else to answer: every row misses
        assert len(alone) == len(mesh) and alone.tobytes() == scene_tri_miss_records(pkg, len(mesh), np.inf).tobytes()
        assert scene.distance_to(instance=0) == float("inf")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_binding_takes_every_input_kind_and_distance_to(pkg):
    mesh, inst, q, pairs = small_scene(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        want = scene.closest_tris(q)
        assert want.dtype == pkg.INSTANCE_TRI_HIT and want.shape == (len(q),)
        bf = scene_tris_dist_brute_force(pkg, q, [mesh], inst, np.inf, pairs=pairs, root_boxes=root_boxes(pkg, [b]))
        assert want[bf["well"]].tobytes() == bf["closest"][bf["well"]].tobytes()
        x = xyz(q)
        dm = {fmt: DeviceMesh(pkg, sc_ctx, q, fmt) for fmt in (0, 1, 2)}
        for got in (scene.closest_tris(x), scene.closest_tris(x.reshape(-1, 9)), scene.closest_tris(x.astype(np.float64)),
                    scene.closest_tris(dm[0].bufs[0]), scene.closest_tris(dm[0].bufs[0].ptr, n=len(q)),
                    scene.closest_tris(dm[1].bufs[0], tri_format=pkg.TRI_PACKED36),
                    scene.closest_tris(vertices=dm[2].bufs[0], indices=dm[2].bufs[1], n_vertices=dm[2].inp.n_vertices, tri_format=pkg.TRI_INDEXED),
                    scene.closest_tris(q, query=pkg.QUERY_CLOSEST), scene.closest_tris(q, radius=float("inf"))):
            assert got.tobytes() == want.tobytes()
        band = scene.closest_tris(q, radius=BAND)
        assert scene_tris_dist_recompute(pkg, q, [mesh], inst, BAND, band).all() and 0 < (band["prim"] != pkg.INVALID).sum() < len(q)
        anyhit = scene.closest_tris(dm[0].bufs[0], radius=BAND, query="any")
        assert np.array_equal(anyhit["prim"] != pkg.INVALID, band["prim"] != pkg.INVALID) and scene_tris_dist_recompute(pkg, q, [mesh], inst, BAND, anyhit).all()
        rows = as_triangles(pkg, instance_queries([mesh], inst, 1, len(mesh)))
        ibf = scene_tris_dist_brute_force(pkg, rows, [mesh], inst, np.inf, skip=1, root_boxes=root_boxes(pkg, [b]))
        igot = scene.closest_tris(instance=1)
        assert igot[ibf["well"]].tobytes() == ibf["closest"][ibf["well"]].tobytes() and (igot["instance"] == 0).all()
        assert scene.closest_tris(instance=1, n=40).tobytes() == igot[:40].tobytes()
        # distance_to: sqrt of the smallest dist2
        hit = want["prim"] != pkg.INVALID
        assert scene.distance_to(q) == float(np.sqrt(np.float64(want["dist2"][hit].min())))
        assert scene.distance_to(instance=1) == float(np.sqrt(np.float64(igot["dist2"].min())))
        lifted = x + np.array([0.0, 0.0, 50.0], dtype=F32)
        d, lw = scene.distance_to(lifted), scene.closest_tris(lifted)
        assert 40.0 < d < 51.0 and d == float(np.sqrt(np.float64(lw["dist2"][lw["prim"] != pkg.INVALID].min())))
        assert scene.distance_to(q[-2:]) == float("inf")                  # (the last queries carry a NaN: nothing answers)
        for dmesh in dm.values():
            dmesh.free()
        for bad in (lambda: scene.closest_tris(np.zeros((4, 5), dtype=F32)), lambda: scene.closest_tris(4096), lambda: scene.closest_tris(),
                    lambda: scene.closest_tris(q, instance=0), lambda: scene.closest_tris(instance=2), lambda: scene.distance_to()):
            with pytest.raises(pkg.BvhError):
                bad()
        empty = scene.closest_tris(q[:0])
        assert len(empty) == 0 and empty.dtype == pkg.INSTANCE_TRI_HIT and scene.distance_to(q[:0]) == float("inf")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()
