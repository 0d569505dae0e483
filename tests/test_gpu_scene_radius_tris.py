"""bvh_scene_radius_tris on the GPU: every triangle of every active instance within the radius of every query triangle, against the two-level numpy brute
force (tests/test_scene_radius_tris.py) byte for byte — the inputs are those of tests/test_gpu_scene_closest_tris.py (their pair matrices are computed once per
session and shared), and the brute force must report NO ill-conditioned accepted pair on any input and radius used here, so whole arrays are compared: sorted
fills, unsorted fills put in order on the host, count-only calls.  1 to 64 instances over BLASes of every builder, layout and format, in both modes; sheared,
far-offset and mirrored instances; one identity instance against bvh_radius_tris; consistency with bvh_scene_closest_tris and bvh_scene_intersect_tris;
independence from the builders; a deep BLAS and a deep top level through the stackless pass, with a short-tree control; bvh_scene_update after moves and after
a BLAS refit; coincident instances; the passes and the capacity decision; rejections, buffer hygiene and the binding."""
import ctypes as C

import numpy as np
import pytest

from test_closest_tris import CROSSING, E_INVALID
from test_deep_trees import QUERY_STACK, combined
from test_gpu_closest_tris import NAN_QUERIES, make_queries
from test_gpu_intersect_tris import DeviceMesh
from test_gpu_query import caterpillar, mesh as named_mesh
from test_gpu_radius_tris import radii as flat_radii, search as flat_search
from test_gpu_refit import jitter, no_negzero
from test_gpu_scene import TLAS_ALGO, Blases, root_boxes, scene_instances
from test_gpu_scene_closest_tris import deep_queries, exact_inputs, instance_inputs, mirrored_set, small_scene, tree_depth
from test_gpu_scene_intersect_tris import INSTANCE_CASES, four_blases
from test_gpu_scene_point import with_shear
from test_intersect_tris import as_triangles, xyz
from test_scene import identity, make_instances, mat34
from test_scene_closest_tris import SCENE_TRIS_INSTANCE, SCENE_TRIS_QUERY, scene_pair_matrix
from test_scene_intersect_tris import instance_queries, left_first_scene_need, tris_deep_top_inputs
from test_scene_knn import cached, inactive_of
from test_scene_point import flat_world_tris, instance_set
from test_scene_radius_tris import SCENE_RADIUS_TRIS_SORTED as SORTED, scene_radius_host_sort, scene_radius_tris_brute_force, scene_radius_tris_recompute

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32
BAND, WIDE = 0.05, 0.25
QUERY_RADII = {"inf": np.inf, "band": BAND, "wide": WIDE, "zero": 0.0, "negative": -1.0, "nan": np.nan}
INSTANCE_RADII = {"inf": np.inf, "band": BAND, "negative": -1.0}
DEEP_TOP_RADII = (0.0, 1.0e-3, np.inf)           # (a covering triangle passes every top-level box at every radius)


def call(pkg, scene, qin, m, mode, k, radius, flags, d_offsets, d_hits, capacity, total=True):
    t = C.c_uint64(0xDEAD)
    rc = pkg.lib().bvh_scene_radius_tris(scene.handle, C.byref(qin) if qin is not None else None, m, mode, k, radius, flags, d_offsets, d_hits, capacity,
                                         C.byref(t) if total else None)
    return rc, t.value


def search(pkg, scene, qin, m, mode, k, radius, flags):
    """a count-only call, then a fill with the exact capacity; returns (offsets, records).  The count-only offsets must equal the fill's."""
    ctx = scene.ctx
    d_off, hits = ctx.alloc((m + 1) * 4), None
    try:
        rc, total = call(pkg, scene, qin, m, mode, k, radius, flags, d_off.ptr, None, 0)
        assert rc == 0, rc
        counted = d_off.download(np.uint32, m + 1)
        assert counted[0] == 0 and counted[-1] == total
        hits = ctx.alloc(max(total, 1) * 16)
        rc, total2 = call(pkg, scene, qin, m, mode, k, radius, flags, d_off.ptr, hits.ptr, total)
        assert rc == 0 and total2 == total
        off = d_off.download(np.uint32, m + 1)
        assert off.tobytes() == counted.tobytes(), "count-only and fill calls disagree on the offsets"
        return off, hits.download(pkg.INSTANCE_TRI_HIT, total)
    finally:
        d_off.free()
        if hits is not None:
            hits.free()


def same(got, bf):
    return got[0].tobytes() == bf["offsets"].tobytes() and got[1].tobytes() == bf["hits"].tobytes()


def check_all_ways(pkg, scene, q, blas_tris, inst, radius, bf, what, qin=None, mode=SCENE_TRIS_QUERY, k=0, sorted_fill=True, recompute=True, inactive=()):
    """the exactness gate (no ill-conditioned accepted pair: a condition on the input, not a measurement), then whole arrays: the sorted fill equals the brute
    force byte for byte; the unsorted fill has equal offsets, equals it once sorted on the host and passes the record checker; search asserts that the
    count-only offsets equal the fill call's.  No inactive (or skipped) instance appears in a record"""
    assert bf["ill_pairs"] == 0 and bf["well"].all(), f"{what}: {bf['ill_pairs']} ill-conditioned accepted pairs: change the input, not the gate"
    m, skip = len(xyz(q)), (k if mode == SCENE_TRIS_INSTANCE else None)
    if sorted_fill:
        assert same(search(pkg, scene, qin, m, mode, k, radius, SORTED), bf), what + ": the sorted fill differs from the brute force"
    uoff, uhits = search(pkg, scene, qin, m, mode, k, radius, 0)
    assert uoff.tobytes() == bf["offsets"].tobytes(), what + ": the unsorted call counts differently"
    assert scene_radius_host_sort(uoff, uhits).tobytes() == bf["hits"].tobytes(), what + ": the unsorted fill is another set"
    if recompute:
        assert scene_radius_tris_recompute(pkg, q, blas_tris, inst, radius, uoff, uhits, skip=skip) is None, what
    answered = set(np.unique(uhits["instance"]).tolist())
    assert not answered & set(inactive), f"{what}: an inactive instance answered"
    assert skip is None or skip not in answered, f"{what}: the query instance answered"


def brute(pkg, key, q, blas_tris, inst, radius, pairs, skip=None, rb=None):
    return cached(("scene radius tris",) + key + (repr(float(radius)), skip),
                  lambda: scene_radius_tris_brute_force(pkg, q, blas_tris, inst, radius, skip=skip, pairs=pairs, root_boxes=rb))


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_inst", [1, 2, 3, 64])
def test_exact_against_brute_force_in_both_modes(pkg, n_inst):
    """1: no top-level tree; 2: a root with two leaf children; 3: the singular instance inactive; 64: all three kinds of inactive instance.  QUERY mode at
    spacing 1.5; INSTANCE mode at spacing 0.6 for 2 and 3 instances.  At 64 instances and radius inf the slices hold up to 5 520 records: the quadratic sorted
    insertion is left to the smaller scenes, and the unsorted fill is put in order on the host"""
    meshes, inst, q, pairs = exact_inputs(pkg, n_inst)
    inactive = inactive_of(n_inst)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = four_blases(pkg, bl, meshes)
        rb = root_boxes(pkg, blases)
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[n_inst], blases, inst)
        dm = DeviceMesh(pkg, sc_ctx, q, n_inst % 3)
        totals = {}
        for label, radius in QUERY_RADII.items():
            bf = brute(pkg, ("exact", n_inst, 1.5), q, meshes, inst, radius, pairs, rb=rb)
            big = n_inst == 64 and label == "inf"
            check_all_ways(pkg, scene, q, meshes, inst, radius, bf, f"{n_inst} instances radius {label}", qin=dm.inp, sorted_fill=not big, recompute=not big,
                           inactive=inactive)
            totals[label] = len(bf["hits"])
            print(f"{n_inst} instances radius {label}: {len(bf['hits'])} records, longest slice {int(bf['counts'].max())}")
        dm.free()
        assert totals["negative"] == 0 and totals["nan"] == 0
        assert 0 < totals["zero"] < totals["band"] < totals["wide"] < totals["inf"]
        n_active_tris = sum(len(meshes[int(inst["blas"][k])]) for k in range(n_inst) if k not in inactive)
        assert totals["inf"] == (len(q) - NAN_QUERIES) * n_active_tris
        zero = brute(pkg, ("exact", n_inst, 1.5), q, meshes, inst, 0.0, pairs, rb=rb)["hits"]
        assert (zero["feature"] == CROSSING).any() and (zero["dist2"] == 0).all()
        boff, bhits = scene.radius_tris(q, radius=BAND)                                        # the Python binding, a host mesh
        assert same((boff, bhits), brute(pkg, ("exact", n_inst, 1.5), q, meshes, inst, BAND, pairs, rb=rb))
        spacing = 0.6 if n_inst in (2, 3) else 1.5
        if n_inst in (2, 3):                                                                    # the interpenetrating scene of the instance mode
            scene.close()
            meshes, inst, _, _ = exact_inputs(pkg, n_inst, 0.6)
            scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[n_inst], blases, inst)
        for k in INSTANCE_CASES[n_inst]:
            _, _, rows, ipairs = instance_inputs(pkg, n_inst, k, spacing)
            n_rows = len(rows)
            itot = {}
            for label, radius in INSTANCE_RADII.items():
                ibf = brute(pkg, ("instance", n_inst, k, spacing), rows, meshes, inst, radius, ipairs, skip=k, rb=rb)
                check_all_ways(pkg, scene, rows, meshes, inst, radius, ibf, f"{n_inst} instances, instance {k}, radius {label}", mode=SCENE_TRIS_INSTANCE, k=k,
                               sorted_fill=not (n_inst == 64 and label == "inf"), inactive=inactive)
                itot[label] = len(ibf["hits"])
            print(f"{n_inst} instances, instance {k}: records {itot}")
            if k in inactive or n_inst == 1:
                assert itot["inf"] == 0                                                         # an inactive query instance, or nobody else to answer
            else:
                assert 0 == itot["negative"] < itot["band"] < itot["inf"]
                n_own = len(meshes[int(inst["blas"][k])])
                ibf = brute(pkg, ("instance", n_inst, k, spacing), rows, meshes, inst, np.inf, ipairs, skip=k, rb=rb)
                assert (ibf["counts"][:n_own] > 0).all() and not ibf["counts"][n_own:].any()     # rows at or beyond the BLAS's n_leaves are empty
            ioff = scene.radius_tris(instance=k, radius=BAND, count_only=True)                  # the binding: as many rows as the largest BLAS has leaves
            assert ioff.tobytes() == brute(pkg, ("instance", n_inst, k, spacing), rows, meshes, inst, BAND, ipairs, skip=k, rb=rb)["offsets"].tobytes()
            if n_inst == 3 and k == 1:                                                           # 65 rows: a partial last wave, fewer rows than the BLAS has leaves
                full = brute(pkg, ("instance", n_inst, k, spacing), rows, meshes, inst, np.inf, ipairs, skip=k, rb=rb)
                cut = search(pkg, scene, None, 65, SCENE_TRIS_INSTANCE, k, np.inf, SORTED)
                assert cut[0].tobytes() == full["offsets"][:66].tobytes() and cut[1].tobytes() == full["hits"][: int(full["offsets"][65])].tobytes()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("kind", ["shear", "far", "mirror"])
def test_sheared_far_offset_and_mirrored_instances(pkg, kind):
    """every instance is rotation x diag(0.25 .. 4) x shear x rotation ("shear"), rigid with translations up to 4096 ("far") or a reflection ("mirror")"""
    def make():
        rng = np.random.default_rng({"shear": 7, "far": 8, "mirror": 9}[kind])
        mesh = no_negzero(pkg.meshgen.uniform(300, 41))
        inst = mirrored_set(pkg, rng, 8) if kind == "mirror" else instance_set(pkg, rng, kind, 8)
        flat, _, _ = flat_world_tris(pkg, [mesh], inst)
        q = make_queries(pkg, flat, 9)
        rows = as_triangles(pkg, instance_queries([mesh], inst, 5, len(mesh)))
        return mesh, inst, q, scene_pair_matrix(pkg, q, [mesh], inst), rows, scene_pair_matrix(pkg, rows, [mesh], inst)
    mesh, inst, q, pairs, rows, ipairs = cached(("scene radius tris kinds", kind), make)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        rb = root_boxes(pkg, [b])
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        dm = DeviceMesh(pkg, sc_ctx, q, 2)
        for label, radius in (("inf", np.inf), ("band", BAND)):
            bf = brute(pkg, ("kinds", kind), q, [mesh], inst, radius, pairs, rb=rb)
            check_all_ways(pkg, scene, q, [mesh], inst, radius, bf, f"{kind} radius {label}", qin=dm.inp, recompute=label != "inf")
            if label == "inf":
                assert len(bf["hits"]) == (len(q) - NAN_QUERIES) * 8 * len(mesh)
            else:
                assert 0 < len(bf["hits"]) and len(set(bf["hits"]["instance"].tolist())) >= 4
        ibf = brute(pkg, ("kinds instance", kind), rows, [mesh], inst, np.inf, ipairs, skip=5, rb=rb)
        assert len(ibf["hits"]) == 7 * len(mesh) * len(mesh)
        check_all_ways(pkg, scene, rows, [mesh], inst, np.inf, ibf, kind + ", instance 5", mode=SCENE_TRIS_INSTANCE, k=5, recompute=False)
        dm.free(); scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- relations --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [1, 3])
def test_one_identity_instance_equals_radius_tris(pkg, algo):
    """((1 x + 0 y) + 0 z) + 0 == x as a value and W = identity maps the query onto itself: offsets and records byte for byte (the flat record's reserved 0 is
    instance 0)"""
    tris = named_mesh(pkg, "uniform_1000")
    q = make_queries(pkg, tris, 1017)
    r = flat_radii(tris)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(algo, tris)
        assert b.result.layout == (0 if algo == 1 else 1)
        scene = pkg.Scene(sc_ctx).build(3, [b], make_instances(pkg, [identity()], [0]))
        d_q = bl.ctxs[0].upload(q)
        qin = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_q.ptr, None, None, 0, 0)
        for label in ("inf", "band", "zero"):
            foff, fhits = flat_search(pkg, bl.ctxs[0], b.result, qin, len(q), r[label], pkg.RADIUS_TRIS_SORTED)
            off, hits = scene.radius_tris(q, radius=r[label])
            assert len(fhits) > 0 and off.tobytes() == foff.tobytes() and hits.tobytes() == fhits.tobytes(), f"radius {label}"
            assert (hits["instance"] == 0).all()
        d_q.free(); scene.close()
    finally:
        bl.close(); sc_ctx.close()


def feature_15_slices(pkg, off, hits):
    """the feature-15 records of every slice in (instance, prim) order, as bvh_scene_intersect_tris's (offsets, INSTANCE_PRIM records)"""
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    keep = hits["feature"] == CROSSING
    rows, h = rows[keep], hits[keep]
    order = np.lexsort((h["prim"], h["instance"], rows))
    recs = np.zeros(len(h), dtype=pkg.INSTANCE_PRIM)
    recs["prim"], recs["instance"] = h["prim"][order], h["instance"][order]
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=len(off) - 1))]).astype(np.uint32), recs


def test_consistent_with_scene_closest_tris_and_scene_intersect_tris(pkg):
    """on the interpenetrating three-instance scene, in both modes: the first sorted record of every non-empty slice is bvh_scene_closest_tris's closest record
    at the same radius and the empty slices are its misses; the feature-15 records at radius 0 are bvh_scene_intersect_tris's set"""
    meshes, inst, q, _ = exact_inputs(pkg, 3, 0.6)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[3], four_blases(pkg, bl, meshes), inst)
        for what, side in (("query mode", {"other": q}), ("instance 1", {"instance": 1})):
            for radius in (np.inf, BAND, 0.0):
                off, hits = scene.radius_tris(radius=radius, **side)
                closest = scene.closest_tris(radius=radius, query="closest", **side)
                nonempty = np.diff(off.astype(np.int64)) > 0
                assert nonempty.any() and (~nonempty).any(), f"{what} radius {radius}"
                assert np.array_equal(nonempty, closest["prim"] != pkg.INVALID), f"{what} radius {radius}: an empty slice is not a miss"
                assert hits[off[:-1][nonempty]].tobytes() == closest[nonempty].tobytes(), f"{what} radius {radius}: the first record is not the closest"
            xoff, xrecs = scene.intersect_tris(**side)
            foff, frecs = feature_15_slices(pkg, off, hits)                # (the last radius is 0)
            assert len(xrecs) > 20 and foff.tobytes() == xoff.tobytes() and frecs.tobytes() == xrecs.tobytes(), f"{what}: the crossings differ"
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- independence, depth and updates ----------------------------------------------------------------------------------------------------------------------------

def builders_inputs(pkg):
    def make():
        rng = np.random.default_rng(9)
        mesh = no_negzero(pkg.meshgen.uniform(200, 77))
        inst = with_shear(pkg, rng, scene_instances(pkg, rng, 64, 1, 1.2), 61)
        flat, _, _ = flat_world_tris(pkg, [mesh], inst)
        q = make_queries(pkg, flat, 5)[::12]
        return mesh, inst, q, scene_pair_matrix(pkg, q, [mesh], inst)
    return cached(("scene radius tris builders",), make)


def test_independent_of_builders(pkg):
    mesh, inst, q, pairs = builders_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(algo, mesh, fmt=algo % 3) for algo in range(4)]
        rb = root_boxes(pkg, blases[:1])
        for label, radius in (("wide", WIDE),):                           # (slices of up to 1 807 records, sorted in each of seven scenes: one radius)
            bf = brute(pkg, ("builders",), q, [mesh], inst, radius, pairs, rb=rb)
            assert bf["ill_pairs"] == 0 and len(bf["hits"]) > 200
            outs = []
            for tl in range(4):                                           # top-level builders over the same BLAS
                outs.append((f"top-level builder {tl}", pkg.Scene(sc_ctx).build(tl, [blases[3]], inst).radius_tris(q, radius=radius)))
            for b in range(3):                                            # BLAS builders (and layouts, and formats) of the same mesh
                outs.append((f"BLAS builder {b}", pkg.Scene(sc_ctx).build(3, [blases[b]], inst).radius_tris(q, radius=radius)))
            for what, o in outs:
                assert same(o, bf), f"{what}, radius {label}"
    finally:
        bl.close(); sc_ctx.close()


def deep_inputs(pkg, H):
    def make():
        tris, nodes, root, n = caterpillar(pkg, H, 3 + H)
        q, aimed, offs = deep_queries(pkg, H)
        inst = make_instances(pkg, [mat34(np.eye(3), t) for t in offs], [0] * len(offs))
        return tris, nodes, root, n, q, inst, scene_pair_matrix(pkg, q, [tris], inst)
    return cached(("scene radius tris deep", H), make)


@pytest.mark.parametrize("H,deep", [(250, True), (20, False)])
def test_deep_blas_takes_the_stackless_pass(pkg, H, deep):
    """the caterpillar under five translated instances.  At radius inf every box passes, so the left-first walk holds one pushed entry per chain node whose
    chain child is its left one: with H = 250 more than the short stack holds — every live query overflows in the count pass AND in the fill pass, and the
    stackless kernel must find the whole set twice, or the offsets and the bytes differ — with H = 20 never (the control on the same code path)"""
    tris, nodes, root, n, q, inst, pairs = deep_inputs(pkg, H)
    m = len(q)
    need = left_first_scene_need(nodes, root, n, np.ones(len(nodes), dtype=bool), False)
    assert (need > QUERY_STACK) if deep else (tree_depth(nodes, root, n - 1) + len(inst) <= QUERY_STACK), need
    c, sc_ctx = pkg.Context(0), pkg.Context(0)
    try:
        d_tris, d_nodes = c.upload(tris), c.upload(nodes)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
        dm = DeviceMesh(pkg, sc_ctx, q, 1)
        for radius in (np.inf, 5.0):
            bf = brute(pkg, ("deep", H), q, [tris], inst, radius, pairs)
            assert bf["ill_pairs"] == 0 and len(bf["hits"]) > 0 and (bf["hits"]["feature"] == CROSSING).any()
            if radius == np.inf:
                assert (bf["counts"][bf["counts"] > 0] == len(inst) * n).all()      # a live query accepts every triangle of every instance
            sc_ctx.set_profiling(2)
            got = search(pkg, scene, dm.inp, m, SCENE_TRIS_QUERY, 0, radius, SORTED)          # count and fill: each takes the stackless pass
            kt = sc_ctx.kernel_times()
            sc_ctx.set_profiling(0)
            assert {"k_scene_radius_tris_walk", "k_scene_radius_tris_deep", "k_overlap_scan"} <= set(kt), sorted(kt)
            launches = {name: v[1] for name, v in kt.items()}              # (search: a count-only call, then a call that counts and fills)
            assert launches["k_scene_radius_tris_walk"] == 3 and launches["k_scene_radius_tris_deep"] == 3 and launches["k_overlap_scan"] == 2, launches
            if radius == np.inf:
                # every live query leaves the stack walk after at most QUERY_STACK pushes and is redone from its start by the stackless kernel, in all three
                # passes: that kernel tests all the 5 n leaves of every query and takes longer than the walk; in the control it only looks at its word
                print(f"caterpillar {H}: summed ms over three passes " + ", ".join(f"{name} {v[0]:.4f}" for name, v in sorted(kt.items())))
                assert (kt["k_scene_radius_tris_deep"][0] > kt["k_scene_radius_tris_walk"][0]) == deep, kt
            assert same(got, bf), f"caterpillar {H} radius {radius}"
            u = search(pkg, scene, dm.inp, m, SCENE_TRIS_QUERY, 0, radius, 0)
            assert u[0].tobytes() == bf["offsets"].tobytes() and scene_radius_host_sort(*u).tobytes() == bf["hits"].tobytes()
        rows = as_triangles(pkg, instance_queries([tris], inst, 2, n))     # (parallel copies 100 apart)
        ibf = cached(("scene radius tris deep rows", H), lambda: scene_radius_tris_brute_force(pkg, rows, [tris], inst, 150.0, skip=2))
        assert ibf["ill_pairs"] == 0 and len(ibf["hits"]) > 0
        assert same(search(pkg, scene, None, n, SCENE_TRIS_INSTANCE, 2, 150.0, SORTED), ibf)
        dm.free(); scene.close(); d_nodes.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()


@pytest.mark.parametrize("tlas_algo,deep", [(2, True), (3, True), (0, False)])
def test_deep_top_level_takes_the_stackless_pass(pkg, tlas_algo, deep):
    """180 instances on the staircase: the PLOC-family top-level trees chain the steps up, and a triangle whose box covers them all has a zero lower bound at
    every node at every radius, so it enters the left child and pushes the right one at every chain node — more than the short stack holds, in the count pass
    and in the fill pass.  The LBVH top level over the same instances is the control: a balanced tree, the same code path, the same answers"""
    mesh, inst, q, _ = tris_deep_top_inputs(pkg)
    tq = as_triangles(pkg, q)
    pairs = cached(("closest tris deep top",), lambda: scene_pair_matrix(pkg, tq, [mesh], inst))
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
        assert (need > QUERY_STACK) == deep, need
        dm = DeviceMesh(pkg, sc_ctx, tq, 0)
        for radius in DEEP_TOP_RADII:
            bf = brute(pkg, ("deep top",), tq, [mesh], inst, radius, pairs)
            assert bf["ill_pairs"] == 0 and (bf["counts"][::32] > 0).all(), "a covering triangle accepts nothing: the deep queries have no records to lose"
            sc_ctx.set_profiling(2)
            got = search(pkg, scene, dm.inp, len(tq), SCENE_TRIS_QUERY, 0, radius, SORTED)
            kt = sc_ctx.kernel_times()
            sc_ctx.set_profiling(0)
            assert {"k_scene_radius_tris_walk", "k_scene_radius_tris_deep", "k_overlap_scan"} <= set(kt), sorted(kt)
            assert same(got, bf), f"deep top level, algo {tlas_algo}, radius {radius}"
            u = search(pkg, scene, dm.inp, len(tq), SCENE_TRIS_QUERY, 0, radius, 0)
            assert u[0].tobytes() == bf["offsets"].tobytes() and scene_radius_host_sort(*u).tobytes() == bf["hits"].tobytes()
        dm.free(); scene.close()
    finally:
        bl.close(); sc_ctx.close()



def update_inputs(pkg):
    def make():
        rng = np.random.default_rng(21)
        meshes = [no_negzero(pkg.meshgen.uniform(n, 5 + n)) for n in (150, 120)]
        inst = scene_instances(pkg, rng, 64, 2, 1.5)
        rng2 = np.random.default_rng(22)
        moved = with_shear(pkg, rng2, scene_instances(pkg, rng2, 64, 2, 1.0), 61)      # (the matrices change kind too: s2 is refreshed by the update)
        moved["blas"][:8] = 1 - np.minimum(moved["blas"][:8], 1)
        flat, _, _ = flat_world_tris(pkg, meshes, moved)
        q = make_queries(pkg, flat, 23)[::16]
        swapped = moved.copy(); swapped["blas"][4] = 1 - swapped["blas"][4]
        n_rows = 33                                                       # (a partial last wave; fewer rows than either BLAS has leaves)
        rows = {name: as_triangles(pkg, instance_queries(meshes, arr, 4, n_rows)) for name, arr in (("swapped", swapped), ("moved", moved))}
        m0 = jitter(meshes[0], 3, 2e-2)
        return {"meshes": meshes, "inst": inst, "moved": moved, "swapped": swapped, "q": q, "rows": rows, "m0": m0,
                "pairs": scene_pair_matrix(pkg, q, meshes, moved), "pairs_refit": scene_pair_matrix(pkg, q, [m0, meshes[1]], moved),
                "ipairs": {"swapped": scene_pair_matrix(pkg, rows["swapped"], meshes, swapped), "moved": scene_pair_matrix(pkg, rows["moved"], meshes, moved)}}
    return cached(("scene radius tris update",), make)


def test_update_after_moves_and_blas_refit(pkg):
    d = update_inputs(pkg)
    meshes, inst, moved, q = d["meshes"], d["inst"], d["moved"], d["q"]
    radii = {"band": BAND, "wide": WIDE}
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        before = scene.radius_tris(q, radius=WIDE)
        scene.update(moved)
        dm = DeviceMesh(pkg, sc_ctx, q)
        rb = root_boxes(pkg, blases)
        for label, radius in radii.items():
            bf = brute(pkg, ("update",), q, meshes, moved, radius, d["pairs"], rb=rb)
            assert len(bf["hits"]) > 100
            check_all_ways(pkg, scene, q, meshes, moved, radius, bf, f"after update, radius {label}", qin=dm.inp, inactive=inactive_of(64))
        after = brute(pkg, ("update",), q, meshes, moved, WIDE, d["pairs"], rb=rb)
        assert not same(before, after)
        assert same(pkg.Scene(sc_ctx).build(3, blases, moved).radius_tris(q, radius=WIDE), after), "an updated and a freshly built scene differ"
        # an update from DEVICE memory that hands instance 4 the other BLAS: instance mode reads the BLAS index on the device, so its rows follow
        d_inst = sc_ctx.upload(d["swapped"])
        scene.update((d_inst, len(moved)))
        for name in ("swapped", "moved"):
            arr, rows = d[name], d["rows"][name]
            ibf = brute(pkg, ("update rows", name), rows, meshes, arr, WIDE, d["ipairs"][name], skip=4, rb=rb)
            assert len(ibf["hits"]) > 50
            check_all_ways(pkg, scene, rows, meshes, arr, WIDE, ibf, f"instance 4, {name}", mode=SCENE_TRIS_INSTANCE, k=4, inactive=inactive_of(64))
            d_inst.upload(moved)
            scene.update((d_inst, len(moved)))
        d_inst.free()
        blases[0].refit(d["m0"])
        bl.ctxs[0].synchronize()                                          # (the refit ran on the BLAS's own stream: complete before the scene reads the root box)
        scene.update(moved)
        meshes2 = [d["m0"], meshes[1]]
        rb = root_boxes(pkg, blases)
        for label, radius in radii.items():
            bf = brute(pkg, ("update refit",), q, meshes2, moved, radius, d["pairs_refit"], rb=rb)
            check_all_ways(pkg, scene, q, meshes2, moved, radius, bf, f"after BLAS refit, radius {label}", qin=dm.inp, inactive=inactive_of(64))
        dm.free(); scene.close()
    finally:
        bl.close(); sc_ctx.close()


def coincident_inputs(pkg):
    def make():
        mesh = no_negzero(pkg.meshgen.uniform(120, 12))
        v = np.concatenate([mesh["v1"], mesh["v2"], mesh["v3"]])
        lo, hi = v.min(axis=0), v.max(axis=0)
        extra = np.zeros(1, dtype=pkg.meshgen.TRIANGLE)                   # (appended: the prim indices of the shared triangles are the same in both BLASes)
        extra["v1"] = (hi[0] + 50, lo[1], lo[2] - 5); extra["v2"] = (hi[0] + 51, lo[1], lo[2] - 5); extra["v3"] = (hi[0] + 50, lo[1] + 1, lo[2] - 5)
        stretched = no_negzero(np.concatenate([mesh, extra]))
        q = make_queries(pkg, mesh, 40)[:-NAN_QUERIES:2]
        inst = make_instances(pkg, [identity(), identity()], [0, 1])
        return mesh, stretched, q, inst
    return cached(("scene radius tris coincident",), make)


@pytest.mark.parametrize("tlas_algo", [0, 1, 2, 3])
def test_coincident_instances_report_both_in_instance_order(pkg, tlas_algo):
    """two instances place the same triangles identically, so every accepted triangle is reported twice, at bit-equal dist2, instance 0 before instance 1; one
    BLAS also holds a far-off extra triangle that stretches its world box, so the two are not walked alike"""
    mesh, stretched, q, inst = coincident_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        plain, far = bl.add(3, mesh), bl.add(1, stretched)
        for order in ((plain, far), (far, plain)):
            blas_tris = [mesh, stretched] if order[0] is plain else [stretched, mesh]
            bf = cached(("scene radius tris coincident bf", order[0] is plain), lambda: scene_radius_tris_brute_force(pkg, q, blas_tris, inst, WIDE))
            assert bf["ill_pairs"] == 0 and len(bf["hits"]) > 200
            off, hits = pkg.Scene(sc_ctx).build(tlas_algo, list(order), inst).radius_tris(q, radius=WIDE)
            assert same((off, hits), bf)
            # (sorted by (dist2, instance, prim): what instance 0 reports and what instance 1 reports are the same (dist2, prim, feature) sequence in every slice,
            # and within a run of equal dist2 all of instance 0's records come before instance 1's — the bytes above say so; here: nothing is reported once only)
            rows = np.repeat(np.arange(len(q)), np.diff(off.astype(np.int64)))
            a, b = hits["instance"] == 0, hits["instance"] == 1
            assert (a | b).all() and a.sum() == b.sum() and np.array_equal(rows[a], rows[b])
            for f in ("dist2", "prim", "feature"):
                assert hits[f][a].tobytes() == hits[f][b].tobytes(), f
            first = off[:-1][np.diff(off.astype(np.int64)) > 0]
            assert (hits["instance"][first] == 0).all()
    finally:
        bl.close(); sc_ctx.close()


# ---- argument handling, memory hygiene and the binding ----------------------------------------------------------------------------------------------------------

def small_brute(pkg, radius, rb=None):
    mesh, inst, q, pairs = small_scene(pkg)
    return brute(pkg, ("small",), q, [mesh], inst, radius, pairs, rb=rb)


def test_passes_capacity_and_bounds(pkg):
    """the count-only pass, a capacity one record short (the fill is skipped, the offsets complete), the exact capacity (guards intact, the same bytes twice), a
    NULL total_out and n == 0.  NOT tested, as for bvh_scene_radius_search, whose sink, scan and tail this call shares: the saturation marks — the per-query
    counter stopping at 0xFFFFFFFD and a total of 2^32 or more — which need more than four thousand million accepted pairs in one call"""
    mesh, inst, q, _ = small_scene(pkg)
    bl, ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        scene = pkg.Scene(ctx).build(2, [b], inst)
        bf = small_brute(pkg, WIDE, root_boxes(pkg, [b]))
        assert bf["ill_pairs"] == 0
        dm = DeviceMesh(pkg, ctx, q)
        m = dm.n
        want = {flags: search(pkg, scene, dm.inp, m, SCENE_TRIS_QUERY, 0, WIDE, flags) for flags in (SORTED, 0)}
        exp_off = bf["offsets"]
        total = int(exp_off[-1])
        assert total > 50 and same(want[SORTED], bf) and want[0][0].tobytes() == exp_off.tobytes()
        extra = 29
        guard_h = np.frombuffer(np.full((total + extra) * 16, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_TRI_HIT)
        guard_o = np.full(m + 1 + extra, 0xA5A5A5A5, dtype=np.uint32)
        d_off, d_hits = ctx.upload(guard_o), ctx.upload(guard_h)
        go = lambda flags, hits, cap, tot=True: call(pkg, scene, dm.inp, m, SCENE_TRIS_QUERY, 0, WIDE, flags, d_off.ptr, hits, cap, total=tot)
        for flags in (SORTED, 0):
            out = {}
            # count only: d_hits untouched, offsets complete, guard words past n_queries + 1 offsets intact
            d_off.upload(guard_o); d_hits.upload(guard_h)
            assert go(flags, None, 0) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_hits.download(pkg.INSTANCE_TRI_HIT, total + extra).tobytes() == guard_h.tobytes()
            # capacity total - 1: the fill is skipped, d_offsets still complete, *total_out set
            d_off.upload(guard_o)
            assert go(flags, d_hits.ptr, total - 1) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_hits.download(pkg.INSTANCE_TRI_HIT, total + extra).tobytes() == guard_h.tobytes()
            # the exact capacity is filled; guard records past the total intact; twice the same bytes
            for rnd in range(2):
                d_off.upload(guard_o); d_hits.upload(guard_h)
                assert go(flags, d_hits.ptr, total) == (0, total)
                o, p = d_off.download(np.uint32, m + 1 + extra), d_hits.download(pkg.INSTANCE_TRI_HIT, total + extra)
                assert o[m + 1:].tobytes() == guard_o[m + 1:].tobytes() and p[total:].tobytes() == guard_h[total:].tobytes()
                assert o[: m + 1].tobytes() == exp_off.tobytes() and p[:total].tobytes() == want[flags][1].tobytes()
                out[rnd] = (o.tobytes(), p.tobytes())
            assert out[0] == out[1], "two identical calls give different bytes"
            # total_out == NULL: the same device bytes after a synchronize
            d_off.upload(guard_o); d_hits.upload(guard_h)
            rc, t = go(flags, d_hits.ptr, total + extra, tot=False)
            assert rc == 0 and t == 0xDEAD
            ctx.synchronize()
            assert (d_off.download(np.uint32, m + 1 + extra).tobytes(), d_hits.download(pkg.INSTANCE_TRI_HIT, total + extra).tobytes()) == out[0]
        # n_queries == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        d_off.upload(guard_o); d_hits.upload(guard_h)
        assert call(pkg, scene, dm.inp, 0, SCENE_TRIS_QUERY, 0, WIDE, SORTED, d_off.ptr, d_hits.ptr, total) == (0, 0)
        o = d_off.download(np.uint32, m + 1 + extra)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes() and d_hits.download(pkg.INSTANCE_TRI_HIT, total + extra).tobytes() == guard_h.tobytes()
        scene.close(); dm.free(); d_off.free(); d_hits.free()
    finally:
        bl.close(); ctx.close()


def test_errors_write_nothing(pkg):
    mesh, inst, q, _ = small_scene(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    L = pkg.lib()
    try:
        b = bl.add(3, mesh)
        bf = small_brute(pkg, WIDE, root_boxes(pkg, [b]))
        dm = {fmt: DeviceMesh(pkg, sc_ctx, q, fmt) for fmt in (0, 1, 2)}
        m = len(q)
        cap = int(bf["offsets"][-1]) + 64
        guard_h = np.frombuffer(np.full(cap * 16, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_TRI_HIT)
        guard_o = np.full(m + 1, 0x5A5A5A5A, dtype=np.uint32)
        hits, offs = sc_ctx.upload(guard_h), sc_ctx.upload(guard_o)
        tot = C.c_uint64(0x77)
        unbuilt, scene = pkg.Scene(sc_ctx), pkg.Scene(sc_ctx).build(2, [b], inst)
        NONE = object()

        def go(sc=scene, qin=dm[0].inp, n=m, mode=SCENE_TRIS_QUERY, k=0, radius=WIDE, flags=SORTED, o=offs.ptr, h=hits.ptr, c=cap):
            return L.bvh_scene_radius_tris(sc.handle if sc is not None else None, C.byref(qin) if qin is not NONE else None, n, mode, k, radius, flags, o, h, c,
                                           C.byref(tot))

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
            "offsets in the triangles": go(o=tris_ptr + 64), "hits in the triangles": go(h=tris_ptr + 64 * (m - 1)),
            "hits in the packed triangles": go(qin=dm[1].inp, h=dm[1].bufs[0].ptr + 8), "hits in the vertices": go(qin=dm[2].inp, h=v_ptr + 8),
            "offsets in the indices": go(qin=dm[2].inp, o=i_ptr + 12 * (m - 1)),
            "hits in offsets": go(h=offs.ptr + 16), "offsets in hits": go(o=hits.ptr + 16 * (cap - 1)),
            "hits over the triangles, capacity clamped": go(h=tris_ptr - 16, c=1 << 40),
            "unbuilt, n_queries 0": go(sc=unbuilt, n=0),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        assert tot.value == 0x77
        sc_ctx.synchronize()
        assert hits.download(pkg.INSTANCE_TRI_HIT, cap).tobytes() == guard_h.tobytes() and offs.download(np.uint32, m + 1).tobytes() == guard_o.tobytes()
        assert dm[0].bufs[0].download(pkg.meshgen.TRIANGLE, m).tobytes() == np.ascontiguousarray(q).tobytes()
        # a count-only call ignores the capacity's range, and the scene still answers — in every query format
        total = int(bf["offsets"][-1])
        assert go(h=None, c=1 << 40) == 0 and tot.value == total
        assert offs.download(np.uint32, m + 1)[-1] == total and hits.download(pkg.INSTANCE_TRI_HIT, cap).tobytes() == guard_h.tobytes()
        for fmt in (0, 1, 2):
            hits.upload(guard_h)
            assert go(qin=dm[fmt].inp) == 0 and tot.value == total
            got = hits.download(pkg.INSTANCE_TRI_HIT, cap)
            assert got[total:].tobytes() == guard_h[total:].tobytes()
            assert same((offs.download(np.uint32, m + 1), got[:total]), bf), f"after the errors, format {fmt}"
        # dead radii accept nothing
        for radius in (-1.0, float("nan")):
            assert go(radius=radius) == 0 and tot.value == 0 and not offs.download(np.uint32, m + 1).any()
        # n_queries == 0 on a built scene: d_offsets[0] = 0 and *total_out = 0
        offs.upload(guard_o)
        assert go(n=0) == 0 and tot.value == 0
        o = offs.download(np.uint32, m + 1)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes()
        scene.close(); unbuilt.close(); hits.free(); offs.free()
        for d in dm.values():
            d.free()
    finally:
        bl.close(); sc_ctx.close()


def test_one_instance_on_a_fresh_ctx(pkg):
    """a one-instance scene builds no top-level tree, so a fresh ctx has no arena yet: the first call reserves the smallest one"""
    mesh, inst, q, _ = small_scene(pkg)
    one = inst[1:].copy()
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(2, mesh)
        scene = pkg.Scene(sc_ctx).build(3, [b], one)
        bf = cached(("scene radius tris one",), lambda: scene_radius_tris_brute_force(pkg, q, [mesh], one, WIDE))
        assert bf["ill_pairs"] == 0 and len(bf["hits"]) > 50
        assert same(scene.radius_tris(q, radius=WIDE), bf)
        ioff = scene.radius_tris(instance=0, count_only=True)             # nobody else to answer: every row empty
        assert len(ioff) == len(mesh) + 1 and not ioff.any()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_binding_takes_every_input_kind(pkg):
    mesh, inst, q, _ = small_scene(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(3, mesh)
        rb = root_boxes(pkg, [b])
        scene = pkg.Scene(sc_ctx).build(3, [b], inst)
        bf = small_brute(pkg, WIDE, rb)
        want_o, want_h = scene.radius_tris(q, radius=WIDE)
        assert want_o.shape == (len(q) + 1,) and want_o.dtype == np.uint32 and want_h.dtype == pkg.INSTANCE_TRI_HIT and len(want_h) == want_o[-1] > 50
        assert same((want_o, want_h), bf)
        x = xyz(q)
        dm = {fmt: DeviceMesh(pkg, sc_ctx, q, fmt) for fmt in (0, 1, 2)}
        for o, h in (scene.radius_tris(x, radius=WIDE), scene.radius_tris(x.reshape(-1, 9), radius=WIDE), scene.radius_tris(x.astype(np.float64), radius=WIDE),
                     scene.radius_tris(dm[0].bufs[0], radius=WIDE), scene.radius_tris(dm[0].bufs[0].ptr, radius=WIDE, n=len(q)),
                     scene.radius_tris(dm[1].bufs[0], radius=WIDE, tri_format=pkg.TRI_PACKED36),
                     scene.radius_tris(vertices=dm[2].bufs[0], indices=dm[2].bufs[1], n_vertices=dm[2].inp.n_vertices, tri_format=pkg.TRI_INDEXED, radius=WIDE),
                     scene.radius_tris(q, radius=WIDE, capacity=len(want_h) + 5), scene.radius_tris(q, radius=WIDE, capacity=1)):      # (too small: re-allocated)
            assert o.tobytes() == want_o.tobytes() and h.tobytes() == want_h.tobytes()
        assert scene.radius_tris(dm[0].bufs[0], radius=WIDE, count_only=True).tobytes() == want_o.tobytes()
        uo, uh = scene.radius_tris(dm[0].bufs[0], radius=WIDE, sorted=False)
        assert uo.tobytes() == want_o.tobytes() and scene_radius_host_sort(uo, uh).tobytes() == want_h.tobytes()
        assert scene_radius_tris_recompute(pkg, q, [mesh], inst, WIDE, uo, uh) is None
        everything = small_brute(pkg, np.inf, rb)                         # radius None: +inf
        assert everything["ill_pairs"] == 0 and same(scene.radius_tris(q), everything)
        rows = as_triangles(pkg, instance_queries([mesh], inst, 1, len(mesh)))
        ibf = cached(("scene radius tris small rows",), lambda: scene_radius_tris_brute_force(pkg, rows, [mesh], inst, WIDE, skip=1))
        io, ih = scene.radius_tris(instance=1, radius=WIDE)
        assert ibf["ill_pairs"] == 0 and len(ih) > 50 and same((io, ih), ibf) and (ih["instance"] == 0).all()
        co, ch = scene.radius_tris(instance=1, radius=WIDE, n=40)
        assert co.tobytes() == io[:41].tobytes() and ch.tobytes() == ih[: int(io[40])].tobytes()
        for d in dm.values():
            d.free()
        for bad in (lambda: scene.radius_tris(np.zeros((4, 5), dtype=F32)), lambda: scene.radius_tris(4096), lambda: scene.radius_tris(),
                    lambda: scene.radius_tris(q, instance=0), lambda: scene.radius_tris(instance=2)):
            with pytest.raises(pkg.BvhError):
                bad()
        eo, eh = scene.radius_tris(q[:0])
        assert eo.tolist() == [0] and len(eh) == 0 and eh.dtype == pkg.INSTANCE_TRI_HIT and scene.radius_tris(q[:0], count_only=True).tolist() == [0]
        scene.close()
    finally:
        bl.close(); sc_ctx.close()
