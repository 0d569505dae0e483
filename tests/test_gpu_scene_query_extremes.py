"""The nine scene queries after bvh_scene_closest_point on the GPU — bvh_scene_knn, bvh_scene_radius_search, bvh_scene_intersect_all, bvh_scene_overlap,
bvh_scene_intersect_tris, bvh_scene_collide, bvh_scene_closest_tris, bvh_scene_radius_tris, bvh_scene_winding_prepare / _number — under the instance ladder of
tests/test_scene_extremes.py (inputs, brute forces and premises: tests/test_scene_query_extremes.py): uniform scales from 2^-64 to 2^64 and past them (s2 = 0, a
denormal, +inf), singular-value ratios up to 2^24, shears up to 2^10, rigid offsets up to 2^23, a mirrored shear, one scene whose s2 spans 2^120, one instance
alone, a deep BLAS through the stackless passes, and bvh_scene_update between tame and extreme matrices.  On every query: each record is an accepted candidate
with bit-equal fields, nothing lies below the brute force, lists ascend with the right padding, no inactive instance, no QUERY_MARK, reserved words 0;
count-only, sorted and unsorted fills agree, and a capacity one short of the total reports the total and fills nothing (the header's rule: the fill is skipped
on the device and the call returns 0).  On the well-conditioned queries (each query's own definition): byte-equal to the brute force, through the existing
checkers where the CPU file's EXACT says that the 99 % floor applies and through their uncapped twins elsewhere.  Relations between the entry points where the
same lines run.  The winding number: records byte-equal to the restatement at every scale, answers within check_walk's bound where the f32 restatement is
finite.  Run with -s for the per-rung figures."""
import numpy as np
import pytest

from test_gpu_intersect_tris import DeviceMesh
from test_gpu_scene_closest_tris import check_exact as check_closest_tris
from test_gpu_scene_closest_tris import raw as closest_tris_raw
from test_gpu_scene_collide import call as call_collide
from test_gpu_scene_collide import check_all_ways as collide_all_ways
from test_gpu_scene_extremes import TLAS, world                      # noqa: F401  (the module-scoped fixture: the two BLASes, built once)
from test_gpu_scene_intersect_tris import call as call_intersect_tris
from test_gpu_scene_intersect_tris import check_all_ways as intersect_tris_all_ways
from test_gpu_scene_winding import blas_trees, check_arrays, check_walk, download_top
from test_gpu_winding import TOL_FACTOR, TOL_FLOOR
from test_gpu_scene_radius_tris import call as call_radius_tris
from test_gpu_scene_radius_tris import check_all_ways as radius_tris_all_ways
from test_gpu_scene_radius_tris import search as radius_tris_search
from test_gpu_scene_knn import check_exact as check_knn
from test_gpu_scene_multihit import all_hits
from test_gpu_scene_multihit import call as call_rays
from test_gpu_scene_overlap import call as call_overlap
from test_gpu_scene_overlap import check_all_ways as overlap_all_ways
from test_gpu_scene_radius import call as call_radius
from test_gpu_scene_radius import check_all_ways as radius_all_ways
from test_gpu_scene_radius import search as radius_search
from test_knn import r2_of
from test_multihit import HITS_SORTED
from test_point_query import closest_formula, point_ok
from test_radius import slice_queries
from test_scene import tris_root_box, world_box
from test_scene_extremes import ONE_INSTANCE, RUNGS, S2_EDGES, meshes
from test_scene_knn import scene_knn_below, scene_knn_recompute
from test_scene_multihit import check_scene_all_hits
from test_scene_point import active_instances, world_culls, world_triangles
from test_scene_collide import SCENE_COLLIDE_BOTH, SCENE_COLLIDE_SORTED, collide_answer
from test_scene_closest_tris import SCENE_TRIS_INSTANCE, SCENE_TRIS_QUERY, scene_tris_dist_recompute, tris_dist_below
from test_scene_query_extremes import (EXACT, KS, TAME, TRI_RADII, asking_instances, closest_tris_reference, collide_reference, decided_at_the_top,
                                       intersect_tris_reference, knn_reference, overlap_reference, radius_reference, radius_tris_reference, rays_reference,
                                       tri_pairs)
from test_query import E_INVALID
from test_scene_query_extremes import BETAS, WIND_EXACT, WIND_RUNGS, near_tame, wind_brute_force, wind_scene, wind_selection
from test_scene_winding import scene_moments_host, scene_walk_host
from test_winding import WIND_NAN_BITS
from test_scene_extremes import DEEP_RUNGS
from test_scene_query_extremes import deep_reference, deep_scene, deep_tri_reference, deep_tri_scene, deep_wind_scene
from test_scene_radius_tris import SCENE_RADIUS_TRIS_SORTED, scene_radius_host_sort, scene_radius_tris_recompute
from test_scene_radius import RADIUS_SORTED, record_keys, scene_host_sort

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
F32 = np.float32
QUERY_MARK = 0xFFFFFFFE                                               # query.hpp: the word a query left to a stackless pass carries until that pass answers it


def no_mark(what, *arrays):
    for a in arrays:
        assert not (np.ascontiguousarray(a).view(np.uint32) == QUERY_MARK).any(), f"{what}: a QUERY_MARK is left in the output"


def rows_differ(a, b):
    return (a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1)


# ---- the uncapped twins of the checkers that carry the 99 % floor -------------------------------------------------------------------------------------------------

def knn_uncapped(pkg, pts, blas_tris, inst, bf, hits, counts, what):
    """test_gpu_scene_knn.check_exact without the 99 % floor: the unconditional guarantees on every query, exactness on whatever is well-conditioned"""
    k = hits.shape[1]
    well = bf["well"]
    bad = np.nonzero(rows_differ(hits, bf["hits"]) & well)[0]
    assert bad.size == 0, f"{what}, k = {k}: {bad.size} well-conditioned lists differ, e.g. query {bad[0]}: got {hits[bad[0]]} want {bf['hits'][bad[0]]}"
    assert np.array_equal(counts[well], bf["counts"][well]), f"{what}, k = {k}: counts differ"
    assert scene_knn_recompute(pkg, pts, blas_tris, inst, hits, counts).all(), f"{what}, k = {k}: an entry is not an accepted candidate, or order / padding / count is wrong"
    assert not scene_knn_below(pkg, hits, bf["hits"]).any(), f"{what}, k = {k}: a list below the brute force"


def radius_uncapped(pkg, points, blas_tris, instances, ref, offsets, hits, sorted_, what, exact_on=None):
    """test_scene_radius.check_scene_radius without the 99 % floor, assertion for assertion; exact_on (default: the well-conditioned queries) is the set on
    which the slices must equal the brute force's"""
    m = len(points)
    off = offsets.astype(np.int64)
    assert len(off) == m + 1 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(hits), f"{what}: offsets are not a scan of the slices"
    assert hits.dtype == pkg.INSTANCE_KNN_HIT and (hits["reserved"] == 0).all(), f"{what}: a reserved word is not 0"
    _, active = active_instances(instances, len(blas_tris))
    q = slice_queries(offsets)
    ins, prim = hits["instance"].astype(np.int64), hits["prim"].astype(np.int64)
    assert (ins < len(instances)).all() and active[ins].all(), f"{what}: a record of an inactive or a missing instance"
    sizes = np.array([len(blas_tris[int(b)]) if b < len(blas_tris) else 0 for b in instances["blas"]], dtype=np.int64)
    assert (prim < sizes[ins]).all(), f"{what}: a primitive index out of range"
    r2, ok = r2_of(points), point_ok(points)
    good = np.zeros(len(hits), dtype=bool)
    for i in np.unique(ins):
        sel = np.nonzero(ins == i)[0]
        V1, V2, V3 = world_triangles(instances["object_to_world"][i], blas_tris[int(instances["blas"][i])][prim[sel]])
        _, d2, _, _, _ = closest_formula(np.ascontiguousarray(points["point"][q[sel]], dtype=F32), V1, V2, V3)
        with np.errstate(invalid="ignore"):
            acc = (d2 <= r2[q[sel]]) & ok[q[sel]]
        good[sel] = acc & (d2.view(np.uint32) == np.ascontiguousarray(hits["dist2"][sel]).view(np.uint32))
    assert good.all(), f"{what}: {np.count_nonzero(~good)} records are not accepted candidates of their (instance, prim) with a bit-equal dist2"
    span = int(sizes.max()) if len(sizes) else 1
    key = (q * len(instances) + ins) * span + prim
    assert len(np.unique(key)) == len(key), f"{what}: an (instance, prim) pair appears twice in a slice"
    ref_q = slice_queries(ref["offsets"])
    ref_key = (ref_q * len(instances) + ref["hits"]["instance"].astype(np.int64)) * span + ref["hits"]["prim"].astype(np.int64)
    assert np.isin(key, ref_key).all(), f"{what}: a slice is not a subset of the true set"
    if sorted_ and len(hits) > 1:
        nxt = q[1:] == q[:-1]
        k64, k32 = record_keys(hits)
        asc = (k64[1:] > k64[:-1]) | ((k64[1:] == k64[:-1]) & (k32[1:] > k32[:-1]))
        assert asc[nxt].all(), f"{what}: {np.count_nonzero(~asc & nxt)} slices are not strictly ascending in (dist2, instance, prim)"
    well = ref["well"] if exact_on is None else exact_on
    counts, ref_counts = np.diff(off), np.diff(ref["offsets"].astype(np.int64))
    assert (counts == ref_counts)[well].all(), f"{what}: counts differ on {np.count_nonzero((counts != ref_counts) & well)} queries that must be exact"
    got = hits if sorted_ else scene_host_sort(offsets, hits)
    assert got[well[q]].tobytes() == ref["hits"][well[ref_q]].tobytes(), f"{what}: the slices of the queries that must be exact differ from the brute force"


def radius_all_ways_uncapped(pkg, scene, pts, blas_tris, inst, ref, what, exact_on=None):
    """test_gpu_scene_radius.check_all_ways through radius_uncapped"""
    off, hits = radius_search(pkg, scene, pts, RADIUS_SORTED)
    radius_uncapped(pkg, pts, blas_tris, inst, ref, off, hits, True, what + " sorted", exact_on)
    uoff, uhits = radius_search(pkg, scene, pts, 0)
    assert uoff.tobytes() == off.tobytes(), f"{what}: sorted and unsorted calls count differently"
    assert scene_host_sort(uoff, uhits).tobytes() == hits.tobytes(), f"{what}: the unsorted slices are not the sorted ones as sets"
    uoff2, uhits2 = radius_search(pkg, scene, pts, 0)
    assert uoff2.tobytes() == uoff.tobytes() and uhits2.tobytes() == uhits.tobytes(), f"{what}: the same unsorted call twice gives other bytes"
    return off, hits


def slices_differ(off, recs, ref_off, ref_recs):
    """per query: the slice's bytes differ from the reference's"""
    o, r = off.astype(np.int64), ref_off.astype(np.int64)
    out = np.diff(o) != np.diff(r)
    for i in np.nonzero(~out)[0]:
        out[i] = recs[o[i]:o[i + 1]].tobytes() != ref_recs[r[i]:r[i + 1]].tobytes()
    return out


def one_short(pkg, ctx, call, scene, queries, flags, off, total, rec_bytes, what):
    """a capacity one short of the total: the call reports the right total and complete offsets, and writes nothing to the records (the header: the fill is
    skipped on the device)"""
    if total == 0:
        return
    guard = np.full(total * rec_bytes, 0xA5, dtype=np.uint8)
    d_q, d_off, d_rec = ctx.upload(queries), ctx.alloc((len(queries) + 1) * 4), ctx.upload(guard)
    try:
        rc, t = call(pkg, scene, d_q.ptr, len(queries), flags, d_off.ptr, d_rec.ptr, total - 1)
        assert (rc, t) == (0, total), f"{what}: capacity total - 1 returned {rc}, total {t} for {total}"
        assert d_off.download(np.uint32, len(queries) + 1).tobytes() == off.tobytes(), f"{what}: capacity total - 1 left other offsets"
        assert d_rec.download(np.uint8, len(guard)).tobytes() == guard.tobytes(), f"{what}: capacity total - 1 wrote records"
    finally:
        d_q.free(); d_off.free(); d_rec.free()


def build(pkg, sc_ctx, blases, inst, tl, one=False):
    scene = pkg.Scene(sc_ctx).build(tl, blases, inst)
    assert (scene.tlas().d_nodes is None) == one
    return scene


# ---- bvh_scene_knn ------------------------------------------------------------------------------------------------------------------------------------------------

def knn_checks(pkg, scene, name, pts, inst, what, one=False):
    outs = {}
    cp = scene.closest_point(pts, query="closest")
    for k in KS:
        bf = knn_reference(pkg, name, k, one)[2]
        hits, counts = scene.knn(pts, k)
        ill = ~bf["well"]
        print(f"knn    {what:32s} k = {k:2d}: lists {int((bf['counts'] > 0).sum()):4d}  well {bf['well'].mean():.4f}  ill-conditioned {int(ill.sum()):3d}, "
              f"{int((rows_differ(hits, bf['hits']) & ill).sum())} of them answered differently")
        if name in EXACT["knn"]:
            check_knn(pkg, pts, meshes(pkg), inst, bf, hits, counts, what)
        knn_uncapped(pkg, pts, meshes(pkg), inst, bf, hits, counts, what)
        no_mark(what, hits, counts)
        outs[k] = hits
    got = outs[1][:, 0]                                               # k = 1 is bvh_scene_closest_point's walk: every query, well-conditioned or not
    assert got["dist2"].tobytes() == cp["dist2"].tobytes() and np.array_equal(got["prim"], cp["prim"]) and np.array_equal(got["instance"], cp["instance"]), \
        f"{what}: k = 1 differs from bvh_scene_closest_point"
    return outs


@pytest.mark.parametrize("name", RUNGS)
def test_knn_ladder(world, name):
    """k = 1, 8 and 32 under both top-level builders, which must agree byte for byte on the well-conditioned lists; three rungs also with one instance alone"""
    pkg, sc_ctx, blases, _ = world
    inst, pts, bf = knn_reference(pkg, name)
    outs = []
    for tl in TLAS:
        scene = build(pkg, sc_ctx, blases, inst, tl)
        outs.append(knn_checks(pkg, scene, name, pts, inst, f"{name} top-level builder {tl}"))
        scene.close()
    well = bf["well"]
    for k in KS:
        assert outs[0][k][well].tobytes() == outs[1][k][well].tobytes(), f"{name}, k = {k}: the two top-level builders differ"
    if name in ONE_INSTANCE:
        inst1, pts1, _ = knn_reference(pkg, name, one=True)
        scene = build(pkg, sc_ctx, blases, inst1, 3, one=True)
        knn_checks(pkg, scene, name, pts1, inst1, f"{name} one instance", one=True)
        scene.close()


# ---- bvh_scene_radius_search --------------------------------------------------------------------------------------------------------------------------------------

def radius_checks(pkg, sc_ctx, scene, floor, pts, inst, ref, what, exact_on=None):
    """floor: the 99 % floor applies (the existing checker runs as well as its uncapped twin)"""
    if floor and exact_on is None:
        radius_all_ways(pkg, scene, pts, meshes(pkg), inst, ref, what)
    off, hits = radius_all_ways_uncapped(pkg, scene, pts, meshes(pkg), inst, ref, what, exact_on)
    ill = ~ref["well"]
    print(f"radius {what:32s} records {len(ref['hits']):7d}  well {ref['well'].mean():.4f}  ill-conditioned {int(ill.sum()):3d}, "
          f"{int((slices_differ(off, hits, ref['offsets'], ref['hits']) & ill).sum())} of them answered differently")
    no_mark(what, off, hits)
    for flags in (RADIUS_SORTED, 0):
        one_short(pkg, sc_ctx, call_radius, scene, pts, flags, off, int(off[-1]), 16, what)
    # the first min(8, count) sorted records are the k = 8 list of the same points (a well-conditioned slice makes each of its entries well-conditioned)
    lists, counts = scene.knn(pts, 8)
    o = off.astype(np.int64)
    want = np.minimum(np.diff(o), 8)
    sel = ref["well"] if exact_on is None else exact_on
    assert np.array_equal(counts[sel], want[sel]), f"{what}: the k = 8 counts differ from min(8, slice length)"
    for i in np.nonzero(sel)[0]:
        assert hits[o[i]: o[i] + want[i]].tobytes() == lists[i, : want[i]].tobytes(), f"{what}, query {i}: the sorted prefix is not bvh_scene_knn's list"
    return off, hits


@pytest.mark.parametrize("name", RUNGS)
def test_radius_ladder(world, name):
    pkg, sc_ctx, blases, _ = world
    inst, pts, ref = radius_reference(pkg, name)
    outs = []
    for tl in TLAS:
        scene = build(pkg, sc_ctx, blases, inst, tl)
        outs.append(radius_checks(pkg, sc_ctx, scene, name in EXACT["radius"], pts, inst, ref, f"{name} top-level builder {tl}"))
        scene.close()
    same = ~slices_differ(outs[0][0], outs[0][1], outs[1][0], outs[1][1])
    assert same[ref["well"]].all(), f"{name}: the two top-level builders differ"
    if name in ONE_INSTANCE:
        inst1, pts1, ref1 = radius_reference(pkg, name, one=True)
        scene = build(pkg, sc_ctx, blases, inst1, 3, one=True)
        radius_checks(pkg, sc_ctx, scene, name in EXACT["radius"], pts1, inst1, ref1, f"{name} one instance")
        scene.close()


# ---- bvh_scene_intersect_all --------------------------------------------------------------------------------------------------------------------------------------

def rays_checks(pkg, sc_ctx, scene, floor, rays, inst, ref, what):
    """floor: at least 99 % of the rays must be well-conditioned"""
    well = ref["well"]
    if floor:
        assert well.mean() >= 0.99, f"{what}: only {well.mean():.4f} of the rays are well-conditioned"
    off, hits = all_hits(pkg, scene, rays, HITS_SORTED)
    check_scene_all_hits(pkg, rays, meshes(pkg), inst, ref, off, hits, True, what + " sorted")
    uoff, uhits = all_hits(pkg, scene, rays, 0)
    assert uoff.tobytes() == off.tobytes(), f"{what}: sorted and unsorted calls count differently"
    check_scene_all_hits(pkg, rays, meshes(pkg), inst, ref, uoff, uhits, False, what + " unsorted")
    order = np.lexsort((uhits["prim"], uhits["instance"], uhits["t"], slice_queries(uoff)))
    assert uhits[order].tobytes() == hits.tobytes(), f"{what}: the sorted fill is not the sort of the unsorted one"
    print(f"rays   {what:32s} records {len(ref['hits']):7d}  well {well.mean():.4f}  ill-conditioned {int((~well).sum()):3d}, "
          f"{int((slices_differ(off, hits, ref['offsets'], ref['hits']) & ~well).sum())} of them answered differently")
    no_mark(what, off, hits, uhits)
    for flags in (HITS_SORTED, 0):
        one_short(pkg, sc_ctx, call_rays, scene, rays, flags, off, int(off[-1]), 32, what)
    closest = scene.intersect(rays, "closest")
    empty = np.diff(off.astype(np.int64)) == 0
    assert (empty == (closest["prim"] == pkg.INVALID))[well].all(), f"{what}: empty slices and closest-hit misses differ"
    has = ~empty & well
    assert has.sum() > (100 if floor else 0) and hits[off[:-1][has]].tobytes() == closest[has].tobytes(), f"{what}: first sorted record != bvh_scene_intersect closest"
    return off, hits


@pytest.mark.parametrize("name", RUNGS)
def test_intersect_all_ladder(world, name):
    pkg, sc_ctx, blases, _ = world
    inst, rays, ref = rays_reference(pkg, name)
    outs = []
    for tl in TLAS:
        scene = build(pkg, sc_ctx, blases, inst, tl)
        outs.append(rays_checks(pkg, sc_ctx, scene, name in EXACT["rays"], rays, inst, ref, f"{name} top-level builder {tl}"))
        scene.close()
    same = ~slices_differ(outs[0][0], outs[0][1], outs[1][0], outs[1][1])
    assert same[ref["well"]].all(), f"{name}: the two top-level builders differ"


# ---- bvh_scene_overlap ----------------------------------------------------------------------------------------------------------------------------------------------

def overlap_checks(pkg, sc_ctx, scene, boxes, touching, ref, what):
    """exact on every box: bvh_scene_overlap has no ill-conditioned queries"""
    off, recs = overlap_all_ways(pkg, scene, boxes, ref, what)
    print(f"boxes  {what:32s} records {len(recs):7d}  exact on every box")
    lens = np.diff(off.astype(np.int64))
    assert (lens[touching] >= 1).all() and (lens[-4:] == 0).all()
    no_mark(what, off, recs)
    for flags in (1, 0):
        one_short(pkg, sc_ctx, call_overlap, scene, boxes, flags, off, int(off[-1]), 8, what)
    return off, recs


@pytest.mark.parametrize("name", RUNGS + S2_EDGES)
def test_overlap_ladder(world, name):
    pkg, sc_ctx, blases, _ = world
    inst, boxes, touching, ref = overlap_reference(pkg, name)
    for tl in TLAS:
        scene = build(pkg, sc_ctx, blases, inst, tl)
        overlap_checks(pkg, sc_ctx, scene, boxes, touching, ref, f"{name} top-level builder {tl}")
        scene.close()
    if name in ONE_INSTANCE:
        inst1, boxes1, touching1, ref1 = overlap_reference(pkg, name, one=True)
        scene = build(pkg, sc_ctx, blases, inst1, 3, one=True)
        overlap_checks(pkg, sc_ctx, scene, boxes1, touching1, ref1, f"{name} one instance")
        scene.close()


# ---- past the s2 edges ------------------------------------------------------------------------------------------------------------------------------------------------

def radius_decided_at_the_top(pkg, pts, inst, ref):
    """under s2 = 0 nothing is culled inside an instance, so a slice is decided by the restated rule iff the top-level rule keeps the world box of every
    instance that has a record in the true slice at the query's own bound r2"""
    out = np.ones(len(pts), dtype=bool)
    q = slice_queries(ref["offsets"])
    r2 = r2_of(pts)
    for k in range(len(inst)):
        wb = world_box(inst["object_to_world"][k], tris_root_box(meshes(pkg)[int(inst["blas"][k])]))
        qi = np.unique(q[ref["hits"]["instance"] == k])
        out[qi] &= ~world_culls(wb, pts["point"][qi], r2[qi])
    return out


@pytest.mark.parametrize("name", S2_EDGES)
def test_s2_edges(world, name):
    """s2 = +inf (2^65), a deep denormal (2^-65) and 0 (2^-75); the instances stay active.  The unconditional guarantees, count == fill and the relations
    between the entry points on every query; exactness on whatever the header still calls well-conditioned; under s2 = 0 also on the queries that the restated
    top-level rule decides (knn k = 1 and the radius search, as test_gpu_scene_extremes.test_s2_edges has it for bvh_scene_closest_point).  The rays do not read
    s2 and are exact."""
    pkg, sc_ctx, blases, _ = world
    inst, pts, _ = knn_reference(pkg, name)
    _, rpts, rref = radius_reference(pkg, name)
    _, rays, yref = rays_reference(pkg, name)
    for tl in TLAS:
        what = f"{name} top-level builder {tl}"
        scene = build(pkg, sc_ctx, blases, inst, tl)
        outs = knn_checks(pkg, scene, name, pts, inst, what)
        off, hits = radius_checks(pkg, sc_ctx, scene, False, rpts, inst, rref, what)
        if name == "uni_2p-75":
            bf1 = knn_reference(pkg, name, 1)[2]
            decided = decided_at_the_top(pkg, pts, inst, bf1["hits"])
            assert decided.mean() >= 0.99
            bad = rows_differ(outs[1], bf1["hits"]) & decided
            assert not bad.any(), f"{what}: k = 1 differs on {bad.sum()} lists that the restated rule decides (first {np.nonzero(bad)[0][:6]})"
            rdec = radius_decided_at_the_top(pkg, rpts, inst, rref)
            print(f"radius {what:32s} the restated top-level rule decides {int(rdec.sum())} of {len(rpts)} slices")
            assert (rdec | ~rref["well"]).all() and rdec.mean() >= 0.99
            radius_uncapped(pkg, rpts, meshes(pkg), inst, rref, off, hits, True, what + " decided at the top", rdec)
        rays_checks(pkg, sc_ctx, scene, True, rays, inst, yref, what)             # (the rays do not read s2: held to the floor at every uniform scale)
        scene.close()


# ---- bvh_scene_update between extremes ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uni_2p-64", "uni_2p64", "ratio_2p16", "far_2p23", "mixed"])
def test_update_between_extremes(world, name):
    """a scene built on the rung, updated to tame matrices and back: after each step the radius search (the s2 path) and the box query (the matrix path) answer
    as a scene freshly built on that step's matrices — byte for byte on the well-conditioned points (the update keeps the topology of the build, a fresh build
    chooses its own: the ill-conditioned answers may differ) and on every box — and exactly against the brute force"""
    pkg, sc_ctx, blases, _ = world
    states = {}
    for s in (name, TAME):
        inst, pts, ref = radius_reference(pkg, s)
        _, boxes, touching, oref = overlap_reference(pkg, s)
        states[s] = (inst, pts, ref, boxes, touching, oref)
    scene = build(pkg, sc_ctx, blases, states[name][0], 3)
    for step, s in (("built on the rung", name), ("updated to tame", TAME), ("updated back", name)):
        inst, pts, ref, boxes, touching, oref = states[s]
        what = f"{name}, {step}"
        if step != "built on the rung":
            scene.update(inst)
        off, hits = radius_checks(pkg, sc_ctx, scene, s == TAME or s in EXACT["radius"], pts, inst, ref, what)
        ooff, orecs = overlap_checks(pkg, sc_ctx, scene, boxes, touching, oref, what)
        fresh = build(pkg, sc_ctx, blases, inst, 3)
        foff, fhits = fresh.radius_search(pts)
        fooff, forecs = fresh.overlap(boxes)
        fresh.close()
        assert not (slices_differ(off, hits, foff, fhits) & ref["well"]).any(), f"{what}: the radius search differs from a fresh build"
        assert ooff.tobytes() == fooff.tobytes() and orecs.tobytes() == forecs.tobytes(), f"{what}: the box query differs from a fresh build"
    scene.close()


# ---- the triangle queries: bvh_scene_intersect_tris, bvh_scene_collide, bvh_scene_closest_tris, bvh_scene_radius_tris ------------------------------------------------

def one_short_of(ctx, do, n_rows, off, rec_bytes, what):
    """one_short for the calls that take a query mesh or an instance: do(d_offsets, d_records, capacity) -> (rc, total)"""
    total = int(off[-1])
    if total == 0:
        return
    guard = np.full(total * rec_bytes, 0xA5, dtype=np.uint8)
    d_off, d_rec = ctx.alloc((n_rows + 1) * 4), ctx.upload(guard)
    try:
        rc, t = do(d_off.ptr, d_rec.ptr, total - 1)
        assert (rc, t) == (0, total), f"{what}: capacity total - 1 returned {rc}, total {t} for {total}"
        assert d_off.download(np.uint32, n_rows + 1).tobytes() == off.tobytes(), f"{what}: capacity total - 1 left other offsets"
        assert d_rec.download(np.uint8, len(guard)).tobytes() == guard.tobytes(), f"{what}: capacity total - 1 wrote records"
    finally:
        d_off.free(); d_rec.free()


def collide_one_short(pkg, ctx, scene, full, what):
    """bvh_scene_collide with a capacity one short of the total, default and BOTH, sorted and unsorted: the call reports the rows and the total, d_row_first and
    d_offsets are complete, and no record is written"""
    n_inst = scene.n_instances
    for both in (False, True):
        ref_first, ref_off, ref_recs = collide_answer(full, both)
        n_rows, total = int(ref_first[-1]), len(ref_recs)
        if total == 0:
            continue
        guard = np.full(total * 8, 0xA5, dtype=np.uint8)
        for flags in ((SCENE_COLLIDE_BOTH if both else 0) | SCENE_COLLIDE_SORTED, SCENE_COLLIDE_BOTH if both else 0):
            d_first, d_off, d_rec = ctx.alloc((n_inst + 1) * 4), ctx.alloc((n_rows + 1) * 4), ctx.upload(guard)
            try:
                rc, rows, t = call_collide(pkg, scene, flags, d_first.ptr, n_rows, d_off.ptr, d_rec.ptr, total - 1)
                assert (rc, rows, t) == (0, n_rows, total), f"{what}, flags {flags}: capacity total - 1 returned {rc}, rows {rows}, total {t} for {n_rows}, {total}"
                assert d_first.download(np.uint32, n_inst + 1).tobytes() == ref_first.tobytes(), f"{what}, flags {flags}: capacity total - 1 left another row_first"
                assert d_off.download(np.uint32, n_rows + 1).tobytes() == ref_off.tobytes(), f"{what}, flags {flags}: capacity total - 1 left other offsets"
                assert d_rec.download(np.uint8, len(guard)).tobytes() == guard.tobytes(), f"{what}, flags {flags}: capacity total - 1 wrote records"
            finally:
                d_first.free(); d_off.free(); d_rec.free()


def tri_modes(pkg, sc_ctx, name, one=False):
    """[(what, rows_of, the query mesh on the device or None, mode, k)]: the query mesh (format 1), then every asking instance"""
    dm = DeviceMesh(pkg, sc_ctx, tri_pairs(pkg, name, None, one)[1], 1)
    out = [("query mesh", None, dm, SCENE_TRIS_QUERY, 0)]
    if not one:
        out += [(f"instance {k} asks", k, None, SCENE_TRIS_INSTANCE, k) for k in asking_instances(name)]
    return out


@pytest.mark.parametrize("name", RUNGS + S2_EDGES)
def test_intersect_tris_and_collide_ladder(world, name):
    """exact on every query and every row at every rung and past the s2 edges: the crossing predicate is the header's f64 one on the f32 world coordinates and
    the box rule is the mapped box; neither reads s2.  bvh_scene_collide's rows are bvh_scene_intersect_tris(INSTANCE, k)'s, row for row, for every k"""
    pkg, sc_ctx, blases, _ = world
    inst, full = collide_reference(pkg, name)
    for tl in TLAS:
        scene = build(pkg, sc_ctx, blases, inst, tl)
        for label, rows_of, dm, mode, k in tri_modes(pkg, sc_ctx, name):
            what = f"{name} top-level builder {tl}, {label}"
            _, q, ref = intersect_tris_reference(pkg, name, rows_of)
            off, recs = intersect_tris_all_ways(pkg, scene, q if dm is not None else None, ref, what, fmt=2, instance=rows_of, rows=len(q))
            print(f"x-tris {what:48s} records {len(recs):6d} in {int(np.count_nonzero(np.diff(off.astype(np.int64)))):3d} slices  exact on every query")
            no_mark(what, off, recs)
            assert rows_of is None or rows_of not in recs["instance"]
            qin = dm.inp if dm is not None else None
            for flags in (1, 0):
                one_short_of(sc_ctx, lambda o, r, cap: call_intersect_tris(pkg, scene, qin, len(q), mode, k, flags, o, r, cap), len(q), off, 8, what)
            if dm is not None:
                dm.free()
        what = f"{name} top-level builder {tl}"
        got = collide_all_ways(pkg, scene, full, what)
        first, off, recs = got[True]
        print(f"collide {what:47s} rows {int(first[-1]):5d}  records {len(recs):6d}  exact on every row")
        no_mark(what, first, off, recs, got[False][1], got[False][2])
        collide_one_short(pkg, sc_ctx, scene, full, what)
        o = off.astype(np.int64)
        for k in range(len(inst)):
            ioff, irecs = scene.intersect_tris(instance=k)                # (300 rows: as many as the largest BLAS has leaves)
            lo, hi = int(first[k]), int(first[k + 1])
            assert (o[lo:hi + 1] - o[lo]).tolist() == ioff[: hi - lo + 1].astype(np.int64).tolist(), f"{what}, instance {k}: collide's offsets are not the instance call's"
            assert ioff[hi - lo] == ioff[-1] and recs[o[lo]:o[hi]].tobytes() == irecs.tobytes(), f"{what}, instance {k}: collide's rows are not the instance call's"
        scene.close()


def closest_tris_uncapped(pkg, q, blas_tris, inst, radius, bf, closest, anyhit, what, skip=None):
    """test_gpu_scene_closest_tris.check_exact without the 99 % floor"""
    well, ref = bf["well"], bf["closest"]
    diff = rows_differ(closest, ref)
    assert not (diff & well).any(), (f"{what}: closest differs on {np.count_nonzero(diff & well)} well-conditioned queries (first {np.nonzero(diff & well)[0][:6]}: "
                                     f"got {closest[diff & well][:3]} want {ref[diff & well][:3]})")
    assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"])[well].all(), f"{what}: any hit/miss differs"
    for kind, out in (("closest", closest), ("any", anyhit)):
        assert scene_tris_dist_recompute(pkg, q, blas_tris, inst, radius, out, skip=skip).all(), \
            f"{what}: a {kind} record is not an accepted candidate of its (instance, prim) (or not the miss record)"
        assert skip is None or skip not in set(out["instance"][out["prim"] != pkg.INVALID].tolist()), f"{what}: the query instance answered"
    assert not tris_dist_below(pkg, closest, ref).any(), f"{what}: closest below the brute force"


def closest_tris_checks(pkg, sc_ctx, scene, name, what, one=False):
    for label, rows_of, dm, mode, k in tri_modes(pkg, sc_ctx, name, one):
        qin = dm.inp if dm is not None else None
        for rl in TRI_RADII:
            inst, q, radius, bf = closest_tris_reference(pkg, name, rl, rows_of, one)
            w = f"{what}, {label}, radius {rl}"
            c = closest_tris_raw(pkg, scene, qin, len(q), mode, k, radius, pkg.QUERY_CLOSEST)
            a = closest_tris_raw(pkg, scene, qin, len(q), mode, k, radius, pkg.QUERY_ANY)
            ill = ~bf["well"]
            print(f"c-tris {w:64s} hits {int(bf['hit'].sum()):3d}  well {bf['well'].mean():.4f}  ill-conditioned {int(ill.sum()):3d}, "
                  f"{int((rows_differ(c, bf['closest']) & ill).sum())} of them answered differently")
            if name in EXACT["closest_tris"]:
                check_closest_tris(pkg, q, meshes(pkg), inst, radius, bf, c, a, w, skip=rows_of)
            closest_tris_uncapped(pkg, q, meshes(pkg), inst, radius, bf, c, a, w, skip=rows_of)
            no_mark(w, c, a)
        if dm is not None:
            dm.free()


@pytest.mark.parametrize("name", RUNGS + S2_EDGES)
def test_closest_tris_ladder(world, name):
    """CLOSEST and ANY at radius +inf, a band and 0, from a query mesh and from the asking instances; three rungs also with one instance alone.  Past the s2
    edges: the unconditional guarantees, and exactness on whatever the header still calls well-conditioned"""
    pkg, sc_ctx, blases, _ = world
    inst = tri_pairs(pkg, name)[0]
    for tl in TLAS:
        scene = build(pkg, sc_ctx, blases, inst, tl)
        closest_tris_checks(pkg, sc_ctx, scene, name, f"{name} top-level builder {tl}")
        scene.close()
    if name in ONE_INSTANCE:
        scene = build(pkg, sc_ctx, blases, tri_pairs(pkg, name, None, True)[0], 3, one=True)
        closest_tris_checks(pkg, sc_ctx, scene, name, f"{name} one instance", one=True)
        scene.close()


def tri_slices_differ(off, hits, bf):
    return slices_differ(off, hits, bf["offsets"], bf["hits"])


def radius_tris_uncapped(pkg, scene, q, blas_tris, inst, radius, bf, what, qin, mode, k):
    """test_gpu_scene_radius_tris.check_all_ways without its gate (no ill-conditioned pair at all): count-only, sorted and unsorted fills agree; every record is
    an accepted candidate with bit-equal fields; every slice is a subset of the truth, a sorted one strictly ascending; the well-conditioned queries' slices
    are the brute force's bytes.  Returns the sorted answer"""
    m, skip = len(q), (k if mode == SCENE_TRIS_INSTANCE else None)
    off, hits = radius_tris_search(pkg, scene, qin, m, mode, k, radius, SCENE_RADIUS_TRIS_SORTED)
    uoff, uhits = radius_tris_search(pkg, scene, qin, m, mode, k, radius, 0)
    assert uoff.tobytes() == off.tobytes(), f"{what}: sorted and unsorted calls count differently"
    assert scene_radius_host_sort(uoff, uhits).tobytes() == hits.tobytes(), f"{what}: the sorted fill is not the sort of the unsorted one"
    for o, h in ((off, hits), (uoff, uhits)):
        said = scene_radius_tris_recompute(pkg, q, blas_tris, inst, radius, o, h, skip=skip)
        assert said is None, f"{what}: {said}"
    rows, ref_rows = slice_queries(off), slice_queries(bf["offsets"])
    key = (rows * len(inst) + hits["instance"].astype(np.int64)) * 300 + hits["prim"].astype(np.int64)
    ref_key = (ref_rows * len(inst) + bf["hits"]["instance"].astype(np.int64)) * 300 + bf["hits"]["prim"].astype(np.int64)
    assert np.isin(key, ref_key).all(), f"{what}: a slice is not a subset of the true set"
    bad = tri_slices_differ(off, hits, bf) & bf["well"]
    assert not bad.any(), f"{what}: {bad.sum()} well-conditioned slices differ from the brute force (first {np.nonzero(bad)[0][:6]})"
    return off, hits


@pytest.mark.parametrize("name", RUNGS + S2_EDGES)
def test_radius_tris_ladder(world, name):
    """one finite radius per call (about 20 accepted pairs per live query), from a query mesh and from the asking instances.  QUERY_ANY of
    bvh_scene_closest_tris at the same radius hits exactly where the row is not empty, on the well-conditioned queries"""
    pkg, sc_ctx, blases, _ = world
    inst = tri_pairs(pkg, name)[0]
    for tl in TLAS:
        scene = build(pkg, sc_ctx, blases, inst, tl)
        for label, rows_of, dm, mode, k in tri_modes(pkg, sc_ctx, name):
            _, q, radius, bf = radius_tris_reference(pkg, name, rows_of)
            qin = dm.inp if dm is not None else None
            what = f"{name} top-level builder {tl}, {label}"
            if name in EXACT["radius_tris"]:
                assert bf["well"].mean() >= 0.99, f"{what}: only {bf['well'].mean():.4f} of the queries are well-conditioned"
            if bf["ill_pairs"] == 0:
                radius_tris_all_ways(pkg, scene, q, meshes(pkg), inst, radius, bf, what, qin=qin, mode=mode, k=k)
            off, hits = radius_tris_uncapped(pkg, scene, q, meshes(pkg), inst, radius, bf, what, qin, mode, k)
            ill = ~bf["well"]
            print(f"r-tris {what:56s} records {len(bf['hits']):6d}  well {bf['well'].mean():.4f}  ill-conditioned {int(ill.sum()):3d}, "
                  f"{int((tri_slices_differ(off, hits, bf) & ill).sum())} of them answered differently")
            no_mark(what, off, hits)
            for flags in (SCENE_RADIUS_TRIS_SORTED, 0):
                one_short_of(sc_ctx, lambda o, r, cap: call_radius_tris(pkg, scene, qin, len(q), mode, k, radius, flags, o, r, cap), len(q), off, 16, what)
            a = closest_tris_raw(pkg, scene, qin, len(q), mode, k, radius, pkg.QUERY_ANY)
            nonempty = np.diff(off.astype(np.int64)) > 0
            assert ((a["prim"] != pkg.INVALID) == nonempty)[bf["well"]].all(), f"{what}: QUERY_ANY hits differ from the non-empty rows"
            if dm is not None:
                dm.free()
        scene.close()


# ---- bvh_scene_winding_prepare / bvh_scene_winding_number ----------------------------------------------------------------------------------------------------------

def winding_checks(pkg, name, trees, inst, top, host, pts, got, beta, what, exact):
    """on every rung: a NaN point answers the canonical NaN, no answer carries the mark, and a live query whose f32 restatement (on the scene's own trees) is
    finite has a finite answer.  Where ``exact``: test_gpu_scene_winding.check_walk's bound — |GPU - f64 host walk| <= 8 x max |f32 host walk - f64 host walk|,
    floor 2^-20, and at beta = +inf the same bound against the f64 brute force — on every query farther than 1e-4 diagonals from the surface whose restatement
    is finite; in the mixed scene also, with a bound of their own, on the queries within two world sizes of the tame instances"""
    xyz = pts["point"]
    dead = np.isnan(xyz).any(axis=1)
    assert (got.view(np.uint32)[dead] == WIND_NAN_BITS).all(), f"{what}: a NaN point does not answer the canonical NaN"
    no_mark(what, got)
    with np.errstate(all="ignore"):
        w64 = scene_walk_host(pkg, trees, inst, top, host, xyz, beta, np.float64)
        w32 = scene_walk_host(pkg, trees, inst, top, host, xyz, beta, np.float32)
    fin = np.isfinite(w32) & ~dead
    assert np.isfinite(got[fin]).all(), f"{what} beta {beta}: {np.count_nonzero(~np.isfinite(got[fin]))} queries with a finite f32 restatement have no finite answer"
    print(f"wind   {what:32s} beta {beta}: finite restatement on {fin.sum():4d} of {int((~dead).sum())} live queries, finite answer on {int(np.isfinite(got[~dead]).sum()):4d}", end="")
    if not exact:
        print()
        return
    assert fin.sum() >= 0.99 * (~dead).sum(), f"{what}: only {fin.sum()} finite restatements"
    sel = wind_selection(pkg, name, w32) & np.isfinite(w64)
    bf = wind_brute_force(pkg, name)
    # (how much of a rung the bound covers is the inputs' doing and is asserted on the CPU: test_scene_query_extremes.test_wind_bounded_share.  The second subset
    # of the mixed scene is bounded by the f32 restatement's own error there, which is of order 1 — the giant's world vertices have an ulp of 64 — so on it
    # this is a finiteness check; what shows that the giant does not cost its neighbours their answers is winding_is_additive)
    subsets = [("every query", sel)] + ([("near the tame instances", np.isfinite(w32) & np.isfinite(w64) & near_tame(pkg, pts))] if name == "mixed" else [])
    print(f"; bounded share {sel.sum() / max(int(fin.sum()), 1):.3f}", end="")
    for label, s in subsets:
        assert s.sum() >= 100, f"{what}, {label}: {s.sum()} queries"
        tol = max(TOL_FACTOR * float(np.abs(w32[s].astype(np.float64) - w64[s]).max()), TOL_FLOOR)
        err = float(np.abs(got[s].astype(np.float64) - w64[s]).max())
        print(f"; {label} ({s.sum()}): |gpu - host f64| max {err:.3e}, tol {tol:.3e}", end="")
        assert err <= tol, f"{what} beta {beta}, {label}: {err:.3e} > {tol:.3e}"
        if np.isinf(beta):
            err = float(np.abs(got[s].astype(np.float64) - bf[s]).max())
            assert err <= tol, f"{what} beta inf against the brute force, {label}: {err:.3e} > {tol:.3e}"
    print()


def winding_is_additive(pkg, sc_ctx, blases, inst, pts, got, what):
    """beta = +inf: the scene's answer is the f64 sum of the f32 solid angles of every world triangle, rounded once, and a world triangle's term does not depend
    on which other instances the scene holds.  So the answer equals the sum of the answers of the one-instance scenes up to those roundings: one of 2^-24
    relative per answer (seven of them) and an f64 sum of 1500 terms in another order (2^-53 each, nothing here).  Bound: 2^-22 of the sum of the magnitudes.
    In the mixed scene this is what shows that an instance of scale 2^30 does not cost the tame instances next to it their contribution"""
    live = ~np.isnan(pts["point"]).any(axis=1)
    total, mag = np.zeros(len(pts)), np.abs(got.astype(np.float64))
    for k in range(len(inst)):
        one = build(pkg, sc_ctx, blases, inst[k:k + 1], 3, one=True)
        one.winding_prepare()
        w = one.winding_number(pts, beta=np.inf).astype(np.float64)
        one.close()
        total += w; mag += np.abs(w)
    fin = live & np.isfinite(total) & np.isfinite(got)
    assert fin.sum() >= 0.99 * live.sum()
    err = np.abs(got.astype(np.float64) - total)[fin]
    near = near_tame(pkg, pts)[fin]
    print(f"wind   {what:32s} beta inf: |scene - sum of the one-instance scenes| max {err.max():.3e} (near the tame instances {err[near].max():.3e}), "
          f"bound 2^-22 x {mag[fin].max():.3g}")
    bad = err > 2.0 ** -22 * mag[fin]
    assert not bad.any(), f"{what}: the scene's answer is not the sum of its instances' on {bad.sum()} queries (largest excess {float((err - 2.0 ** -22 * mag[fin]).max()):.3e})"


@pytest.mark.parametrize("name", WIND_RUNGS)
def test_winding_ladder(world, name):
    """the instance records (C, smax, the instance moment) and the top-level records byte for byte against scene_moments_host at every rung — where the f32
    products overflow the restatement holds the same infinities and NaNs — and the answers at beta = 2 and +inf"""
    pkg, sc_ctx, blases, _ = world
    inst, pts = wind_scene(pkg, name)
    trees = blas_trees(pkg, blases, meshes(pkg))
    for tl in TLAS:
        what = f"{name} top-level builder {tl}"
        scene = build(pkg, sc_ctx, blases, inst, tl)
        scene.winding_prepare()
        top = download_top(pkg, sc_ctx, scene)
        with np.errstate(all="ignore"):
            host = scene_moments_host(pkg, trees, inst, top)
        check_arrays(pkg, scene, blases, trees, host, what)
        for beta in BETAS:
            got = scene.winding_number(pts, beta=beta)
            winding_checks(pkg, name, trees, inst, top, host, pts, got, beta, what, name in WIND_EXACT)
        if name == "mixed":
            winding_is_additive(pkg, sc_ctx, blases, inst, pts, got, what)
        scene.close()


@pytest.mark.parametrize("name", ["uni_2p-64", "uni_2p64", "ratio_2p16", "far_2p23", "mixed"])
def test_winding_update_between_extremes(world, name):
    """built on the rung, updated to tame matrices and back: before the re-prepare the query is refused (stale moments) and writes nothing; after it the maps,
    instance moments and top-level moments are the restatement's on the step's matrices and the refit top-level tree, byte for byte, the maps and instance
    moments are those of a freshly built scene (the top-level sums follow the tree, whose topology an update keeps and a fresh build chooses), and the answers
    meet the bound"""
    pkg, sc_ctx, blases, _ = world
    L = pkg.lib()
    trees = blas_trees(pkg, blases, meshes(pkg))
    scene = build(pkg, sc_ctx, blases, wind_scene(pkg, name)[0], 3)
    scene.winding_prepare()
    for step, s in (("built on the rung", name), ("updated to tame", TAME), ("updated back", name)):
        inst, pts = wind_scene(pkg, s)
        what = f"{name}, {step}"
        if step != "built on the rung":
            scene.update(inst)
            sent = np.full(len(pts) * 4, 0x5A, dtype=np.uint8)
            d_pts, d_w = sc_ctx.upload(pts), sc_ctx.upload(sent)
            assert L.bvh_scene_winding_number(scene.handle, d_pts.ptr, len(pts), 2.0, d_w.ptr) == E_INVALID, f"{what}: stale moments were not refused"
            sc_ctx.synchronize()
            assert d_w.download(np.uint8, len(sent)).tobytes() == sent.tobytes(), f"{what}: the refused call wrote"
            d_pts.free(); d_w.free()
            scene._winding_ready = False
            scene.winding_prepare()
        top = download_top(pkg, sc_ctx, scene)
        with np.errstate(all="ignore"):
            host = scene_moments_host(pkg, trees, inst, top)
        check_arrays(pkg, scene, blases, trees, host, what)
        fresh = build(pkg, sc_ctx, blases, inst, 3)
        fresh.winding_prepare()
        for a, b in zip(scene.winding_instances(), fresh.winding_instances()):
            assert a.tobytes() == b.tobytes(), f"{what}: the instance records differ from a fresh build's"
        fresh.close()
        for beta in BETAS:
            winding_checks(pkg, s, trees, inst, top, host, pts, scene.winding_number(pts, beta=beta), beta, what, s == TAME or s in WIND_EXACT)
    scene.close()


# ---- the stackless passes under non-rigid instances ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", DEEP_RUNGS)
def test_deep_passes_under_non_rigid_instances(pkg, name):
    """the caterpillar BLAS (H = 70) under five instances of a rung (that some queries overflow the 64-entry stack and others of the same wave do not is
    tests/test_scene_query_extremes.py::test_deep_premises and ::test_deep_triangle_and_winding_premises): bvh_scene_knn (k = 8), bvh_scene_radius_search,
    bvh_scene_intersect_all, bvh_scene_overlap, bvh_scene_closest_tris (unbounded), bvh_scene_radius_tris (one finite radius) and the winding number at
    beta = +inf (test_gpu_scene_winding.check_walk's bound as it stands) get their answers from the stackless passes with s2 != 1, a non-rigid W and a non-zero e.  The unconditional guarantees on every query, byte-equal to the brute
    force on the well-conditioned ones, count == fill (a marked query's count is its fill: the search helpers compare the offsets of both calls) and no mark
    left.  The stackless kernels are launched on every call and return at once while nothing overflowed, so their names in a profile would say only that
    they were launched: that they did the work rests on the CPU file's stack needs"""
    tris, left, root, n, inst, pts, rays, boxes, _ = deep_scene(pkg, name)
    c, sc_ctx = pkg.Context(0), pkg.Context(0)
    try:
        d_nodes, d_tris = c.upload(left), c.upload(tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
        what = f"deep {name}"
        bf = deep_reference(pkg, name, "knn")
        hits, counts = scene.knn(pts, 8)
        knn_uncapped(pkg, pts, [tris], inst, bf, hits, counts, what)
        no_mark(what, hits, counts)
        ref = deep_reference(pkg, name, "radius")
        off, rhits = radius_all_ways_uncapped(pkg, scene, pts, [tris], inst, ref, what)
        no_mark(what, off, rhits)
        yref = deep_reference(pkg, name, "rays")
        yoff, yhits = all_hits(pkg, scene, rays, HITS_SORTED)
        check_scene_all_hits(pkg, rays, [tris], inst, yref, yoff, yhits, True, what + " rays sorted")
        uoff, uhits = all_hits(pkg, scene, rays, 0)
        assert uoff.tobytes() == yoff.tobytes(), f"{what}: sorted and unsorted ray calls count differently"
        check_scene_all_hits(pkg, rays, [tris], inst, yref, uoff, uhits, False, what + " rays unsorted")
        no_mark(what, yoff, yhits, uhits)
        oref = deep_reference(pkg, name, "overlap")
        ooff, orecs = overlap_all_ways(pkg, scene, boxes, oref, what + " boxes")
        no_mark(what, ooff, orecs)
        q, _, radius = deep_tri_scene(pkg, name)
        dm = DeviceMesh(pkg, sc_ctx, q, 1)
        cbf = deep_tri_reference(pkg, name, "closest_tris")
        tc = closest_tris_raw(pkg, scene, dm.inp, len(q), SCENE_TRIS_QUERY, 0, np.inf, pkg.QUERY_CLOSEST)
        ta = closest_tris_raw(pkg, scene, dm.inp, len(q), SCENE_TRIS_QUERY, 0, np.inf, pkg.QUERY_ANY)
        closest_tris_uncapped(pkg, q, [tris], inst, np.inf, cbf, tc, ta, what + " closest_tris")
        no_mark(what, tc, ta)
        tbf = deep_tri_reference(pkg, name, "radius_tris")
        toff, thits = radius_tris_uncapped(pkg, scene, q, [tris], inst, radius, tbf, what + " radius_tris", dm.inp, SCENE_TRIS_QUERY, 0)
        no_mark(what, toff, thits)
        dm.free()
        scene.winding_prepare()
        trees = [(left, None, 0, root, tris)]
        top = download_top(pkg, sc_ctx, scene)
        with np.errstate(all="ignore"):
            host = scene_moments_host(pkg, trees, inst, top)
        assert scene.winding_moments(0).tobytes() == host["blas"][0].tobytes() and scene.winding_moments(None).tobytes() == host["top"].tobytes()
        wpts, wdist, wdiag, wbf = deep_wind_scene(pkg, name)
        wgot = scene.winding_number(wpts, beta=np.inf)
        no_mark(what, wgot)
        check_walk(pkg, what + " winding", trees, inst, top, host, wpts, wdist, wdiag, wbf, wgot, np.inf)
        print(f"deep   {name:14s} closest_tris well {cbf['well'].mean():.4f}, {int(cbf['hit'].sum())} hits; radius_tris well {tbf['well'].mean():.4f}, {len(thits)} records")
        print(f"deep   {name:14s} knn well {bf['well'].mean():.4f} ({int((rows_differ(hits, bf['hits']) & ~bf['well']).sum())} ill-conditioned lists differ); "
              f"radius well {ref['well'].mean():.4f}, {len(rhits)} records; rays well {yref['well'].mean():.4f}, {len(yhits)} records; boxes {len(orecs)} records")
        scene.close(); d_nodes.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()
