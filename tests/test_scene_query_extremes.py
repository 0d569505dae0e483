"""CPU: the inputs of tests/test_gpu_scene_query_extremes.py — the instance ladder of tests/test_scene_extremes.py (uniform scales 2^+-10 to 2^+-64, singular-value
ratios up to 2^24, shears up to 2^10, rigid offsets up to 2^23, a mirrored shear, one scene whose s2 spans 2^120, the s2 edges 2^65, 2^-65 and 2^-75) under the
nine scene queries that came after it: bvh_scene_knn, bvh_scene_radius_search, bvh_scene_intersect_all, bvh_scene_overlap, bvh_scene_intersect_tris,
bvh_scene_collide, bvh_scene_closest_tris, bvh_scene_radius_tris and bvh_scene_winding_number.  The scene, the points and the rays are that file's; the radii of
the radius search, the query boxes, the query triangles and their radii are made here.  Each query's brute force, checker and definition of "well-conditioned"
are its own CPU file's, unchanged.  Checked without a device: per (query kind, rung) the share of well-conditioned queries, from the brute force alone, against
the literal EXACT that tells the GPU tests where the 99 % floor applies; per rung the share of queries whose f32 restatement of the winding number is finite,
against WIND_EXACT, with local rungs that bracket the scale at which it stops being a number; that the inputs are what they claim; what the cull rule of a list
or a radius does when its bound is +inf or s2 is 0; and that the deep scene's queries overflow the short stack and stay in it within one wave.  Run with -s for
the tables."""
import numpy as np
import pytest

from test_closest_tris import query_ok
from test_intersect_tris import as_triangles, xyz
from test_overlap import as_boxes
from test_point_query import point_ok
from test_scene_extremes import (MIN_OFFSET, ONE_INSTANCE, RAY_EXACT, RUNGS, S2_EDGES, meshes, point_reference, ray_reference, rung_instances, rung_seed,
                                 scene_bounds, surface_samples, tame_instances, ladder_points, unit, world_parts)
from test_scene_closest_tris import scene_pair_matrix, scene_tris_dist_brute_force
from test_scene_collide import scene_collide_full
from test_scene_intersect_tris import instance_queries, scene_tris_brute_force
from test_scene_knn import MAX_K, scene_knn_brute_force, scene_knn_truncate
from test_scene_multihit import scene_all_hits_brute_force
from test_scene_overlap import mapped_leaf_boxes, scene_overlap_brute_force, tri_leaf_boxes
from test_scene_point import active_instances, scene_culls, world_culls
from test_scene_radius import scene_radius_brute_force
from test_scene_winding import median_split_tlas, scene_moments_host, scene_walk_host, scene_winding_brute_force
from test_scene_extremes import family_matrix
from test_scene import make_instances
from test_scene_radius_tris import scene_radius_tris_brute_force

F32 = np.float32
F64 = np.float64
KS = (1, 8, 32)
N_BOXES = 512
KINDS = ["knn", "radius", "rays", "overlap", "intersect_tris", "collide", "closest_tris", "radius_tris"]
N_TRIS = 256
TRI_RADII = ("inf", "band", "zero")                                   # bvh_scene_closest_tris: unbounded, a band of BAND scene diagonals, touching or crossing only
BAND = 0.02
PAIRS_PER_QUERY = 20                                                  # bvh_scene_radius_tris: the one radius of a call accepts about this many pairs per live query
TAME = "tame"                                                         # (not a rung: the envelope of the other scene tests, for bvh_scene_update)
_REF = {}


def cached(key, make):
    """references are computed once per session and shared (never modified) by the tests that need them"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------------------------------

def scene_of(pkg, name, one=False):
    """(instances, points, rays) of a rung: test_scene_extremes' own references' (one: its first instance alone, with ladder_points of its own); "tame": six
    instances of the envelope of the other scene tests with 512 points and rays"""
    if name == TAME:
        inst = tame_instances(pkg, 6)
        return inst, ladder_points(pkg, meshes(pkg), inst, 512, 31), None
    if one:
        inst = rung_instances(pkg, name)[:1].copy()
        return inst, ladder_points(pkg, meshes(pkg), inst, 512, rung_seed(name) + 100), None
    inst, pts, _ = point_reference(pkg, name)
    return inst, pts, ray_reference(pkg, name)[1]


def seed_of(name, one):
    return (31 if name == TAME else rung_seed(name) + (100 if one else 0))


def ladder_offsets(pkg, blas_tris, inst, m, seed):
    """the near-surface offsets that ladder_points(pkg, blas_tris, inst, m, seed) gave its first m // 2 points, from the same draws in the same order, and the
    points they give (test_radius_points_are_what_they_claim compares them with ladder_points' own)"""
    rng = np.random.default_rng(seed)
    parts = world_parts(pkg, blas_tris, inst)
    h = m // 2
    on, cen, size, vertex = surface_samples(parts, h, rng)
    d = unit(rng.normal(size=(h, 3)))
    away = on - cen
    d[vertex] = unit(away[vertex] / size[vertex, None] + 0.3 * d[vertex])
    off = np.maximum(10.0 ** rng.uniform(-4.0, np.log10(3.0), h) * size, MIN_OFFSET)
    with np.errstate(over="ignore"):
        return off, (on + d * off[:, None]).astype(F32)


def radius_points(pkg, name, one=False):
    """the rung's points with every infinite radius replaced by a finite one: 2, 4 or 8 times the near-surface offset for the near-surface half, 1e-3 .. 1e-1 of
    the scene's diagonal for the uniform half.  The finite radii (half or twice the offset: empty slices among them) and the eight dead queries stay"""
    def make():
        inst, pts, _ = scene_of(pkg, name, one)
        m, h = len(pts), len(pts) // 2
        off, _ = ladder_offsets(pkg, meshes(pkg), inst, m, seed_of(name, one))
        lo, hi = scene_bounds(world_parts(pkg, meshes(pkg), inst))
        rng = np.random.default_rng([41, seed_of(name, one)])
        r = np.concatenate([off * rng.choice([2.0, 4.0, 8.0], h), 10.0 ** rng.uniform(-3.0, -1.0, m - h) * np.linalg.norm(hi - lo)])
        out = pts.copy()
        inf = np.isposinf(pts["radius"])
        with np.errstate(over="ignore"):
            out["radius"][inf] = r[inf].astype(F32)
        cap = far_speck_cap(pkg, inst, pts["point"])
        with np.errstate(invalid="ignore"):
            capped = out["radius"] > cap
        out["radius"][capped] = cap[capped].astype(F32)
        return out
    return cached(("radius points", name, one), make)


SPECK = 64.0


def far_speck_cap(pkg, inst, p):
    """per point, the largest radius that takes in no instance seen as a speck: 0.99 of the distance to the nearest world box whose largest |coordinate| is
    less than 1 / SPECK of that distance (+inf without one).  From that far every triangle of the instance has the same f32 dist2, whose rounding (2^-24 of it)
    exceeds what the definition grows the world box by (2^-17 of its largest |coordinate|): each such candidate is ill-conditioned by definition, whatever the
    walk does.  A nearest-triangle query never answers with such an instance while anything is nearer; a radius takes in all 300 of its triangles at once.
    Only the mixed scene has such instances (the 2^-30 speck and the tame ones, seen from the 2^30 giant's far side)"""
    from test_scene import tris_root_box, world_box
    p = np.asarray(p, dtype=F64)
    cap = np.full(len(p), np.inf)
    for k in range(len(inst)):
        wb = world_box(inst["object_to_world"][k], tris_root_box(meshes(pkg)[int(inst["blas"][k])])).astype(F64)
        with np.errstate(invalid="ignore"):
            d = np.sqrt((np.maximum(np.maximum(wb[:3] - p, p - wb[3:]), 0.0) ** 2).sum(axis=1))
            speck = d > SPECK * np.abs(wb).max()
        cap = np.where(speck, np.minimum(cap, 0.99 * d), cap)
    return cap


def query_boxes(pkg, name, one=False, m=N_BOXES):
    """m boxes centred on surface_samples of the rung's world triangles, half-extents log-uniform 1e-3 .. 0.3 of that instance's world size per axis; the last
    eight as test_scene_overlap.scene_query_boxes has them: two that share exactly one face with a mapped leaf box (touching: reported), a mapped leaf box, a
    point box, two inverted boxes, two with a NaN.  Returns (boxes, the indices of the two touching boxes)"""
    def make():
        inst = scene_of(pkg, name, one)[0]
        rng = np.random.default_rng([43, seed_of(name, one)])
        parts = world_parts(pkg, meshes(pkg), inst)
        on, _, size, _ = surface_samples(parts, m, rng)
        half = 10.0 ** rng.uniform(-3.0, np.log10(0.3), (m, 3)) * size[:, None]
        with np.errstate(over="ignore"):
            q = np.concatenate([on - half, on + half], axis=1).astype(F32)
        _, active = active_instances(inst, 2)
        wl = np.concatenate([mapped_leaf_boxes(inst["object_to_world"][k], tri_leaf_boxes(meshes(pkg)[int(inst["blas"][k])])) for k in np.nonzero(active)[0]])
        t = wl[rng.integers(0, len(wl), 4)]
        tail = np.concatenate([t["min"], t["max"]], axis=1).astype(F32)
        for row, ax in ((0, 0), (1, 2)):                              # max = the leaf box's min on one axis: they share exactly that face
            tail[row, 3 + ax] = t["min"][row, ax]
            with np.errstate(over="ignore"):
                tail[row, ax] = np.nextafter(F32(t["min"][row, ax] - F32(0.01) * F32(size[row])), F32(-np.inf))
        tail[3, 3:] = tail[3, :3]
        inv = q[[5, 6]].copy(); inv[:, [0, 3]] = inv[:, [3, 0]]
        flat = inv[:, 0] == inv[:, 3]                                 # (a half-extent below an ulp of the centre: make min.x the next float above max.x)
        inv[flat, 0] = np.nextafter(inv[flat, 3], F32(np.inf))
        nan = q[[7, 8]].copy(); nan[0, 1] = np.nan; nan[1, 5] = np.nan
        q[m - 8:] = np.concatenate([tail, inv, nan])
        return as_boxes(q), np.array([m - 8, m - 7])
    return cached(("boxes", name, one), make)


def tri_queries(pkg, name, one=False, m=N_TRIS):
    """m world-space query triangles (TRIANGLE records).  Two thirds: a vertex 1e-4 .. 1 world sizes off a point of a world triangle, the other two at edge
    lengths of 1e-2 .. 0.5 world sizes from it in random directions.  A third (every third): a world triangle itself, moved 1e-4 .. 1e-1 world sizes along its
    normal — parallel to its original and to nothing else.  The last eight have a NaN coordinate"""
    def make():
        inst = scene_of(pkg, name, one)[0]
        rng = np.random.default_rng([47, seed_of(name, one)])
        parts = world_parts(pkg, meshes(pkg), inst)
        on, _, size, _ = surface_samples(parts, m, rng)
        p0 = on + unit(rng.normal(size=(m, 3))) * (10.0 ** rng.uniform(-4.0, 0.0, m) * size)[:, None]
        q = np.stack([p0] + [p0 + unit(rng.normal(size=(m, 3))) * (10.0 ** rng.uniform(-2.0, np.log10(0.5), m) * size)[:, None] for _ in range(2)], axis=1)
        which = rng.integers(0, len(parts), m)
        for i in range(0, m, 3):
            _, V, s = parts[which[i]]
            t = rng.integers(0, len(V[0]))
            a, b, c = V[0][t], V[1][t], V[2][t]
            n = np.cross((b - a) / s, (c - a) / s)
            n = n / np.linalg.norm(n) if np.linalg.norm(n) > 0 else np.array([0.0, 0.0, 1.0])
            q[i] = np.stack([a, b, c]) + n * (10.0 ** rng.uniform(-4.0, -1.0) * s)
        with np.errstate(over="ignore"):
            q = q.astype(F32)
        for j, i in enumerate(range(m - 8, m)):
            q[i, j % 3, (j // 3) % 3] = np.nan
        q[q == 0] = 0.0
        return as_triangles(pkg, q)
    return cached(("tris", name, one), make)


def scene_diagonal(pkg, inst):
    lo, hi = scene_bounds(world_parts(pkg, meshes(pkg), inst))
    return float(np.linalg.norm(hi - lo))


def tri_pairs(pkg, name, rows_of=None, one=False):
    """(instances, the query triangles, their pair matrix): rows_of = None: tri_queries; rows_of = k: the rows of BVH_SCENE_TRIS_INSTANCE(k), as many as
    instance k's BLAS has leaves"""
    def make():
        inst = scene_of(pkg, name, one)[0]
        q = tri_queries(pkg, name, one) if rows_of is None else \
            as_triangles(pkg, instance_queries(meshes(pkg), inst, rows_of, len(meshes(pkg)[int(inst["blas"][rows_of])])))
        with np.errstate(all="ignore"):
            return inst, q, scene_pair_matrix(pkg, q, meshes(pkg), inst)
    return cached(("tri pairs", name, rows_of, one), make)


def tri_radius(pkg, name, label, rows_of=None, one=False):
    """the radius of a bvh_scene_closest_tris call (inf, BAND of the scene's diagonal, 0) or, for label "pairs", of a bvh_scene_radius_tris call: the square
    root (rounded down to f32) of the dist2 at which the pair matrix accepts PAIRS_PER_QUERY pairs per live query — chosen from the reference alone"""
    inst, q, ((d2, _), ks, _) = tri_pairs(pkg, name, rows_of, one)
    if label == "inf":
        return float(np.inf)
    if label == "zero":
        return 0.0
    if label == "band":
        return float(F32(BAND * scene_diagonal(pkg, inst)))
    live = query_ok(q, 1.0)
    d = d2[live][:, ks != rows_of] if rows_of is not None else d2[live]
    d = np.sort(d[np.isfinite(d)].astype(F64))
    want = min(PAIRS_PER_QUERY * int(live.sum()), len(d) - 1)
    r = F32(np.sqrt(d[want]))
    while F64(r) * F64(r) > d[want] and r > 0:
        r = np.nextafter(r, F32(0.0))
    return float(r)


def intersect_tris_reference(pkg, name, rows_of=None, one=False):
    """(instances, queries (m, 3, 3), brute force): exact on every query — the predicate is the header's f64 one, restated operation for operation"""
    def make():
        inst, q, _ = tri_pairs(pkg, name, rows_of, one)
        with np.errstate(all="ignore"):
            return inst, xyz(q), scene_tris_brute_force(xyz(q), meshes(pkg), inst, skip=rows_of)
    return cached(("intersect tris", name, rows_of, one), make)


def collide_reference(pkg, name):
    def make():
        inst = scene_of(pkg, name)[0]
        with np.errstate(all="ignore"):
            return inst, scene_collide_full(meshes(pkg), inst)
    return cached(("collide", name), make)


def closest_tris_reference(pkg, name, label, rows_of=None, one=False):
    """(instances, queries, radius, brute force) of bvh_scene_closest_tris at the radius ``label``"""
    def make():
        inst, q, pairs = tri_pairs(pkg, name, rows_of, one)
        radius = tri_radius(pkg, name, label, rows_of, one)
        with np.errstate(all="ignore"):
            return inst, q, radius, scene_tris_dist_brute_force(pkg, q, meshes(pkg), inst, radius, skip=rows_of, pairs=pairs)
    return cached(("closest tris", name, label, rows_of, one), make)


def radius_tris_reference(pkg, name, rows_of=None):
    def make():
        inst, q, pairs = tri_pairs(pkg, name, rows_of)
        radius = tri_radius(pkg, name, "pairs", rows_of)
        with np.errstate(all="ignore"):
            return inst, q, radius, scene_radius_tris_brute_force(pkg, q, meshes(pkg), inst, radius, skip=rows_of, pairs=pairs)
    return cached(("radius tris", name, rows_of), make)


def asking_instances(name):
    """BVH_SCENE_TRIS_INSTANCE: instance 0 asks in every rung; in mixed the 2^-30 speck (0) and the 2^30 giant (1) ask in turn"""
    return (0, 1) if name == "mixed" else (0,)


# ---- the references, one per (rung, query kind) -----------------------------------------------------------------------------------------------------------------

def knn_reference(pkg, name, k=MAX_K, one=False):
    """(instances, points, the brute force at k) — computed once at k = 32 and cut"""
    def make():
        inst, pts, _ = scene_of(pkg, name, one)
        with np.errstate(invalid="ignore", over="ignore"):            # (s2 = +inf: inf x 0 in the well-conditioned test)
            return inst, pts, scene_knn_brute_force(pkg, pts, meshes(pkg), inst, MAX_K)
    inst, pts, bf = cached(("knn", name, one), make)
    return inst, pts, (bf if k == MAX_K else scene_knn_truncate(pkg, bf, k))


def radius_reference(pkg, name, one=False):
    def make():
        inst = scene_of(pkg, name, one)[0]
        pts = radius_points(pkg, name, one)
        with np.errstate(invalid="ignore", over="ignore"):
            return inst, pts, scene_radius_brute_force(pkg, pts, meshes(pkg), inst)
    return cached(("radius", name, one), make)


def rays_reference(pkg, name):
    def make():
        inst, _, rays = scene_of(pkg, name)
        return inst, rays, scene_all_hits_brute_force(pkg, rays, meshes(pkg), inst)
    return cached(("rays", name), make)


def overlap_reference(pkg, name, one=False):
    """(instances, boxes, touching, brute force): bvh_scene_overlap is exact on every query, so there is no well-conditioned subset"""
    def make():
        inst = scene_of(pkg, name, one)[0]
        boxes, touching = query_boxes(pkg, name, one)
        return inst, boxes, touching, scene_overlap_brute_force(boxes, [tri_leaf_boxes(t) for t in meshes(pkg)], inst)
    return cached(("overlap", name, one), make)


def well_share(pkg, kind, name):
    if kind == "knn":
        return float(knn_reference(pkg, name)[2]["well"].mean())      # (at k = 32: a list cut at a smaller k is well-conditioned wherever the longer one is)
    if kind == "radius":
        return float(radius_reference(pkg, name)[2]["well"].mean())
    if kind == "rays":
        return float(rays_reference(pkg, name)[2]["well"].mean())
    if kind == "closest_tris":
        return min(float(closest_tris_reference(pkg, name, label)[3]["well"].mean()) for label in TRI_RADII)
    if kind == "radius_tris":
        return float(radius_tris_reference(pkg, name)[3]["well"].mean())
    return 1.0                                                        # overlap, intersect_tris, collide: exact on every query


# where the 99 % floor applies: the rungs on which at least 99 % of the queries are well-conditioned by the query's own definition, measured on the brute force
# alone (test_exact_is_what_the_brute_force_gives).  The GPU tests run the existing checkers there and their uncapped twins elsewhere.  The rays' list is
# test_scene_extremes.RAY_EXACT: every accepted hit of a ray must be well-conditioned, not only the closest, and the same two rungs fall short.
EXACT = {"knn": list(RUNGS), "radius": list(RUNGS), "rays": list(RAY_EXACT), "overlap": list(RUNGS), "intersect_tris": list(RUNGS), "collide": list(RUNGS),
         "closest_tris": list(RUNGS), "radius_tris": list(RUNGS)}
REQUIRED = ["uni_2p10", "uni_2p-10", "ratio_2p8", "shear_2p4", "far_2p16", "mirror_shear"]


def test_exact_is_what_the_brute_force_gives(pkg):
    print()
    print(f"{'rung':14s} " + " ".join(f"{k[:8]:>8s}" for k in KINDS))
    for name in RUNGS + S2_EDGES:
        shares = {kind: well_share(pkg, kind, name) for kind in KINDS}
        print(f"{name:14s} " + " ".join(f"{shares[k]:8.4f}" for k in KINDS))
        if name in RUNGS:
            for kind in KINDS:
                assert (shares[kind] >= 0.99) == (name in EXACT[kind]), f"{kind} {name}: share {shares[kind]:.4f} against the literal"
    for kind in KINDS:
        assert set(REQUIRED) <= set(EXACT[kind]), kind
    assert EXACT["knn"] == RUNGS and EXACT["radius"] == RUNGS and EXACT["rays"] == RAY_EXACT


@pytest.mark.parametrize("name", RUNGS + S2_EDGES)
def test_radius_points_are_what_they_claim(pkg, name):
    """ladder_offsets restates ladder_points' draws (the points it gives are ladder_points'); no radius is infinite any more; the dead queries are untouched;
    the slices are neither all empty nor all of the scene: some empty, most in the tens, the longest bounded"""
    inst, pts, _ = scene_of(pkg, name)
    h = len(pts) // 2
    _, restated = ladder_offsets(pkg, meshes(pkg), inst, len(pts), rung_seed(name))
    live = ~np.isnan(pts["point"][:h]).any(axis=1)
    assert restated[live].tobytes() == pts["point"][:h][live].tobytes()
    rp = radius_points(pkg, name)
    assert not np.isposinf(rp["radius"]).any() and rp["point"].tobytes() == pts["point"].tobytes()
    keep = ~np.isposinf(pts["radius"])
    capped = rp["radius"][keep].tobytes() != pts["radius"][keep].tobytes()
    assert (name == "mixed") == capped or name in S2_EDGES, "far_speck_cap binds in the mixed scene and nowhere else"
    with np.errstate(invalid="ignore"):
        assert not (rp["radius"][keep] > pts["radius"][keep]).any() and (~point_ok(rp)).sum() >= 6
    bf = radius_reference(pkg, name)[2]
    c = bf["counts"]
    print(f"radius {name:14s} records {c.sum():7d}  empty {np.count_nonzero(c == 0):4d}  median {int(np.median(c[c > 0])) if (c > 0).any() else 0:4d}  "
          f"longest {c.max():4d}  well {bf['well'].mean():.4f}")
    if name in RUNGS:
        assert (c == 0).sum() >= 20 and (c > 8).sum() >= len(pts) // 8 and c.max() <= 6 * 300
        assert np.median(c[c > 0]) <= 6 * 300 // 4


@pytest.mark.parametrize("name", RUNGS + S2_EDGES)
def test_knn_and_ray_premises(pkg, name):
    """partial lists and full lists at k = 32, rays with more than one hit: the list bound (+inf until the list is full) and the multi-hit order are exercised"""
    _, pts, bf = knn_reference(pkg, name)
    full, partial = (bf["counts"] == MAX_K).sum(), ((bf["counts"] > 0) & (bf["counts"] < MAX_K)).sum()
    _, rays, rbf = rays_reference(pkg, name)
    print(f"knn    {name:14s} full lists {full:4d}  partial {partial:4d}  well at k = 1 / 8 / 32: "
          + " / ".join(f"{scene_knn_truncate(pkg, bf, k)['well'].mean():.4f}" for k in (1, 8)) + f" / {bf['well'].mean():.4f}"
          + f"   rays: records {rbf['n_acc'].sum():6d}  several hits {np.count_nonzero(rbf['n_acc'] > 1):4d}  well {rbf['well'].mean():.4f}")
    if name in RUNGS:
        assert full >= len(pts) // 2 and partial >= 10
        assert (rbf["n_acc"] > 1).sum() >= len(rays) // 8 and (rbf["n_acc"] == 0).sum() >= 20


@pytest.mark.parametrize("name", RUNGS + S2_EDGES)
def test_box_premises(pkg, name):
    """every mapped leaf box is finite; the touching boxes and the leaf box report, the inverted and NaN boxes do not; empty and long slices both occur"""
    inst, boxes, touching, bf = overlap_reference(pkg, name)
    c = bf["counts"]
    print(f"boxes  {name:14s} records {c.sum():7d}  empty {np.count_nonzero(c == 0):4d}  longer than 64 {np.count_nonzero(c > 64):4d}  longest {c.max():4d}")
    for k in range(len(inst)):
        leaf = mapped_leaf_boxes(inst["object_to_world"][k], tri_leaf_boxes(meshes(pkg)[int(inst["blas"][k])]))
        assert np.isfinite(leaf["min"]).all() and np.isfinite(leaf["max"]).all(), f"{name}: instance {k} maps a leaf box to a value that is not finite"
    assert (c[touching] >= 1).all() and c[-6] >= 1 and (c[-4:] == 0).all()
    assert (c > 64).sum() >= 10 and c.max() <= 6 * 300 and set(bf["recs"]["instance"].tolist()) == set(range(len(inst)))


@pytest.mark.parametrize("name", RUNGS + S2_EDGES)
def test_triangle_premises(pkg, name):
    """what the triangle queries find, per rung: crossings, nearest answers at each radius (and how many of their dist2 are finite: where the quartic terms of
    the segment-segment formula overflow or underflow the formula answers NaN, which is never accepted, or 0), pairs per live query at the one radius of the
    radius call, and the collide rows"""
    inst, q, xbf = intersect_tris_reference(pkg, name)
    live = query_ok(as_triangles(pkg, q), 1.0)
    assert (~live).sum() == 8
    line = f"tris   {name:14s} crossings {xbf['counts'].sum():5d} in {np.count_nonzero(xbf['counts']):3d} slices;"
    for label in TRI_RADII:
        _, _, radius, bf = closest_tris_reference(pkg, name, label)
        d = bf["closest"]["dist2"][bf["hit"]]
        line += f"  {label} hits {bf['hit'].sum():3d} (finite {int(np.isfinite(d).sum()):3d}, zero {int((d == 0).sum()):3d}) well {bf['well'].mean():.4f};"
    _, _, radius, rbf = radius_tris_reference(pkg, name)
    line += f"  radius {radius:.3g}: {rbf['counts'].sum() / live.sum():.1f} pairs per live query, ill pairs {rbf['ill_pairs']}, well {rbf['well'].mean():.4f};"
    full = collide_reference(pkg, name)[1]
    line += f"  collide rows {int(full['row_first'][-1])}, records {len(full['recs'])}"
    print(line)
    if name in RUNGS:
        assert closest_tris_reference(pkg, name, "inf")[3]["hit"].sum() >= N_TRIS // 2 and 1.0 <= rbf["counts"].sum() / live.sum() <= 50.0
        assert int(full["row_first"][-1]) == 3 * 300 + 3 * 200
        assert len(full["recs"]) > 0 or name.startswith("far"), "no two instances cross"     # (the rigid offsets of the far rungs scatter the six bodies)


@pytest.mark.parametrize("name", ONE_INSTANCE)
def test_one_instance_premises(pkg, name):
    for kind, bf in (("knn", knn_reference(pkg, name, one=True)[2]), ("radius", radius_reference(pkg, name, one=True)[2])):
        print(f"one instance {name:12s} {kind:7s} well {bf['well'].mean():.4f}")
        assert bf["well"].mean() >= 0.99
    assert overlap_reference(pkg, name, one=True)[3]["counts"].sum() > 1000


def test_tame_premises(pkg):
    """the tame state of the update tests is held to the 99 % floor as well"""
    share = radius_reference(pkg, TAME)[2]["well"].mean()
    c = overlap_reference(pkg, TAME)[3]["counts"]
    print(f"tame: radius well {share:.4f}, box records {c.sum()}")
    assert share >= 0.99 and c.sum() > 1000


def test_what_a_list_or_radius_bound_does_at_the_edges():
    """the cull s2 x lb' x (1 - 2^-20) > bound with the bounds that only the list and radius queries have.  bound = +inf (a list that is not full; r2 of a
    radius of 2^64 and above): nothing is culled whatever s2 is — inf > inf is false, NaN > inf is false.  s2 = 0 (uni_2p-75): nothing is culled at any bound,
    so a full list is never cut short and the walk of an entered instance is exhaustive; only the top-level rule decides.  s2 = +inf (uni_2p65) with a finite
    bound: every box that does not hold p' is culled."""
    lo = np.array([[0.0, 0.0, 0.0]], dtype=F32); hi = np.array([[1.0, 1.0, 1.0]], dtype=F32)
    inside = np.array([[0.5, 0.5, 0.5]], dtype=F32); outside = np.array([[3.0, 0.5, 0.5]], dtype=F32); beyond = np.array([[np.inf, 0.5, 0.5]], dtype=F32)
    e = np.zeros(1, dtype=F32)
    inf = F32(np.inf)
    for s2 in (F32(0.0), F32(2.0 ** -128), F32(1.0), F32(3.0e38), inf):
        for p in (inside, outside, beyond):
            assert not scene_culls(lo, hi, p, e, s2, inf)[0]
    with np.errstate(over="ignore"):
        assert np.isposinf(F32(2.0 ** 64) * F32(2.0 ** 64)) and np.isfinite(F32(2.0 ** 63) * F32(2.0 ** 64))
    for bound in (F32(0.0), F32(1e-45), F32(1.0)):
        assert not scene_culls(lo, hi, outside, e, F32(0.0), bound)[0]
        assert scene_culls(lo, hi, outside, e, inf, bound)[0] and not scene_culls(lo, hi, inside, e, inf, bound)[0]
    wb = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0], dtype=F32)
    assert not world_culls(wb, outside, np.array([inf]))[0] and world_culls(wb, outside, np.array([F32(1.0)]))[0]


def decided_at_the_top(pkg, pts, inst, hits):
    """test_scene_extremes.decisive_under_zero_s2 for lists: under s2 = 0 nothing is culled inside an instance, so a query is decided by the restated rule iff
    the top-level rule keeps the world box of every listed entry's instance at that entry's own dist2 (the bound is never below a listed entry's dist2).  hits:
    [m, k] lists or, for a radius search, handled by the caller per record"""
    from test_scene import tris_root_box, world_box
    out = np.ones(len(pts), dtype=bool)
    valid = hits["prim"] != pkg.INVALID
    for k in range(len(inst)):
        wb = world_box(inst["object_to_world"][k], tris_root_box(meshes(pkg)[int(inst["blas"][k])]))
        qi, sj = np.nonzero(valid & (hits["instance"] == k))
        culled = world_culls(wb, pts["point"][qi], hits["dist2"][qi, sj])
        np.logical_and.at(out, qi, ~culled)
    return out


def test_zero_s2_lists_are_decided_at_the_top(pkg):
    inst, pts, bf = knn_reference(pkg, "uni_2p-75", 1)
    decided = decided_at_the_top(pkg, pts, inst, bf["hits"])
    print(f"uni_2p-75: the restated top-level rule decides {decided.sum()} of {len(pts)} k = 1 lists")
    assert decided.mean() >= 0.99


# ---- bvh_scene_winding_number: where the f32 restatement is a number ------------------------------------------------------------------------------------------------

WIND_LOCAL = ["uni_2p40", "uni_2p42", "uni_2p44", "uni_2p-40", "uni_2p-48", "uni_2p-50", "uni_2p-52"]        # rungs of this file alone: they bracket the scale at which the far-field term stops being a number
WIND_RUNGS = RUNGS + WIND_LOCAL
BETAS = (2.0, np.inf)


def wind_scene(pkg, name):
    """(instances, points) of a winding rung: the ladder's own, or six uniform instances of scale 2^K with ladder_points of their own for the local rungs"""
    if name in WIND_LOCAL:
        def make():
            K = int(name.split("_2p")[1])
            rng = np.random.default_rng([53, K + 100])
            inst = make_instances(pkg, [family_matrix(rng, "uni", K) for _ in range(6)], np.arange(6) % 2)
            return inst, ladder_points(pkg, meshes(pkg), inst, 1024, 7100 + K)
        return cached(("wind scene", name), make)
    return scene_of(pkg, name)[:2]


def wind_conditioning(pkg, name):
    """(distance of every point to the scene's surface in f64 — NaN for a dead point —, the scene's diagonal): test_scene_winding.scene_conditioning from the
    f64 world triangles, so that a scale at which the f32 dist2 overflows or underflows still has a distance"""
    def make():
        inst, pts = wind_scene(pkg, name)
        parts = world_parts(pkg, meshes(pkg), inst)
        p = pts["point"].astype(F64)
        best = np.full(len(p), np.inf)
        lo, hi = scene_bounds(parts)
        diag = float(np.linalg.norm(hi - lo))
        from test_point_query import closest_formula
        for _, V, _ in parts:
            # (the f32 formula's order in f64 on coordinates brought to the scene's size: distances come back in units of the diagonal)
            with np.errstate(all="ignore"):
                _, d2, _, _, _ = closest_formula((p / diag)[:, None, :], (V[0] / diag)[None], (V[1] / diag)[None], (V[2] / diag)[None])
            best = np.fmin(best, np.where(np.isnan(d2), np.inf, d2).min(axis=1))
        dist = np.sqrt(best) * diag
        dist[np.isnan(p).any(axis=1)] = np.nan
        return dist, diag
    return cached(("wind conditioning", name), make)


def wind_brute_force(pkg, name):
    return cached(("wind brute", name), lambda: scene_winding_brute_force(pkg, meshes(pkg), wind_scene(pkg, name)[0], wind_scene(pkg, name)[1]["point"]))


def wind_selection(pkg, name, w32):
    """the live queries farther than 1e-4 diagonals from the surface (check_walk's well-conditioned ones) whose f32 restatement is finite"""
    dist, diag = wind_conditioning(pkg, name)
    with np.errstate(invalid="ignore"):
        return (dist > 1e-4 * diag) & np.isfinite(w32)


def near_tame(pkg, pts):
    """mixed: the queries within two world sizes of one of the two tame instances (4 and 5) and farther than 1e-4 of that size from the scene's surface —
    check_walk's conditioning premise with the tame instance's size where it has the scene's diagonal (2^31 here: by that measure every point near the tame
    instances lies on the surface)"""
    parts = {k: (V, s) for k, V, s in world_parts(pkg, meshes(pkg), rung_instances(pkg, "mixed"))}
    p = pts["point"].astype(F64)
    out = np.zeros(len(p), dtype=bool)
    for k in (4, 5):
        V, s = parts[k]
        allv = np.concatenate(V)
        lo, hi = allv.min(axis=0), allv.max(axis=0)
        with np.errstate(invalid="ignore"):
            out |= (np.sqrt((np.maximum(np.maximum(lo - p, p - hi), 0.0) ** 2).sum(axis=1)) <= 2.0 * s) & (wind_conditioning(pkg, "mixed")[0] > 1e-4 * s)
    return out


def wind_host(pkg, orc, name):
    """the restatement on the CPU oracle's trees (builders 1 and 3) under a hand-made median-split top level: (trees, instances, top, moments)"""
    def make():
        inst, _ = wind_scene(pkg, name)
        trees = []
        for algo, tris in zip((1, 3), meshes(pkg)):
            t = orc.build_tree(algo, tris)
            trees.append((t["nodes"], t["leaves"], t["layout"], t["root"], tris))
        pre = scene_moments_host(pkg, trees, inst)
        top = median_split_tlas(pkg, pre["wbox"])
        return trees, inst, top, scene_moments_host(pkg, trees, inst, top)
    return cached(("wind host", name), make)


def wind_finite_share(pkg, orc, name):
    """{beta: the share of live queries whose f32 restatement is finite}"""
    def make():
        trees, inst, top, mom = wind_host(pkg, orc, name)
        pts = wind_scene(pkg, name)[1]
        live = ~np.isnan(pts["point"]).any(axis=1)
        return {beta: float(np.isfinite(scene_walk_host(pkg, trees, inst, top, mom, pts["point"], beta, F32))[live].mean()) for beta in BETAS}
    return cached(("wind share", name), make)


# the rungs on which at least 99 % of the live queries have a finite f32 restatement at both betas, measured here (test_wind_exact_is_what_the_restatement_gives)
WIND_EXACT = ["uni_2p10", "uni_2p-10", "uni_2p30", "uni_2p-30", "ratio_2p8", "ratio_2p16", "ratio_2p24", "shear_2p4", "shear_2p10", "far_2p16", "far_2p20",
              "far_2p23", "mirror_shear", "mixed"]


def test_wind_exact_is_what_the_restatement_gives(pkg, orc):
    print()
    print(f"{'rung':14s} finite at beta 2  finite at beta inf  finite instance records  finite top-level records")
    for name in WIND_RUNGS:
        share = wind_finite_share(pkg, orc, name)
        mom = wind_host(pkg, orc, name)[3]
        fin_i = int(np.isfinite(mom["inst"].view(F32).reshape(len(mom["inst"]), -1)).all(axis=1).sum())
        fin_t = int(np.isfinite(mom["top"].view(F32).reshape(len(mom["top"]), -1)).all(axis=1).sum())
        print(f"{name:14s} {share[2.0]:16.4f}  {share[np.inf]:18.4f}  {fin_i:10d} of {len(mom['inst'])}  {fin_t:10d} of {len(mom['top'])}")
        if name in RUNGS:
            assert (min(share.values()) >= 0.99) == (name in WIND_EXACT), f"{name}: shares {share} against the literal"
    assert {"uni_2p10", "uni_2p-10", "uni_2p30", "uni_2p-30", "ratio_2p8", "ratio_2p16", "ratio_2p24", "shear_2p4", "shear_2p10", "far_2p16", "far_2p20", "far_2p23",
            "mirror_shear", "mixed"} <= set(WIND_EXACT)


def wind_bounded_floor(name):
    """the share of live queries that the 1e-4-diagonal premise must leave under the bound.  ladder_points puts half the points 1e-4 .. 3 world sizes off the
    surface (log-uniform) and half anywhere in the scene's bounds.  Where the diagonal is a few world sizes the premise drops about a tenth of the first
    half; on the far rungs the diagonal is 2^K against a world size of 1.7, so all of the first half lies nearer than 1e-4 diagonals and the second half is
    what is bounded; in the mixed scene the same holds for the points placed on the small instances"""
    return 0.45 if name.startswith("far") else 0.5 if name == "mixed" else 0.85


@pytest.mark.parametrize("name", WIND_EXACT)
def test_wind_bounded_share(pkg, name):
    dist, diag = wind_conditioning(pkg, name)
    live = ~np.isnan(dist)
    with np.errstate(invalid="ignore"):
        share = float((dist > 1e-4 * diag)[live].mean())
    print(f"wind {name:14s} {share:.3f} of the live queries lie farther than 1e-4 diagonals from the surface (floor {wind_bounded_floor(name)})")
    assert share >= wind_bounded_floor(name)


def test_wind_mixed_has_queries_near_the_tame_instances(pkg):
    _, pts = wind_scene(pkg, "mixed")
    near = near_tame(pkg, pts)
    dist, diag = wind_conditioning(pkg, "mixed")
    print(f"mixed: {near.sum()} of {len(pts)} points lie within two world sizes of a tame instance; the scene's diagonal is {diag:.3g}")
    assert near.sum() >= 100


# ---- the stackless passes under non-rigid instances ---------------------------------------------------------------------------------------------------------------

from test_deep_trees import QUERY_STACK, chain_left                        # noqa: E402
from test_gpu_point_query import first_descent_pushes                      # noqa: E402
from test_gpu_query import caterpillar, tree_height_and_stack              # noqa: E402
from test_scene import instance_inverse                                    # noqa: E402
from test_scene_extremes import DEEP_H, DEEP_RUNGS, deep_queries           # noqa: E402
from test_scene_overlap import blas_pass, left_first_scene_need, mapped_box    # noqa: E402
from test_scene_radius import mixed_wave, scene_radius_needs               # noqa: E402


def deep_scene(pkg, name):
    """test_scene_extremes' deep scene — the caterpillar BLAS (H = 70, chained below the left links: the list and slice walks are left-first) under five
    instances of the rung — with its points and rays, and 256 boxes by i % 4: the whole of the instance it is aimed at (every chain node passes with its side
    node), a run of far side nodes, the near triangle alone, nothing — each the world box of an object-space box under the instance's matrix.
    -> (tris, nodes chained left, root, n, inst, pts, rays, boxes, the BLAS-level stack need of every box in the instance it is aimed at)"""
    def make():
        tris, nodes, root, n = caterpillar(pkg, DEEP_H, 3 + DEEP_H)
        left = chain_left(nodes, n - 1)
        inst, pts, rays = deep_queries(pkg, name)
        rng = np.random.default_rng([59, DEEP_RUNGS.index(name)])
        m = 256
        aimed = rng.integers(0, len(inst), m)
        q = np.zeros((m, 6), dtype=F32)
        for i in range(m):
            a, w = rng.uniform(0, 2 * DEEP_H - 1), rng.uniform(0, 40)
            o = np.array([(-20, -20, -100, 40, 40, 5000), (-1, -1, 1000 + a, 1, 1, 1000 + a + w), (-1, -1, 0, 1, 1, 0.25), (-1, -1, 0.625, 1, 1, 999)][i % 4], dtype=F32)
            lo, hi = mapped_box(inst["object_to_world"][aimed[i]][None], o[None, :3], o[None, 3:])
            q[i] = np.concatenate([lo[0], hi[0]])
        need = np.array([left_first_scene_need(left, root, n, blas_pass(left, inst["object_to_world"][aimed[i]], q[i]), False) for i in range(m)])
        return tris, left, root, n, inst, pts, rays, as_boxes(q), need
    return cached(("deep scene", name), make)


def deep_reference(pkg, name, kind):
    def make():
        tris, left, root, n, inst, pts, rays, boxes, _ = deep_scene(pkg, name)
        with np.errstate(all="ignore"):
            if kind == "knn":
                return scene_knn_brute_force(pkg, pts, [tris], inst, 8)
            if kind == "radius":
                return scene_radius_brute_force(pkg, pts, [tris], inst)
            if kind == "rays":
                return scene_all_hits_brute_force(pkg, rays, [tris], inst)
            return scene_overlap_brute_force(boxes, [tri_leaf_boxes(tris)], inst)
    return cached(("deep", name, kind), make)


@pytest.mark.parametrize("name", DEEP_RUNGS)
def test_deep_premises(pkg, name):
    """some queries overflow the 64-entry stack and some do not, in one wave: the unbounded points push one entry per chain node on their first descent
    (whichever instance they enter first), the radius walk's own need (test_scene_radius.scene_radius_needs) is above 64 for some and at most 64 for others
    of one wave, likewise the boxes'; an axis ray passes every chain node"""
    tris, left, root, n, inst, pts, rays, boxes, box_need = deep_scene(pkg, name)
    w, active = instance_inverse(inst["object_to_world"])
    assert active.all()
    W = w.astype(F64).reshape(-1, 3, 4)
    pushes = [min(first_descent_pushes(left, root, n - 1, W[k, :, :3] @ pts["point"][j].astype(F64) + W[k, :, 3]) for k in range(len(inst))) for j in range(0, len(pts) // 2, 8)]
    assert max(pushes) > QUERY_STACK, max(pushes)
    lower, upper = scene_radius_needs(left, root, n, inst, pts)
    assert (lower > QUERY_STACK).sum() >= 64 and (upper <= QUERY_STACK).sum() >= 64 and mixed_wave(lower, upper), "no wave mixes overflowing and quiet points"
    assert (box_need > QUERY_STACK).sum() >= 32 and mixed_wave(box_need, box_need + len(inst) - 1), "no wave mixes overflowing and quiet boxes"
    _, depth = tree_height_and_stack(left, root, n - 1, (0.0, 0.0, -1.0), (0.0, 0.0, 1.0))
    assert depth > QUERY_STACK, depth
    shares = {kind: float(deep_reference(pkg, name, kind)["well"].mean()) for kind in ("knn", "radius", "rays")}
    print(f"deep {name:14s} well: " + "  ".join(f"{k} {v:.4f}" for k, v in shares.items()) + f"   box records {deep_reference(pkg, name, 'overlap')['counts'].sum()}")


# ... the triangle queries and the winding number through the stackless passes

from test_scene_closest_tris import scene_tris_culls, world_tris_culls        # noqa: E402
from test_scene import world_box                                              # noqa: E402
from test_scene_point import flat_world_tris, scene_s2                        # noqa: E402
from test_scene_winding import scene_conditioning, scene_make_points          # noqa: E402
from test_winding import stack_depth_all_open                                 # noqa: E402

DEEP_TRI_REACH = 100.0                                                        # object units: the far triangles are 2 apart, so a query among them reaches about 100 side nodes' worth of z


def deep_tri_scene(pkg, name, m=256):
    """query triangles for the deep scene, by the kinds of test_gpu_scene_closest_tris.deep_queries in the object space of the instance each is aimed at (small
    triangles below the near face, between the two near faces, coplanar with the face, through both, and — the last quarter — among the far triangles), mapped
    to the world by that instance's matrix in f64 and rounded; the last four have a NaN coordinate.  The one radius of the radius call is DEEP_TRI_REACH
    object units of instance 0 (its smallest singular value times that)
    -> (query TRIANGLE records, the instance each is aimed at, the radius)"""
    def make():
        inst = deep_scene(pkg, name)[4]
        rng = np.random.default_rng([61, DEEP_RUNGS.index(name)])
        aimed = np.arange(m) % len(inst)
        c = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-3, -0.5, m)], axis=1)
        c[: m // 6, 2] = 0.25
        c[3 * m // 4:, 2] = rng.uniform(1000, 1000 + 2 * DEEP_H, m - 3 * m // 4)
        q = c[:, None, :] + rng.normal(0, 0.05, (m, 3, 3))
        q[m // 6: m // 3, :, 2] = 0.0
        q[m // 3: m // 2, 0, 2] = 0.75; q[m // 3: m // 2, 1:, 2] = -0.5
        M = inst["object_to_world"].astype(F64).reshape(-1, 3, 4)[aimed]
        w = (np.einsum("nij,nvj->nvi", M[:, :, :3], q) + M[:, None, :, 3]).astype(F32)
        for j, i in enumerate(range(m - 4, m)):
            w[i, j % 3, j % 3] = np.nan
        w[w == 0] = 0.0
        smin = np.linalg.svd(inst["object_to_world"].astype(F64).reshape(-1, 3, 4)[0, :, :3], compute_uv=False)[2]
        return as_triangles(pkg, w), aimed, float(F32(DEEP_TRI_REACH * smin))
    return cached(("deep tris", name), make)


def deep_tri_needs(pkg, name):
    """(lower, upper) bounds of the radius walk's short-stack need per query triangle (scene_radius_needs for triangles): inside an instance the left-first
    need on the walk's own box test at the fixed bound r2 (exact), the top level adds at most n_inst - 1"""
    tris, left, root, n, inst = deep_scene(pkg, name)[:5]
    q, _, radius = deep_tri_scene(pkg, name)
    x = xyz(q)
    live = query_ok(q, radius)
    w, _ = active_instances(inst, 1)
    s2 = scene_s2(w)
    r2 = F32(radius) * F32(radius)
    lower = np.zeros(len(x), dtype=np.int64)
    N = len(left)
    for k in range(len(inst)):
        wb = world_box(inst["object_to_world"][k], np.concatenate([left["min"][root], left["max"][root]]))
        entered = ~world_tris_culls(wb, x, np.full(len(x), r2)) & live
        for i in np.nonzero(entered)[0]:
            xi = np.broadcast_to(x[i], (N, 3, 3))
            passes = ~scene_tris_culls(left["min"], left["max"], w[k], xi, s2[k], np.full(N, r2))
            lower[i] = max(lower[i], left_first_scene_need(left, root, n, passes, False))
    return lower, lower + (len(inst) - 1)


def deep_tri_reference(pkg, name, kind):
    def make():
        tris, _, _, _, inst = deep_scene(pkg, name)[:5]
        q, _, radius = deep_tri_scene(pkg, name)
        with np.errstate(all="ignore"):
            pairs = cached(("deep tri pairs", name), lambda: scene_pair_matrix(pkg, q, [tris], inst))
            if kind == "closest_tris":
                return scene_tris_dist_brute_force(pkg, q, [tris], inst, np.inf, pairs=pairs)
            return scene_radius_tris_brute_force(pkg, q, [tris], inst, radius, pairs=pairs)
    return cached(("deep tri", name, kind), make)


def deep_wind_scene(pkg, name):
    """300 points of test_scene_winding.scene_make_points on the deep scene's world triangles -> (points, distance to the surface, diagonal, f64 brute force)"""
    def make():
        tris, _, _, _, inst = deep_scene(pkg, name)[:5]
        flat, _, _ = flat_world_tris(pkg, [tris], inst)
        pts = scene_make_points(pkg, flat, 300, 67)
        dist, diag = scene_conditioning(pkg, pts, flat)
        return pts, dist, diag, scene_winding_brute_force(pkg, [tris], inst, pts["point"])
    return cached(("deep wind", name), make)


@pytest.mark.parametrize("name", DEEP_RUNGS)
def test_deep_triangle_and_winding_premises(pkg, name):
    """closest_tris: an unbounded query below the near face passes every box until its first candidate, so its first descent in whichever instance it enters
    first pushes one entry per chain node, more than the stack holds; the dead queries of the same waves are not walked.  radius_tris: at the call's one
    radius the walk's own need is above 64 for some queries and at most 64 for others of one wave.  Winding at beta = +inf opens every node: every live query
    needs stack_depth_all_open entries, more than 64, beside the NaN points of the last wave"""
    tris, left, root, n, inst = deep_scene(pkg, name)[:5]
    q, aimed, radius = deep_tri_scene(pkg, name)
    m = len(q)
    w, _ = instance_inverse(inst["object_to_world"])
    W = w.astype(F64).reshape(-1, 3, 4)
    cen = xyz(q).astype(F64).mean(axis=1)
    pushes = [min(first_descent_pushes(left, root, n - 1, W[k, :, :3] @ cen[j] + W[k, :, 3]) for k in range(len(inst))) for j in range(m // 2, 3 * m // 4, 4)]
    assert max(pushes) > QUERY_STACK, max(pushes)
    lower, upper = deep_tri_needs(pkg, name)
    cbf, rbf = deep_tri_reference(pkg, name, "closest_tris"), deep_tri_reference(pkg, name, "radius_tris")
    print(f"deep {name:14s} triangles: radius {radius:.4g}, {int((lower > QUERY_STACK).sum())} overflow, {int((upper <= QUERY_STACK).sum())} stay, mixed waves {mixed_wave(lower, upper)}; "
          f"closest well {cbf['well'].mean():.4f}, radius records {len(rbf['hits'])} well {rbf['well'].mean():.4f} longest {rbf['counts'].max()}")
    assert (lower > QUERY_STACK).sum() >= 16 and (upper <= QUERY_STACK).sum() >= 64 and mixed_wave(lower, upper), "no wave mixes overflowing and quiet triangles"
    assert cbf["hit"].sum() >= m // 2 and len(rbf["hits"]) > 500
    assert stack_depth_all_open(left, root, n - 1) > QUERY_STACK
    pts, dist, diag, _ = deep_wind_scene(pkg, name)
    with np.errstate(invalid="ignore"):
        share = float((dist > 1e-4 * diag).mean())
    print(f"deep {name:14s} winding: {share:.4f} of the points lie farther than 1e-4 diagonals from the surface; all-open stack depth {stack_depth_all_open(left, root, n - 1)}")
    assert share >= 0.95 and np.isnan(pts["point"]).any(axis=1).sum() == 8
