"""CPU: the inputs of tests/test_gpu_query_extremes.py — meshes with non-finite, huge, far-offset and denormal vertices, queries with infinite, huge, denormal,
-0 and zero components — and the checks that those inputs are worth running: the share of well-conditioned queries of every (mesh, family) pair that the GPU file
compares bit for bit, and the coverage each family is there for (ties, all-inf distances, the replaced triangle as an answer).  The brute forces are the existing
ones, unchanged (test_query, test_multihit, test_point_query, test_knn, test_radius, test_overlap, test_scene).  Run with -s for the table of shares."""
import numpy as np
import pytest

from test_gpu_point_query import make_points
from test_gpu_query import make_rays
from test_gpu_round5 import _special
from test_knn import knn_brute_force, truncate
from test_multihit import all_hits_brute_force
from test_overlap import AABB, as_boxes, make_boxes, overlap_brute_force
from test_point_query import F32, point_brute_force
from test_query import brute_force
from test_radius import radius_brute_force
from test_scene import make_instances, mat34, scene_brute_force, xf_points

FLT_MAX = np.finfo(F32).max
N_SPECIAL, N_FRAME = 4000, 1000
BULK, AIMED, SIDE = 256, 64, 64                    # queries per family: make_rays / make_points, aimed at the replaced triangle, one query-side special
KS = (1, 8, 32)

# the tree-side specials of test_gpu_round5 (one triangle of uniform(4000, 77) replaced), four frames of uniform(1000, 77), round 5's x + 3e38
SPECIAL_MESHES = ["inf_vertex", "neg_inf_vertex", "huge_triangle", "nan_coordinate", "nan_vertex", "neg_nan_coordinate", "ff_filled_triangle"]
FRAMES = ["offset_2p20", "scale_2p40", "scale_2p60", "denormals"]
MESH_NAMES = ["base"] + SPECIAL_MESHES + FRAMES + ["huge_offset"]
RAY_MESHES = MESH_NAMES                                       # every ray family is compared bit for bit
POINT_MESHES = [m for m in MESH_NAMES if m != "huge_offset"]    # (huge_offset carries the rays off its plane only)
POINT_EXACT = [m for m in POINT_MESHES if m != "denormals"]     # denormals: every dist2 underflows; only the unconditional guarantees are asserted
RAY_SIDE = ["tmax_inf", "tmin_neginf", "origin_inf", "dir_inf", "dir_denormal", "dir_negzero", "origin_3e38", "dir_2p100", "dir_2m100", "dir_zero"]
POINT_SIDE = ["coord_inf", "coord_3e38", "radius_1e30", "radius_1e-41", "radius_negzero"]

_MESHES, _RAYS, _POINTS, _RAY_REF, _POINT_REF = {}, {}, {}, {}, {}


def mesh(pkg, name):
    if name not in _MESHES:
        if name == "base":
            t = pkg.meshgen.uniform(N_SPECIAL, 77)
        elif name in SPECIAL_MESHES or name == "huge_offset":
            t = _special(pkg, name)
        else:
            t = pkg.meshgen.uniform(N_FRAME, 77)
            for v in ("v1", "v2", "v3"):
                if name == "offset_2p20":
                    t[v] = t[v] + F32(2.0 ** 20)
                elif name == "denormals":
                    t[v] = (t[v] * F32(1e-41)).astype(F32)            # (as round 5)
                else:
                    t[v] = t[v] * F32(2.0 ** {"scale_2p40": 40, "scale_2p60": 60}[name])
        _MESHES[name] = t
    return _MESHES[name]


def replaced(pkg, name):
    """the index of the one triangle in which a special mesh differs from the base mesh"""
    a, b = mesh(pkg, name), mesh(pkg, "base")
    diff = np.nonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))[0]
    assert len(diff) == 1
    return int(diff[0])


def centroid(pkg, name):
    t = mesh(pkg, "base")[replaced(pkg, name)]
    return (t["v1"].astype(np.float64) + t["v2"] + t["v3"]) / 3.0


def unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def plain_rays(pkg, tris, m, rng):
    """origins inside and around the mesh's box towards random points of it, unit directions, [0, 3e38)"""
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    o = lo - 0.25 * (hi - lo) + rng.random((m, 3)) * 1.5 * (hi - lo)
    r = np.zeros(m, dtype=pkg.RAY)
    r["origin"] = o; r["direction"] = unit(lo + rng.random((m, 3)) * (hi - lo) - o)
    r["tmax"] = F32(3.0e38)
    return r


def side_rays(pkg, tris, seed):
    """SIDE rays per query-side special; the component cycles over the axes, the sign alternates"""
    rng = np.random.default_rng(seed)
    i = np.arange(SIDE); c = i % 3; sign = np.where((i // 3) % 2 == 0, 1.0, -1.0).astype(F32)
    out = {}
    for fam in RAY_SIDE:
        r = plain_rays(pkg, tris, SIDE, rng)
        if fam == "tmax_inf":
            r["tmax"] = np.inf
        elif fam == "tmin_neginf":
            r["tmin"] = -np.inf; r["tmax"] = np.inf
        elif fam == "origin_inf":
            r["origin"][i, c] = sign * F32(np.inf)
        elif fam == "dir_inf":
            r["direction"][i, c] = sign * F32(np.inf)
        elif fam == "dir_denormal":
            r["direction"][i, c] = sign * F32(1e-41)
        elif fam == "dir_negzero":
            r["direction"][i, c] = F32(-0.0)
        elif fam == "origin_3e38":                                   # far out on one axis, pointing back at the mesh
            o = r["origin"].astype(np.float64); target = o + r["direction"].astype(np.float64)
            o[i, c] = sign * 3.0e38
            r["origin"] = o; r["direction"] = unit(target - o); r["tmax"] = np.inf
        elif fam == "dir_2p100":
            r["direction"] *= F32(2.0 ** 100); r["tmax"] = np.inf
        elif fam == "dir_2m100":
            r["direction"] *= F32(2.0 ** -100); r["tmax"] = np.inf
        elif fam == "dir_zero":
            r["direction"] = 0.0
        out[fam] = r
    return out


def side_points(pkg, tris, seed):
    rng = np.random.default_rng(seed)
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]])
    lo, hi = v.astype(np.float64).min(axis=0), v.astype(np.float64).max(axis=0)
    i = np.arange(SIDE); c = i % 3; sign = np.where((i // 3) % 2 == 0, 1.0, -1.0).astype(F32)
    out = {}
    for fam in POINT_SIDE:
        p = np.zeros(SIDE, dtype=pkg.POINT_QUERY)
        p["point"] = lo - 0.25 * (hi - lo) + rng.random((SIDE, 3)) * 1.5 * (hi - lo)
        if fam == "coord_inf":
            p["point"][i, c] = sign * F32(np.inf); p["radius"] = np.inf
        elif fam == "coord_3e38":
            p["point"][i, c] = sign * F32(3.0e38); p["radius"] = np.inf
        elif fam == "radius_1e30":
            p["radius"] = 1e30                                       # r2 overflows to +inf
        else:                                                        # r2 == 0: only dist2 == 0 is accepted, so half of the points sit on vertices
            p["point"][::2] = v[rng.integers(0, len(v), size=SIDE // 2)]
            p["radius"] = F32(1e-41) if fam == "radius_1e-41" else F32(-0.0)
        out[fam] = p
    return out


def aimed_rays(pkg, name, seed):
    """from centroid + N(0, 0.5) towards centroid + N(0, 0.01) of the replaced triangle as the base mesh has it"""
    rng = np.random.default_rng(seed)
    c = centroid(pkg, name)
    o = c + rng.normal(0, 0.5, (AIMED, 3))
    r = np.zeros(AIMED, dtype=pkg.RAY)
    r["origin"] = o; r["direction"] = unit(c + rng.normal(0, 0.01, (AIMED, 3)) - o); r["tmax"] = F32(3.0e38)
    return r


def aimed_points(pkg, name, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros(AIMED, dtype=pkg.POINT_QUERY)
    p["point"] = centroid(pkg, name) + rng.normal(0, 0.02, (AIMED, 3))
    p["radius"] = np.where(np.arange(AIMED) % 2 == 0, np.inf, 0.1)
    return p


def plane_rays(pkg, tris, seed):
    """huge_offset: every x is 3e38 after rounding.  Origins 0 to 8 ulps off that plane on either side, aimed at points of triangles (d.x = the exact offset back
    to the plane: t = 1); the rays that start on the plane run along +-x with tmin = -1, so that their hit at t = 0 is inside the window"""
    rng = np.random.default_rng(seed)
    x = tris["v1"][0, 0]
    assert (np.concatenate([tris["v1"][:, 0], tris["v2"][:, 0], tris["v3"][:, 0]]) == x).all()
    ulp = np.float64(np.spacing(x))
    i = np.arange(AIMED); j = i % 9; side = np.where((i // 9) % 2 == 0, 1.0, -1.0)
    w = rng.dirichlet((1.0, 1.0, 1.0), size=AIMED)
    t = tris[rng.integers(0, len(tris), size=AIMED)]
    target = t["v1"].astype(np.float64) * w[:, :1] + t["v2"].astype(np.float64) * w[:, 1:2] + t["v3"].astype(np.float64) * w[:, 2:]
    o = target + rng.normal(0, 0.3, (AIMED, 3)) * (j > 0)[:, None]           # (a ray that starts on the plane starts on its triangle)
    o[:, 0] = np.float64(x) + side * j * ulp
    d = target - o
    d[:, 0] = np.where(j == 0, side, -side * j * ulp)
    r = np.zeros(AIMED, dtype=pkg.RAY)
    r["origin"] = o; r["direction"] = d; r["tmax"] = F32(3.0e38)
    r["tmin"][j == 0] = -1.0
    assert (r["direction"][:, 0] != 0).all() and (r["origin"][:, 0].astype(np.float64) == o[:, 0]).all()
    return r


def families(parts):
    """one array and the slice of every family in it"""
    out, at = {}, 0
    for fam, a in parts.items():
        out[fam] = slice(at, at + len(a)); at += len(a)
    return np.concatenate(list(parts.values())), out


def rays_of(pkg, name):
    """(rays, {family: slice}) of a mesh"""
    if name not in _RAYS:
        seed = 1000 + MESH_NAMES.index(name)
        if name == "base":
            parts = side_rays(pkg, mesh(pkg, name), seed)
        elif name in SPECIAL_MESHES:                                 # (the extent of the special mesh itself is NaN or infinite: the bulk is the base mesh's)
            parts = {"bulk": make_rays(pkg, mesh(pkg, "base"), BULK, seed), "aimed": aimed_rays(pkg, name, seed)}
        elif name == "huge_offset":
            parts = {"plane": plane_rays(pkg, mesh(pkg, name), seed)}
        else:
            parts = {"frame": make_rays(pkg, mesh(pkg, name), BULK, seed)}
        _RAYS[name] = families(parts)
    return _RAYS[name]


def points_of(pkg, name):
    if name not in _POINTS:
        seed = 2000 + MESH_NAMES.index(name)
        if name == "base":
            parts = side_points(pkg, mesh(pkg, name), seed)
        elif name in SPECIAL_MESHES:
            parts = {"bulk": make_points(pkg, mesh(pkg, "base"), BULK, seed), "aimed": aimed_points(pkg, name, seed)}
        else:
            parts = {"frame": make_points(pkg, mesh(pkg, name), BULK, seed)}
        _POINTS[name] = families(parts)
    return _POINTS[name]


def ray_reference(pkg, name):
    """(rays, families, closest / any brute force, all-hits brute force), computed once"""
    if name not in _RAY_REF:
        rays, fam = rays_of(pkg, name)
        tris = mesh(pkg, name)
        _RAY_REF[name] = (rays, fam, brute_force(rays, tris), all_hits_brute_force(rays, tris))
    return _RAY_REF[name]


def point_reference(pkg, name):
    """(points, families, closest-point brute force, {k: kNN brute force}, radius brute force), computed once"""
    if name not in _POINT_REF:
        pts, fam = points_of(pkg, name)
        tris = mesh(pkg, name)
        big = knn_brute_force(pkg, pts, tris, 32)
        knn = {32: big, 8: truncate(pkg, big, 8), 1: truncate(pkg, big, 1)}
        _POINT_REF[name] = (pts, fam, point_brute_force(pkg, pts, tris), knn, radius_brute_force(pkg, pts, tris))
    return _POINT_REF[name]


def extreme_boxes(leaf_boxes, seed, skip=None):
    """BULK + 116 boxes of test_overlap.make_boxes over the leaf boxes (without leaf ``skip``, whose box a special mesh makes infinite, huge or empty), then: all of
    space {-inf .. +inf}; {-FLT_MAX .. FLT_MAX}; the scene with its +x plane at +inf; a point box at (FLT_MAX, y, z); a box flat at x = +inf; and per axis two
    boxes that lie flat in the planes +FLT_MAX and -FLT_MAX across the first leaf that has a coordinate there (across the scene when there is none)"""
    lb = as_boxes(leaf_boxes)
    usable = lb if skip is None else np.delete(lb, skip)
    with np.errstate(over="ignore"):
        boxes, _ = make_boxes(usable, seed, m=BULK)
    lo, hi = usable["min"].min(axis=0), usable["max"].max(axis=0)
    mid = (lo.astype(np.float64) + hi) / 2
    inf = np.inf
    with np.errstate(invalid="ignore"):
        far = np.nonzero((lb["max"][:, 0] >= FLT_MAX) & (lb["min"] <= lb["max"]).all(axis=1))[0]      # a leaf that reaches x = FLT_MAX: the point box lies in it
    if len(far):
        mid = (lb["min"][far[0]].astype(np.float64) + lb["max"][far[0]]) / 2
    extra = [(-inf, -inf, -inf, inf, inf, inf), (-FLT_MAX,) * 3 + (FLT_MAX,) * 3, (lo[0], lo[1], lo[2], inf, hi[1], hi[2]),
             (FLT_MAX, mid[1], mid[2], FLT_MAX, mid[1], mid[2]), (inf, lo[1], lo[2], inf, hi[1], hi[2])]
    at = np.nonzero((np.abs(lb["min"]) == FLT_MAX).any(axis=1) | (np.abs(lb["max"]) == FLT_MAX).any(axis=1))[0]
    across = (lb["min"][at[0]], lb["max"][at[0]]) if len(at) else (lo, hi)
    for ax in range(3):
        for plane in (FLT_MAX, -FLT_MAX):
            b = np.concatenate([np.minimum(across[0], across[1]), np.maximum(across[0], across[1])]).astype(F32)
            b[ax] = b[3 + ax] = plane
            extra.append(tuple(b))
    return np.concatenate([boxes, as_boxes(np.array(extra, dtype=F32))])


def stage_e_boxes(tris):
    """stage E's box of every triangle, restated: fminf / fmaxf drop a NaN coordinate, the minimum stays at or below FLT_MAX and the maximum at or above -FLT_MAX
    (an all-NaN axis keeps the reset box's planes)"""
    lo = np.fmin(F32(FLT_MAX), np.fmin(np.fmin(tris["v1"], tris["v2"]), tris["v3"]))
    hi = np.fmax(F32(-FLT_MAX), np.fmax(np.fmax(tris["v1"], tris["v2"]), tris["v3"]))
    return as_boxes(np.concatenate([lo, hi], axis=1))


SCENE_BLASES = ["nan_vertex", "inf_vertex", "huge_triangle", "base"]
SCENE_FAR = 12                                              # the instance whose translation is 2^20


def scene_instances(pkg):
    """13 instances of the four BLASes in turn: axis permutations with sign flips and scales 1, 1/2 or 1/4 per axis, translations on a grid of spacing 4 — every
    entry a power of two or 0, so the inverse is exact and no product with a plane at FLT_MAX overflows.  The last one lies 2^20 away."""
    rng = np.random.default_rng(4242)
    mats = []
    for k in range(SCENE_FAR + 1):
        A = np.zeros((3, 3)); A[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3) * 2.0 ** -rng.integers(0, 3, 3)
        t = np.array([k % 3, (k // 3) % 3, k // 9], dtype=np.float64) * 4.0 + 0.25
        if k == SCENE_FAR:
            t[0] += 2.0 ** 20
        mats.append(mat34(A, t))
    return make_instances(pkg, mats, np.arange(SCENE_FAR + 1) % len(SCENE_BLASES))


def scene_rays(pkg, inst):
    """per instance 20 rays around the base mesh as that instance places it and 4 aimed at the world position of the triangle its BLAS replaces (triangle 0 of
    the base mesh's own instances)"""
    rng = np.random.default_rng(4243)
    base = mesh(pkg, "base")
    parts = []
    for k in range(len(inst)):
        m = inst["object_to_world"][k]
        w = np.zeros(len(base), dtype=pkg.meshgen.TRIANGLE)
        for f in ("v1", "v2", "v3"):
            w[f] = xf_points(m, base[f])
        parts.append(plain_rays(pkg, w, 20, rng))
        name = SCENE_BLASES[inst["blas"][k]]
        t = w[replaced(pkg, name) if name != "base" else 0]
        c = (t["v1"].astype(np.float64) + t["v2"] + t["v3"]) / 3.0
        o = c + rng.normal(0, 0.5, (4, 3))
        r = np.zeros(4, dtype=pkg.RAY)
        r["origin"] = o; r["direction"] = unit(c + rng.normal(0, 0.01, (4, 3)) - o); r["tmax"] = F32(3.0e38)
        parts.append(r)
    return np.concatenate(parts)


def share(mask, sl):
    return float(mask[sl].mean())


# ---- the meshes -----------------------------------------------------------------------------------------------------------------------------------------------

def test_meshes_are_what_their_names_say(pkg):
    base = mesh(pkg, "base")
    assert len(base) == N_SPECIAL and np.isfinite(np.concatenate([base["v1"], base["v2"], base["v3"]])).all()
    for name in SPECIAL_MESHES:
        t = mesh(pkg, name)[replaced(pkg, name)]
        v = np.concatenate([t["v1"], t["v2"], t["v3"]])
        assert not np.isfinite(v).all() or np.abs(v).max() >= F32(3e38), name
    v = {name: np.concatenate([mesh(pkg, name)[f] for f in ("v1", "v2", "v3")]).astype(np.float64) for name in FRAMES + ["huge_offset"]}
    tiny = np.finfo(F32).tiny
    assert v["offset_2p20"].min() >= 2.0 ** 20 - 1 and v["offset_2p20"].max() <= 2.0 ** 20 + 2
    for name, e in (("scale_2p40", 40), ("scale_2p60", 60)):                     # everything stays normal
        nz = np.abs(v[name][v[name] != 0])
        assert nz.min() >= tiny and nz.max() <= 2.0 ** (e + 1)
    assert np.abs(v["denormals"]).max() < tiny and (v["denormals"] != 0).any()
    assert len(np.unique(mesh(pkg, "huge_offset")["v1"][:, 0])) == 1             # extent 0 in x after rounding


# ---- well-conditioned shares: the existing suite's cap on every pair the GPU file compares bit for bit ---------------------------------------------------------

@pytest.mark.parametrize("name", RAY_MESHES)
def test_ray_families_are_well_conditioned(pkg, name):
    rays, fam, bf, ref = ray_reference(pkg, name)
    assert (ref["n_acc"] == bf["n_acc"]).all() and (ref["well"] == bf["well"]).all()
    for f, sl in fam.items():
        print(f"rays   {name:20s} {f:14s} well {share(bf['well'], sl):.3f}  hit {share(bf['hit'], sl):.3f}  tie {share(bf['tie'], sl):.3f}  "
              f"mean hits {ref['n_acc'][sl].mean():.2f}")
        assert share(bf["well"], sl) >= 0.99, (name, f)


@pytest.mark.parametrize("name", POINT_MESHES)
def test_point_families_are_well_conditioned(pkg, name):
    pts, fam, bf, knn, rad = point_reference(pkg, name)
    for f, sl in fam.items():
        print(f"points {name:20s} {f:14s} well: closest {share(bf['well'], sl):.3f} k=8 {share(knn[8]['well'], sl):.3f} k=32 {share(knn[32]['well'], sl):.3f} "
              f"radius {share(rad['well'], sl):.3f}  tie: closest {share(bf['tie'], sl):.3f} k-th (8) {share(knn[8]['kth_tie'], sl):.3f} "
              f"k-th (32) {share(knn[32]['kth_tie'], sl):.3f} radius {share(rad['tie'], sl):.3f}  records {int(rad['counts'][sl].sum())}")
        if name in POINT_EXACT:
            for what, well in (("closest", bf["well"]), ("k=1", knn[1]["well"]), ("k=8", knn[8]["well"]), ("k=32", knn[32]["well"]), ("radius", rad["well"])):
                assert share(well, sl) >= 0.99, (name, f, what)
    if name == "denormals":                                          # the products of denormal edges underflow: dist2 falls below the boxes' f64 distance
        assert 0.3 <= bf["well"].mean() <= 0.8
    # the three families agree with each other: k = 1 is the closest point, the sorted radius slice starts with the kNN list
    assert knn[1]["hits"]["dist2"][:, 0].tobytes() == bf["closest"]["dist2"].tobytes() and knn[1]["hits"]["prim"][:, 0].tobytes() == bf["closest"]["prim"].tobytes()
    take = np.minimum(rad["counts"], 8)
    assert (take == knn[8]["counts"]).all()
    head = np.arange(8)[None] < take[:, None]
    idx = (rad["offsets"][:-1].astype(np.int64)[:, None] + np.arange(8)[None])[head]
    assert rad["hits"][idx].tobytes() == knn[8]["hits"][head].tobytes()


# ---- coverage: the inputs cannot silently stop testing anything ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SPECIAL_MESHES)
def test_aimed_queries_meet_the_replaced_triangle_on_the_base_mesh_only(pkg, name):
    rep = replaced(pkg, name)
    rays, rfam, rbf, rall = ray_reference(pkg, name)
    pts, pfam, pbf, knn, rad = point_reference(pkg, name)
    base_rays = brute_force(rays[rfam["aimed"]], mesh(pkg, "base"))
    base_pts = point_brute_force(pkg, pts[pfam["aimed"]], mesh(pkg, "base"))
    n_rays = int((base_rays["closest"]["prim"] == rep).sum()); n_pts = int((base_pts["closest"]["prim"] == rep).sum())
    print(f"{name}: the replaced triangle {rep} is the base mesh's answer of {n_rays} aimed rays and {n_pts} aimed points")
    assert n_rays >= 1 and n_pts >= 1
    assert not (rbf["closest"]["prim"] == rep).any() and not (pbf["closest"]["prim"] == rep).any()
    print(f"{name}: on the special mesh it is in {int((rall['hits']['prim'] == rep).sum())} all-hits slices, {int((knn[32]['hits']['prim'] == rep).sum())} kNN lists "
          f"and {int((rad['hits']['prim'] == rep).sum())} radius slices")


def test_the_far_frame_ties(pkg):
    """at 2^20 the ulp is 1/8 and the mesh is of unit size: answers tie on dist2 and on t, which the near-origin meshes of the other files never do"""
    rays, _, bf, _ = ray_reference(pkg, "offset_2p20")
    pts, _, pbf, knn, rad = point_reference(pkg, "offset_2p20")
    print(f"offset_2p20: ties on {pbf['tie'].mean():.3f} of the closest-point queries, k-th tie (k = 8) {knn[8]['kth_tie'].mean():.3f}, ray ties {int(bf['tie'].sum())} "
          f"of {len(rays)}")
    assert pbf["tie"].mean() >= 0.25 and bf["tie"].sum() >= 1
    assert knn[8]["kth_tie"].sum() >= 1 and rad["tie"].sum() >= 1


@pytest.mark.parametrize("fam", ["coord_inf", "coord_3e38", "radius_1e30"])
def test_infinite_distances_tie_and_an_infinite_r2_accepts_them(pkg, fam):
    pts, pfam, bf, knn, rad = point_reference(pkg, "base")
    sl = pfam[fam]
    assert (rad["counts"][sl] == N_SPECIAL).all()                   # the radius slices hold all n triangles
    if fam == "radius_1e30":
        return
    assert bf["tie"][sl].all() and (bf["closest"]["dist2"][sl] == np.inf).all() and (bf["closest"]["prim"][sl] == 0).all()
    assert (knn[32]["hits"]["prim"][sl] == np.arange(32)[None]).all() and knn[32]["kth_tie"][sl].all()      # decided purely by prim_idx


@pytest.mark.parametrize("fam", ["radius_1e-41", "radius_negzero"])
def test_a_zero_r2_accepts_exactly_dist2_zero(pkg, fam):
    pts, pfam, bf, knn, rad = point_reference(pkg, "base")
    sl = pfam[fam]
    assert (pts["radius"][sl].astype(F32) * pts["radius"][sl].astype(F32) == 0).all()
    assert bf["hit"][sl][::2].all() and not bf["hit"][sl][1::2].any() and (bf["closest"]["dist2"][sl][::2] == 0).all()


def test_ray_side_specials_keep_what_they_must(pkg):
    rays, fam, bf, ref = ray_reference(pkg, "base")
    hits = {f: int(bf["hit"][sl].sum()) for f, sl in fam.items()}
    print("hits per ray-side special:", hits)
    for f in ("tmax_inf", "tmin_neginf", "dir_denormal", "dir_negzero", "dir_2p100", "dir_2m100"):
        assert hits[f] >= 1, f
    assert hits["dir_zero"] == 0
    sl = fam["tmin_neginf"]
    assert (ref["hits"]["t"][ref["offsets"][sl.start]:ref["offsets"][sl.stop]] < 0).any()      # the window reaches behind the origin
    d = rays["direction"]
    assert (np.signbit(d[fam["dir_negzero"]]) & (d[fam["dir_negzero"]] == 0)).any(axis=1).all()
    assert (np.abs(d[fam["dir_denormal"]]) == F32(1e-41)).any(axis=1).all() and np.isinf(d[fam["dir_inf"]]).any(axis=1).all()
    assert np.isinf(rays["origin"][fam["origin_inf"]]).any(axis=1).all() and (np.abs(rays["origin"][fam["origin_3e38"]]) == F32(3e38)).any(axis=1).all()


def test_plane_rays_hit_from_every_offset(pkg):
    rays, fam, bf, _ = ray_reference(pkg, "huge_offset")
    x = mesh(pkg, "huge_offset")["v1"][0, 0]
    off = np.rint((rays["origin"][:, 0].astype(np.float64) - np.float64(x)) / np.float64(np.spacing(x))).astype(int)
    assert set(off.tolist()) == set(range(-8, 9))
    print("huge_offset: hits per offset in ulps", {k: int(bf["hit"][off == k].sum()) for k in range(-8, 9)})
    assert all(bf["hit"][off == k].any() for k in range(-8, 9))


# ---- the overlap boxes ---------------------------------------------------------------------------------------------------------------------------------------------

def test_extreme_boxes_against_clamped_infinite_and_empty_leaves(pkg):
    """the generator on leaf boxes as stage E makes them of the special triangles: an infinite plane, a huge box, the reset box of an all-NaN triangle"""
    t = mesh(pkg, "base")
    lo = np.minimum(np.minimum(t["v1"], t["v2"]), t["v3"]); hi = np.maximum(np.maximum(t["v1"], t["v2"]), t["v3"])
    leaf = as_boxes(np.concatenate([lo, hi], axis=1)).copy()
    leaf["max"][10, 0] = np.inf                                     # inf_vertex
    leaf["min"][11] = -3e38; leaf["max"][11] = 3e38                 # huge_triangle
    leaf["min"][12] = FLT_MAX; leaf["max"][12] = -FLT_MAX            # ff_filled_triangle: the reset box, the empty set
    boxes = extreme_boxes(leaf, 5, skip=[10, 11, 12])
    m = len(boxes) - 11
    assert boxes.dtype == AABB and m == BULK + 116
    sets = overlap_brute_force(boxes, leaf)
    valid = np.delete(np.arange(N_SPECIAL), 12)
    assert sets[m].tolist() == valid.tolist()                        # all of space: every leaf but the empty one
    assert sets[m + 1].tolist() == valid.tolist() and sets[m + 2].tolist() == valid.tolist()
    assert sets[m + 3].tolist() == [10] and sets[m + 4].tolist() == [10]      # only the infinite box reaches x = FLT_MAX and x = +inf
    assert all(s.tolist() in ([], [10], [11], [10, 11]) for s in sets[m + 5:]) and not any(12 in s for s in sets)
    assert sets[m + 5].tolist() == [10]


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_scene_rays_are_well_conditioned_and_reach_the_far_instance(pkg):
    meshes = [mesh(pkg, name) for name in SCENE_BLASES]
    inst = scene_instances(pkg)
    rays = scene_rays(pkg, inst)
    roots = []
    for t in meshes:                                                # the root box is the union (fminf / fmaxf) of stage E's boxes
        b = stage_e_boxes(t)
        roots.append(np.concatenate([b["min"].min(axis=0), b["max"].max(axis=0)]).astype(F32))
    assert roots[0].tolist() == roots[3].tolist() and roots[1][3] == np.inf and np.abs(roots[2]).max() == F32(3e38)
    bf = scene_brute_force(pkg, rays, meshes, inst, roots)
    hit = bf["closest"]["instance"][bf["hit"]]
    print(f"scene: well {bf['well'].mean():.3f}, hit {bf['hit'].mean():.3f}, {int((hit == SCENE_FAR).sum())} closest hits on the instance at 2^20")
    assert bf["well"].mean() >= 0.99 and bf["hit"].mean() >= 0.5
    assert set(hit.tolist()) == set(range(SCENE_FAR + 1))            # every instance answers some ray


# ---- the formula at the extremes, restated by hand -------------------------------------------------------------------------------------------------------------------

def test_nan_and_infinite_candidates_by_hand(pkg):
    """the header's sentences on one triangle: a NaN vertex is never accepted, not even by an infinite radius; dist2 == +inf is accepted by an infinite r2 only"""
    tri = np.zeros(2, dtype=pkg.meshgen.TRIANGLE)
    tri["v1"] = (0, 0, 0); tri["v2"] = (1, 0.1, 0.2); tri["v3"] = (0.1, 1, 0.3)            # (no zero edge component: 0 * inf is NaN)
    tri["v2"][1, 1] = np.nan
    pts = np.zeros(4, dtype=pkg.POINT_QUERY)
    pts["point"] = [(0.2, 0.2, 1.0), (np.inf, 0.2, 0.0), (3e38, 0.2, 0.0), (3e38, 0.2, 0.0)]
    pts["radius"] = (np.inf, np.inf, 1e30, 3e38)
    rad = radius_brute_force(pkg, pts, tri)
    assert rad["counts"].tolist() == [1, 1, 1, 1] and (rad["hits"]["prim"] == 0).all()
    assert np.isfinite(rad["hits"]["dist2"][0]) and rad["hits"]["dist2"][1:].tolist() == [np.inf, np.inf, np.inf]
    pts["radius"][1:] = 1e19                                        # r2 = 1e38 is finite: dist2 = inf is above it
    assert radius_brute_force(pkg, pts, tri)["counts"].tolist() == [1, 0, 0, 0]
