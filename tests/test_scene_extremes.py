"""CPU: the inputs of tests/test_gpu_scene_extremes.py — a named ladder of instance sets that leaves the envelope of the other scene tests (uniform scales 2^+-10
to 2^+-64, singular-value ratios up to 2^24, shears up to 2^10, rigid offsets up to 2^23, a mirrored shear, one scene that mixes them), point and ray queries
aimed at the world triangles of such scenes, and a list of matrices on the edges of the activity rule — with the checks that those inputs are worth running: per
rung the share of hits and of well-conditioned queries of the existing brute forces (test_scene, test_scene_point; unchanged), the cull rule on the true leaf, and
what the restated rule does when s2 is a denormal, 0 or infinite.  Run with -s for the table of shares."""
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_query import caterpillar
from test_gpu_refit import no_negzero
from test_point_query import tri_arrays
from test_query_extremes import SCENE_BLASES, SCENE_FAR, mesh, stage_e_boxes
from test_query_extremes import scene_instances as non_finite_scene_instances
from test_scene import FLT_MAX, instance_inverse, make_instances, mat34, rot, scene_brute_force, tris_root_box, world_box, xf_points
from test_scene_point import active_instances, object_points, scene_culls, scene_point_brute_force, scene_s2, world_culls

F32 = np.float32
F64 = np.float64
M_QUERIES = 1024

UNI = ["uni_2p10", "uni_2p-10", "uni_2p30", "uni_2p-30", "uni_2p60", "uni_2p-60", "uni_2p-64", "uni_2p64"]      # the last two: s2 on the f32 edges
RATIO = ["ratio_2p8", "ratio_2p16", "ratio_2p24"]
SHEAR = ["shear_2p4", "shear_2p10"]
FAR = ["far_2p16", "far_2p20", "far_2p23"]
RUNGS = UNI + RATIO + SHEAR + FAR + ["mirror_shear", "mixed"]
S2_EDGES = ["uni_2p65", "uni_2p-65", "uni_2p-75"]           # s2 = +inf, a deep denormal, 0: the instances stay active; only the unconditional guarantees hold
ONE_INSTANCE = ["uni_2p-30", "ratio_2p16", "far_2p20"]                # rungs whose first instance also runs alone (n_inst == 1: no top-level tree)
DEEP_RUNGS = ["ratio_2p8", "shear_2p4", "mirror_shear", "far_2p16"]
TAME = "tame"

_MESHES, _INST, _POINT_REF, _RAY_REF, _ONE_REF, _NON_FINITE = [], {}, {}, {}, {}, []


def meshes(pkg):
    """the two BLAS meshes of every rung: 300 and 200 triangles in the unit cube"""
    if not _MESHES:
        _MESHES.extend([no_negzero(pkg.meshgen.uniform(300, 91)), no_negzero(pkg.meshgen.uniform(200, 92))])
    return _MESHES


def two_rotations(rng):
    return rot(rng.integers(3), rng.uniform(0, 2 * np.pi)) @ rot(rng.integers(3), rng.uniform(0, 2 * np.pi))


def placed(A, c):
    """x -> A (x + c): the translation A c is scaled along with the matrix"""
    return mat34(A, np.asarray(A, dtype=F64) @ np.asarray(c, dtype=F64))


def family_matrix(rng, family, K, c=None):
    """one matrix of a family (R1 . D . R2 unless rigid) placing the unit cube shifted by c (default: U(-1.2, 1.2)^3, so that neighbours overlap)"""
    R1, R2 = two_rotations(rng), two_rotations(rng)
    c = rng.uniform(-1.2, 1.2, 3) if c is None else c
    if family == "uni":
        return placed(2.0 ** K * R1, c)
    if family == "ratio":                                             # singular values 2^-K/2, 1, 2^K/2
        return placed(R1 @ np.diag([2.0 ** (-K / 2), 1.0, 2.0 ** (K / 2)]) @ R2, c)
    if family in ("shear", "mirror_shear"):                           # diag(0.25 .. 4) x a unit upper triangle with entries of magnitude 2^K (0.5 .. 1 of it)
        S = np.eye(3)
        S[0, 1], S[0, 2], S[1, 2] = rng.choice([-1.0, 1.0], 3) * rng.uniform(0.5, 1.0, 3) * 2.0 ** K
        D = np.diag(rng.uniform(0.25, 4.0, 3))
        if family == "mirror_shear":
            D = D @ np.diag([-1.0, 1.0, 1.0])
        return placed(R1 @ D @ S @ R2, c)
    if family == "far":                                               # rigid; |t| reaches 2^K on one axis at least
        t = rng.uniform(-1.0, 1.0, 3) * 2.0 ** K
        t[rng.integers(3)] = rng.choice([-1.0, 1.0]) * 2.0 ** K * rng.uniform(0.75, 1.0)
        return mat34(R1, t)
    if family == TAME:
        return placed(R1 @ np.diag(rng.uniform(0.5, 2.0, 3)) @ R2, c)
    raise KeyError(family)


def parse(name):
    """"uni_2p-30" -> ("uni", -30); "mirror_shear" -> ("mirror_shear", 2)"""
    if name == "mirror_shear":
        return name, 2
    if name == TAME:
        return name, 0
    family, k = name.split("_2p")
    return family, int(k)


def rung_instances(pkg, name, seed=0):
    """the instance set of a rung: 6 instances over the two meshes (mixed: the six kinds the issue names)"""
    key = (name, seed)
    if key not in _INST:
        rng = np.random.default_rng([seed, (RUNGS + S2_EDGES + [TAME]).index(name)])
        if name == "mixed":
            centre = -np.full(3, 0.5)
            mats = [family_matrix(rng, "uni", -30, centre + rng.uniform(-0.05, 0.05, 3)),                           # a speck at the origin, inside the tame meshes
                    family_matrix(rng, "uni", 30, centre + rng.uniform(-0.05, 0.05, 3)),                            # spans everything, the far one included
                    family_matrix(rng, "ratio", 16, centre + rng.uniform(-0.05, 0.05, 3)),
                    family_matrix(rng, "far", 20),
                    family_matrix(rng, TAME, 0, centre + rng.uniform(-0.3, 0.3, 3)), family_matrix(rng, TAME, 0, centre + rng.uniform(-0.3, 0.3, 3))]
        else:
            family, K = parse(name)
            mats = [family_matrix(rng, family, K) for _ in range(6)]
        _INST[key] = make_instances(pkg, mats, np.arange(len(mats)) % 2)
    return _INST[key]


def world_parts(pkg, blas_tris, inst):
    """per active instance: (k, world triangles (v1, v2, v3) in f64 from the f32 world vertices, world size = its box diagonal)"""
    _, active = active_instances(inst, len(blas_tris))
    out = []
    for k in np.nonzero(active)[0]:
        V = [xf_points(inst["object_to_world"][k], v).astype(F64) for v in tri_arrays(blas_tris[int(inst["blas"][k])])]
        allv = np.concatenate(V)
        out.append((int(k), V, float(np.linalg.norm(allv.max(axis=0) - allv.min(axis=0)))))
    return out


def unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def surface_samples(parts, m, rng):
    """m points on random world triangles of random instances: (point, triangle centroid, world size of the instance, is a vertex); every third is a vertex"""
    on, cen, size = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m)
    which = rng.integers(0, len(parts), m)
    vertex = np.arange(m) % 3 == 2
    for i, (_, V, s) in enumerate(parts):
        idx = np.nonzero(which == i)[0]
        t = rng.integers(0, len(V[0]), len(idx))
        b = rng.dirichlet((1.0, 1.0, 1.0), size=len(idx))
        b[vertex[idx]] = np.eye(3)[rng.integers(0, 3, int(vertex[idx].sum()))]
        on[idx] = V[0][t] * b[:, :1] + V[1][t] * b[:, 1:2] + V[2][t] * b[:, 2:]
        cen[idx] = (V[0][t] + V[1][t] + V[2][t]) / 3.0
        size[idx] = s
    return on, cen, size, vertex


def scene_bounds(parts):
    allv = np.concatenate([np.concatenate(V) for _, V, _ in parts])
    return allv.min(axis=0), allv.max(axis=0)


# a dist2 below 2^-136 is an f32 denormal with fewer than 13 significant bits: its rounding alone is more than the 2^-10 that s2 keeps in hand, so no rule can be
# exact about it.  The near-surface offsets therefore stay at or above 2^-68 (which only binds on uni_2p-64 and below, where it is 0.04 world sizes).
MIN_OFFSET = 2.0 ** -68


def ladder_points(pkg, blas_tris, inst, m, seed):
    """half near-surface: offsets 1e-4 .. 3 (log-uniform) times the instance's world size from points of its world triangles, along random directions (every
    third: from a vertex, away from its triangle — the vertex regions are what the formula still answers where its products overflow or underflow); half uniform
    in the scene bounds grown by a tenth.  A third have finite radii (half or twice the offset; a share of the scene's size), and the eight dead-query kinds of
    test_scene_point.scene_points are there"""
    rng = np.random.default_rng(seed)
    parts = world_parts(pkg, blas_tris, inst)
    h = m // 2
    on, cen, size, vertex = surface_samples(parts, h, rng)
    d = unit(rng.normal(size=(h, 3)))
    away = on - cen
    d[vertex] = unit(away[vertex] / size[vertex, None] + 0.3 * d[vertex])
    off = np.maximum(10.0 ** rng.uniform(-4.0, np.log10(3.0), h) * size, MIN_OFFSET)
    lo, hi = scene_bounds(parts)
    ext = hi - lo
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    with np.errstate(over="ignore"):
        pts["point"][:h] = (on + d * off[:, None]).astype(F32)
        pts["point"][h:] = (lo - 0.1 * ext + rng.random((m - h, 3)) * 1.2 * ext).astype(F32)
        pts["radius"] = np.inf
        fin = rng.random(m) < 1.0 / 3.0
        r = np.concatenate([off * np.where(rng.random(h) < 0.5, 0.5, 2.0), 10.0 ** rng.uniform(-3.0, 0.0, m - h) * np.linalg.norm(ext)])
        pts["radius"][fin] = r[fin].astype(F32)
    dead = rng.choice(m, 8, replace=False)
    pts["point"][dead[0], 0] = np.nan; pts["point"][dead[1], 2] = np.nan
    pts["radius"][dead[2]] = np.nan; pts["radius"][dead[3]] = -1.0; pts["radius"][dead[4]] = -np.inf; pts["radius"][dead[5]] = -0.5
    pts["radius"][dead[6]] = 0.0; pts["radius"][dead[7]] = -0.0
    return pts


def ladder_rays(pkg, blas_tris, inst, m, seed):
    """three quarters aimed: a target on a random triangle of a random instance, the origin 0.01 .. 3 mesh sizes off it along a random direction — both chosen in
    the instance's object space and mapped to the world in f64, so that the object-space ray is of the mesh's own size however the instance stretches it (a ray
    that is long in object units loses its hit point to the rounding of t: that is the formula's doing, not the walk's) — and the direction = (target - the
    rounded origin) x U(0.5, 2): t is near 1 at every scale.  A third of all rays have windows that end before or begin after the target.  One quarter start at
    points of the scene bounds in random directions of the scene's size.  Eight dead rays (NaN, tmax == tmin, tmax < tmin)."""
    rng = np.random.default_rng(seed)
    parts = world_parts(pkg, blas_tris, inst)
    a = 3 * m // 4
    ks = np.array([k for k, _, _ in parts])
    which = ks[rng.integers(0, len(ks), a)]
    M = inst["object_to_world"].astype(F64).reshape(-1, 3, 4)
    on, o = np.zeros((a, 3)), np.zeros((a, 3))
    for k in ks:
        idx = np.nonzero(which == k)[0]
        v = [x.astype(F64) for x in tri_arrays(blas_tris[int(inst["blas"][k])])]
        allv = np.concatenate(v)
        size = np.linalg.norm(allv.max(axis=0) - allv.min(axis=0))
        t = rng.integers(0, len(v[0]), len(idx))
        b = rng.dirichlet((1.0, 1.0, 1.0), size=len(idx))
        x = v[0][t] * b[:, :1] + v[1][t] * b[:, 1:2] + v[2][t] * b[:, 2:]
        xo = x + unit(rng.normal(size=(len(idx), 3))) * (10.0 ** rng.uniform(-2.0, np.log10(3.0), len(idx)) * size)[:, None]
        on[idx] = x @ M[k, :, :3].T + M[k, :, 3]; o[idx] = xo @ M[k, :, :3].T + M[k, :, 3]
    lo, hi = scene_bounds(parts)
    ext = hi - lo
    rays = np.zeros(m, dtype=pkg.RAY)
    with np.errstate(over="ignore"):
        rays["origin"][:a] = o.astype(F32)
        rays["direction"][:a] = ((on - rays["origin"][:a].astype(F64)) * rng.uniform(0.5, 2.0, a)[:, None]).astype(F32)
        rays["origin"][a:] = (lo - 0.1 * ext + rng.random((m - a, 3)) * 1.2 * ext).astype(F32)
        rays["direction"][a:] = (unit(rng.normal(size=(m - a, 3))) * np.linalg.norm(ext)).astype(F32)
    rays["tmin"] = 0.0; rays["tmax"] = F32(3.0e38)
    w = rng.random(m) < 1.0 / 3.0
    rays["tmax"][w] = rng.uniform(0.25, 4.0, m)[w]
    w2 = ~w & (rng.random(m) < 0.15)
    rays["tmin"][w2] = rng.uniform(0.25, 4.0, m)[w2]
    dead = rng.choice(m, 8, replace=False)
    rays["origin"][dead[0], 0] = np.nan; rays["origin"][dead[1], 2] = np.nan; rays["direction"][dead[2], 1] = np.nan; rays["direction"][dead[3], 0] = np.nan
    rays["tmin"][dead[4]] = np.nan; rays["tmax"][dead[5]] = np.nan
    rays["tmax"][dead[6]] = rays["tmin"][dead[6]]; rays["tmin"][dead[7]] = 5.0; rays["tmax"][dead[7]] = 4.0
    return rays


def rung_seed(name):
    return 7000 + (RUNGS + S2_EDGES + [TAME]).index(name)


def point_reference(pkg, name):
    """(instances, points, the two-level point brute force) of a rung, computed once; the BLAS root boxes are the triangles' (tests/test_gpu_scene_extremes.py
    checks that the built trees hold exactly those)"""
    if name not in _POINT_REF:
        inst = rung_instances(pkg, name)
        pts = ladder_points(pkg, meshes(pkg), inst, M_QUERIES, rung_seed(name))
        with np.errstate(invalid="ignore"):                          # (s2 = +inf: inf x 0 in the well-conditioned test)
            _POINT_REF[name] = (inst, pts, scene_point_brute_force(pkg, pts, meshes(pkg), inst))
    return _POINT_REF[name]


def one_instance_reference(pkg, name):
    """the first instance of a rung alone (n_inst == 1: no top-level tree), with 512 points and 512 rays of its own: (instances, points, point brute force,
    rays, ray brute force)"""
    if name not in _ONE_REF:
        inst = rung_instances(pkg, name)[:1].copy()
        pts = ladder_points(pkg, meshes(pkg), inst, M_QUERIES // 2, rung_seed(name) + 100)
        rays = ladder_rays(pkg, meshes(pkg), inst, M_QUERIES // 2, rung_seed(name) + 600)
        _ONE_REF[name] = (inst, pts, scene_point_brute_force(pkg, pts, meshes(pkg), inst), rays, scene_brute_force(pkg, rays, meshes(pkg), inst))
    return _ONE_REF[name]


def tame_instances(pkg, n):
    """n instances of the envelope the other scene tests stay in (rotation x diag(0.5 .. 2) x rotation, small translations), over the two meshes"""
    rng = np.random.default_rng([5, n])
    return make_instances(pkg, [family_matrix(rng, TAME, 0) for _ in range(n)], np.arange(n) % 2)


def ray_reference(pkg, name):
    if name not in _RAY_REF:
        inst = rung_instances(pkg, name)
        rays = ladder_rays(pkg, meshes(pkg), inst, M_QUERIES, rung_seed(name) + 500)
        _RAY_REF[name] = (inst, rays, scene_brute_force(pkg, rays, meshes(pkg), inst))
    return _RAY_REF[name]


def true_leaf_culled(pkg, pts, blas_tris, inst, bf):
    """test_scene_point.test_cull_rule_keeps_the_true_leaf's check for any number of BLASes: per hit, whether the rule culls the answer's leaf box, its BLAS's
    root box or its instance's world box at best = the answer's dist2"""
    c = bf["closest"]
    w, _ = active_instances(inst, len(blas_tris))
    s2 = scene_s2(w)
    culled = np.zeros(len(pts), dtype=bool)
    for k in np.unique(c["instance"][bf["hit"]]):
        tris = blas_tris[int(inst["blas"][k])]
        v1, v2, v3 = tri_arrays(tris)
        lo, hi = np.minimum(np.minimum(v1, v2), v3), np.maximum(np.maximum(v1, v2), v3)
        root = tris_root_box(tris)
        idx = np.nonzero(bf["hit"] & (c["instance"] == k))[0]
        j = c["prim"][idx]
        pp, e = object_points(w[k], pts["point"][idx])
        sk = np.full(len(idx), s2[k])
        culled[idx] = scene_culls(lo[j], hi[j], pp, e, sk, c["dist2"][idx]) | \
                      scene_culls(np.broadcast_to(root[:3], (len(idx), 3)), np.broadcast_to(root[3:], (len(idx), 3)), pp, e, sk, c["dist2"][idx]) | \
                      world_culls(world_box(inst["object_to_world"][k], root), pts["point"][idx], c["dist2"][idx])
    return culled


# ---- the activity edges -----------------------------------------------------------------------------------------------------------------------------------------

def cancelling_matrix():
    """a matrix whose determinant is -2^-60 exactly while the header's f64 evaluation of it is 0.  (A determinant cannot *underflow* in f64: a product of three
    non-zero f32 values is at least 2^-447.  What f64 can do is round a small one away: here c00 = 1 - 2^-60 rounds to 1 and cancels against c01 = -1.)"""
    return np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 2.0 ** -30], [0.0, 2.0 ** -30, 1.0]])


def exact_det(A):
    f = [[Fraction(float(x)) for x in row] for row in np.asarray(A, dtype=F32)]
    return f[0][0] * (f[1][1] * f[2][2] - f[1][2] * f[2][1]) + f[0][1] * (f[1][2] * f[2][0] - f[1][0] * f[2][2]) + f[0][2] * (f[1][0] * f[2][1] - f[1][1] * f[2][0])


def activity_edges():
    """[(label, object_to_world (12,) f32, active by the header's rule)]"""
    big = 2.0 ** 100
    out = [("singular: zero", mat34(np.zeros((3, 3))), False),                                                      # test_scene's hand cases
           ("singular: rank 2", mat34(np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1.0]])), False),
           ("NaN translation", mat34(np.eye(3), (np.nan, 0, 0)), False),
           ("infinite translation", mat34(np.eye(3), (np.inf, 0, 0)), False),
           ("diag(1e-39, 1, 1): inverse 1e39", mat34(np.diag([1e-39, 1.0, 1.0])), False),
           ("diag(1e-30 ..): det 1e-90", mat34(np.diag([1e-30, 1e-30, 1e-30])), True),
           ("-2^-130: inverse entry -inf, det finite", mat34(np.diag([-2.0 ** -130, 1.0, 1.0])), False),
           ("shear 2^100 over 2^-40: inverse entry -2^140", mat34(np.array([[1.0, big, 0], [0, 2.0 ** -40, 0], [0, 0, 1.0]])), False),
           ("translation entry of the inverse overflows", mat34(np.diag([2.0 ** -100, 1.0, 1.0]), (2.0 ** 100, 0, 0)), False),
           ("diag(2^127, 1, 1): inverse entry a denormal", mat34(np.diag([2.0 ** 127, 1.0, 1.0]), (1.0, 2.0, 3.0)), True),
           ("2^126 x rotation: every inverse entry a denormal", mat34(2.0 ** 126 * (rot(2, 0.3) @ rot(0, 1.1)), (2.0 ** 100, 0, -2.0 ** 90)), True),
           ("denormal entries 2^-140: inverse 2^140", mat34(np.diag([2.0 ** -140] * 3)), False)]
    for K in (65, -65, -75, 64, -64):
        out.append((f"uniform 2^{K}", mat34(2.0 ** K * (rot(1, 0.7) @ rot(2, 2.1)), np.array([0.25, -0.5, 0.125]) * 2.0 ** K), True))
    out.append(("det rounds to 0 in f64, -2^-60 exactly", mat34(cancelling_matrix(), (1.0, 2.0, 3.0)), False))
    return out


def edge_instances(pkg):
    """the activity edges as one instance set over the two meshes, with two tame instances in front (a scene needs something to hit)"""
    rng = np.random.default_rng(77)
    mats = [family_matrix(rng, TAME, 0), family_matrix(rng, TAME, 0)] + [m for _, m, _ in activity_edges()]
    return make_instances(pkg, mats, np.arange(len(mats)) % 2)


def test_activity_edges_are_what_their_labels_say():
    edges = activity_edges()
    assert exact_det(cancelling_matrix()) == -Fraction(1, 1 << 60)
    w, active = instance_inverse(np.array([m for _, m, _ in edges]))
    for (label, m, want), got in zip(edges, active):
        print(f"{label:55s} active {bool(got)}")
        assert bool(got) == want, label
    by = {label: (w[i], scene_s2(w[i:i + 1])[0]) for i, (label, _, _) in enumerate(edges)}
    tiny = np.finfo(F32).tiny
    wd = np.abs(by["2^126 x rotation: every inverse entry a denormal"][0][[0, 1, 2, 4, 5, 6, 8, 9, 10]])
    assert (wd < tiny).all() and (wd > 0).sum() >= 6
    assert 0 < abs(by["diag(2^127, 1, 1): inverse entry a denormal"][0][0]) < tiny
    # s2 on and past the f32 edges, the instance active all the while
    assert by["uniform 2^65"][1] == np.inf and by["uniform 2^-75"][1] == 0.0
    assert 0 < by["uniform 2^-65"][1] < tiny and 0 < by["uniform 2^-64"][1] < tiny                  # denormals: about 2^-130 and 2^-128
    assert by["uniform 2^-64"][1] == pytest.approx(2.0 ** -128, rel=2e-3)
    assert FLT_MAX / 1.01 < by["uniform 2^64"][1] < np.inf                                          # the last binade below the overflow
    print("s2:", {label: float(s) for label, (_, s) in by.items() if label.startswith("uniform")})


def test_edge_scene_has_every_edge_behind_two_tame_instances(pkg):
    inst = edge_instances(pkg)
    _, active = active_instances(inst, 2)
    assert list(active) == [True, True] + [a for _, _, a in activity_edges()]


def test_what_the_rule_does_with_an_infinite_and_a_zero_s2():
    """s2 = +inf: inf x 0 is NaN and never culls (a box that holds p'); inf x (a positive lb') culls once best is finite and never while best is +inf.  s2 = 0:
    0 x lb' is 0 (or NaN for an infinite lb') and never culls.  So under s2 = 0 the walk inside the instance is exhaustive, and under s2 = +inf it is cut short
    after the first finite candidate: only candidates whose boxes hold p' are still reached."""
    lo = np.array([[0.0, 0.0, 0.0]], dtype=F32); hi = np.array([[1.0, 1.0, 1.0]], dtype=F32)
    inside = np.array([[0.5, 0.5, 0.5]], dtype=F32); outside = np.array([[3.0, 0.5, 0.5]], dtype=F32)
    e = np.zeros(1, dtype=F32)
    inf, zero = F32(np.inf), F32(0.0)
    assert not scene_culls(lo, hi, inside, e, inf, F32(1.0))[0] and not scene_culls(lo, hi, inside, e, inf, F32(0.0))[0]
    assert scene_culls(lo, hi, outside, e, inf, F32(1e30))[0] and scene_culls(lo, hi, outside, e, inf, F32(FLT_MAX))[0]
    assert not scene_culls(lo, hi, outside, e, inf, inf)[0]
    for best in (zero, F32(1e-45), F32(1.0), inf):
        assert not scene_culls(lo, hi, outside, e, zero, best)[0] and not scene_culls(lo, hi, inside, e, zero, best)[0]
    assert not scene_culls(lo, hi, np.array([[np.inf, 0.5, 0.5]], dtype=F32), e, zero, F32(1.0))[0]
    # a denormal s2 is a number like any other: 2^-128 x 2^100 against 2^-30
    d = np.array([[2.0 ** 50 + 1.0, 0.5, 0.5]], dtype=F32)
    assert scene_culls(lo, hi, d, e, F32(2.0 ** -128), F32(2.0 ** -30))[0] and not scene_culls(lo, hi, d, e, F32(2.0 ** -128), F32(2.0 ** -27))[0]


# ---- the ladder ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_rungs_are_what_their_names_say(pkg):
    for name in RUNGS + S2_EDGES:
        inst = rung_instances(pkg, name)
        assert 4 <= len(inst) <= 8 and set(inst["blas"].tolist()) == {0, 1} and max(len(t) for t in meshes(pkg)) <= 300
        w, active = instance_inverse(inst["object_to_world"])
        assert active.all(), name
        A = inst["object_to_world"].astype(F64).reshape(-1, 3, 4)
        sv = np.linalg.svd(A[:, :, :3], compute_uv=False)
        family, K = parse(name) if name != "mixed" else ("mixed", 0)
        if family == "uni":
            assert np.allclose(sv, 2.0 ** K, rtol=1e-6), name
        elif family == "ratio":
            # (the entries are rounded to f32: an ulp of the largest, 2^(K/2 - 24), against the smallest singular value 2^-K/2 — all of it at K = 24)
            assert (sv[:, 0] / sv[:, 2] > 2.0 ** (K - 2)).all() and np.allclose(sv[:, 0], 2.0 ** (K / 2), rtol=1e-3) and np.allclose(sv[:, 1], 1.0, rtol=1e-2), name
        elif family == "shear":
            assert (sv[:, 0] / sv[:, 2] > 2.0 ** (2 * K - 6)).all(), name
        elif family == "far":
            assert np.allclose(sv, 1.0, rtol=1e-6) and (np.abs(A[:, :, 3]).max(axis=1) >= 0.75 * 2.0 ** K).all() and np.abs(A[:, :, 3]).max() <= 2.0 ** K, name
        elif family == "mirror_shear":
            assert (np.linalg.det(A[:, :, :3]) < 0).all()
    s2 = scene_s2(instance_inverse(rung_instances(pkg, "mixed")["object_to_world"])[0]).astype(F64)
    print(f"mixed: s2 from {s2.min():.3g} to {s2.max():.3g}, a factor of 2^{np.log2(s2.max() / s2.min()):.0f}")
    assert s2.max() / s2.min() > 2.0 ** 115                            # best passes between instances whose s2 differ by about 2^120


def overlapping_world_boxes(pkg, inst):
    boxes = np.array([world_box(inst["object_to_world"][k], tris_root_box(meshes(pkg)[int(inst["blas"][k])])) for k in range(len(inst))]).astype(F64)
    return [(i, j) for i in range(len(inst)) for j in range(i + 1, len(inst))
            if (boxes[i, :3] <= boxes[j, 3:]).all() and (boxes[j, :3] <= boxes[i, 3:]).all()]


def test_mixed_scene_overlaps(pkg):
    """the world boxes of the 2^30 instance and of every other one overlap, and so do the speck's and a tame one's: best is carried between them"""
    pairs = overlapping_world_boxes(pkg, rung_instances(pkg, "mixed"))
    assert {(0, 1), (1, 2), (1, 3), (1, 4), (1, 5)} <= set(pairs) and ({(0, 4), (0, 5)} & set(pairs)), pairs
    _, _, bf = point_reference(pkg, "mixed")
    answered = set(bf["closest"]["instance"][bf["hit"]].tolist())
    print("mixed: instances that answer some point", sorted(answered))
    assert answered == set(range(6))


@pytest.mark.parametrize("name", RUNGS)
def test_point_premises(pkg, name):
    """the caps on the reference alone: >= 99 % well-conditioned, at least a quarter of the queries hit, at least 20 miss, and the restated cull rule keeps the
    true leaf of every well-conditioned query"""
    inst, pts, bf = point_reference(pkg, name)
    culled = true_leaf_culled(pkg, pts, meshes(pkg), inst, bf)
    finite = np.isfinite(bf["closest"]["dist2"][bf["hit"]]).mean() if bf["hit"].any() else 0.0
    print(f"points {name:14s} hits {bf['hit'].sum():4d} of {len(pts)}  well {bf['well'].mean():.4f}  true leaf culled {np.count_nonzero(culled & bf['well'])} "
          f"(ill-conditioned: {np.count_nonzero(culled & ~bf['well'])})  finite dist2 on {finite:.3f} of the hits")
    assert bf["well"].mean() >= 0.99
    assert bf["hit"].sum() >= len(pts) // 4 and (~bf["hit"]).sum() >= 20
    assert not (culled & bf["well"]).any()


# rays: on these two rungs fewer than 99 % of the aimed rays are well-conditioned (measured: ratio_2p24 0.758, shear_2p10 0.379).  The object-space origin
# o' = W o is a sum of products of about 2^12 x 2^12 (2^10 x 2^10 x the mesh's offset) that cancels to the mesh's size: rounded to f32 it is off by about a mesh
# size, so the object-space ray that the formula is defined on meets the mesh somewhere else than the world ray meets the world box.  That is the defined
# formula's doing and no choice of rays avoids it, so on these rungs the GPU file asserts the unconditional guarantees (every record recomputes, nothing below the
# brute force) and exactness on whatever is well-conditioned, without the 99 % floor.  The point queries of the same rungs are exact (e absorbs that error).
RAY_UNCAPPED = ["ratio_2p24", "shear_2p10"]
RAY_EXACT = [r for r in RUNGS if r not in RAY_UNCAPPED]


@pytest.mark.parametrize("name", RUNGS)
def test_ray_premises(pkg, name):
    """>= 99 % well-conditioned on RAY_EXACT; on every rung at least a quarter of the rays hit and at least 20 miss.  With rays aimed in object space no rung is
    without hits (test_gpu_scene's make_rays, spread over the scene's bounds, finds none at uniform scales of 2^-20 and below or offsets of 2^12 and above), so
    no rung needs the all-miss exemption"""
    inst, rays, bf = ray_reference(pkg, name)
    print(f"rays   {name:14s} hits {bf['hit'].sum():4d} of {len(rays)}  well {bf['well'].mean():.4f}")
    if name in RAY_EXACT:
        assert bf["well"].mean() >= 0.99
    else:
        assert bf["well"].mean() < 0.99, f"{name} meets the cap: move it to RAY_EXACT"
    assert bf["hit"].sum() >= len(rays) // 4 and (~bf["hit"]).sum() >= 20


def decisive_under_zero_s2(pkg, pts, blas_tris, inst, bf):
    """the queries on which the restated rule decides the answer when every s2 is 0.  Inside an instance nothing is culled then (0 x lb' is 0 or NaN), so the walk
    of an entered instance is exhaustive; the only test that can lose the true answer is the top-level one, on its instance's world box or on an ancestor of it
    — whose box contains that box and grows by at least as much, so that its f32 distance is no larger.  Decisive: the misses (a record is an accepted candidate
    or the miss record) and the hits whose answer's world box world_culls does not cull at best = the answer's dist2.  This contains the well-conditioned
    queries (condition (2) is the f64 statement of the same test with half the growth) and is not all queries in principle: where the squares underflow, an
    answer's dist2 can be 0 while its world box is a positive f32 distance away, and once another candidate has brought best to 0 that box is culled."""
    c = bf["closest"]
    out = ~bf["hit"]
    for k in np.unique(c["instance"][bf["hit"]]):
        idx = np.nonzero(bf["hit"] & (c["instance"] == k))[0]
        wb = world_box(inst["object_to_world"][k], tris_root_box(blas_tris[int(inst["blas"][k])]))
        out[idx] = ~world_culls(wb, pts["point"][idx], c["dist2"][idx])
    return out


@pytest.mark.parametrize("name", S2_EDGES)
def test_s2_edge_premises(pkg, name):
    """past the edges only the unconditional guarantees are asserted on the GPU.  Which queries remain well-conditioned by the header's definition: under
    s2 = +inf condition (1) reads inf x D <= dist2, which holds for an infinite dist2 only (inf x 0 is NaN: an exact zero-distance hit is not well-conditioned
    either), so the misses and the all-infinite ties are what is left; under s2 = 0 condition (1) always holds and the definition is condition (2) alone"""
    inst, pts, bf = point_reference(pkg, name)
    s2 = scene_s2(instance_inverse(inst["object_to_world"])[0])
    hit, well, d2 = bf["hit"], bf["well"], bf["closest"]["dist2"]
    print(f"points {name:14s} s2 {float(s2[0]):.3g}  hits {hit.sum():4d} of {len(pts)}  well {well.mean():.4f}  well hits {np.count_nonzero(well & hit)}")
    assert (~hit).sum() >= 20 and well[~hit].all()
    if name == "uni_2p65":
        assert (s2 == np.inf).all() and not (well & hit & np.isfinite(d2)).any()
    elif name == "uni_2p-75":
        assert (s2 == 0).all() and hit.sum() >= len(pts) // 4
        assert (d2[hit] < np.finfo(F32).tiny).all() and (d2[hit] == 0).sum() >= 100     # squares underflow: many ties at dist2 = 0, decided by (instance, prim)
        decisive = decisive_under_zero_s2(pkg, pts, meshes(pkg), inst, bf)
        print(f"points {name:14s} the restated rule is decisive on {decisive.sum()} of {len(pts)} queries ({np.count_nonzero(decisive & ~well)} of them ill-conditioned)")
        assert (decisive | ~well).all() and decisive.mean() >= 0.99
    else:
        assert ((s2 > 0) & (s2 < np.finfo(F32).tiny)).all()
    inst, rays, rbf = ray_reference(pkg, name)
    print(f"rays   {name:14s} hits {rbf['hit'].sum():4d} of {len(rays)}  well {rbf['well'].mean():.4f}")


# ---- the deep BLAS under non-rigid instances --------------------------------------------------------------------------------------------------------------------

DEEP_H = 70
# shear_2p4: 0.968 of the rays are well-conditioned.  An unbounded ray is accepted by every one of the 142 parallel triangles, out to t = 1140, and W M differs from
# the identity by about 2^-16 under a shear of 16: at that distance the object-space ray has drifted off the world ray by more than the world box grows, which
# the definition counts against the ray.  The test asserts exactness on the well-conditioned rays of this rung without the 99 % floor; the other three meet it.
DEEP_RAYS_UNCAPPED = ["shear_2p4"]


def deep_instances(pkg, name):
    """five instances of the caterpillar BLAS (test_gpu_query.caterpillar) by the matrices of a rung, each placing the object-space origin where the existing deep
    tests put it: on a grid of spacing 100 (far_2p16: wherever the rung's translation is)"""
    rng = np.random.default_rng([11, DEEP_RUNGS.index(name)])
    family, K = parse(name)
    offs = np.array([(0, 0, 0), (100, 0, 0), (0, 100, 0), (100, 100, 0), (200, 50, 0)], dtype=F64) * (1.0 if family != "far" else 0.0)
    mats = []
    for t in offs:
        M = family_matrix(rng, family, K, np.zeros(3)).astype(F64).reshape(3, 4)
        mats.append(mat34(M[:, :3], M[:, 3] + t))
    return make_instances(pkg, mats, [0] * len(mats))


def deep_queries(pkg, name, m=500):
    """object-space queries as the existing deep tests choose them (below the near face, unbounded; on it; bounded; among the far triangles), each mapped to the
    world by its instance's matrix in f64 and rounded: (instances, points, rays)"""
    inst = deep_instances(pkg, name)
    rng = np.random.default_rng([12, DEEP_RUNGS.index(name)])
    k = rng.integers(0, len(inst), m)
    M = inst["object_to_world"].astype(F64).reshape(-1, 3, 4)[k]
    obj = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-3, -0.5, m)], axis=1)
    obj[: m // 6, 2] = 0.0
    obj[3 * m // 4:, 2] = rng.uniform(1000, 1000 + 2 * DEEP_H, m - 3 * m // 4)
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    pts["point"] = np.einsum("nij,nj->ni", M[:, :, :3], obj) + M[:, :, 3]
    pts["radius"] = np.inf
    smin = np.linalg.svd(M[:, :, :3], compute_uv=False)[:, 2]
    pts["radius"][m // 2: 3 * m // 4] = 5.0 * smin[m // 2: 3 * m // 4]
    ro = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), np.full(m, -1.0)], axis=1)
    rd = np.stack([rng.normal(0, 1e-3, m), rng.normal(0, 1e-3, m), np.ones(m)], axis=1)
    rd[: m // 4, :2] = 0.0
    rays = np.zeros(m, dtype=pkg.RAY)
    rays["origin"] = np.einsum("nij,nj->ni", M[:, :, :3], ro) + M[:, :, 3]
    rays["direction"] = np.einsum("nij,nj->ni", M[:, :, :3], rd)
    rays["tmax"] = 1e30
    rays["tmin"][m // 2:] = rng.uniform(0, 1000 + 2 * DEEP_H, m - m // 2)
    return inst, pts, rays


@pytest.mark.parametrize("name", DEEP_RUNGS)
def test_deep_premises(pkg, name):
    tris, nodes, root, n = caterpillar(pkg, DEEP_H, 3 + DEEP_H)
    inst, pts, rays = deep_queries(pkg, name)
    pbf = scene_point_brute_force(pkg, pts, [tris], inst)
    rbf = scene_brute_force(pkg, rays, [tris], inst)
    print(f"deep {name:14s} points: hits {pbf['hit'].sum()} well {pbf['well'].mean():.4f}   rays: hits {rbf['hit'].sum()} well {rbf['well'].mean():.4f}")
    assert pbf["well"].mean() >= 0.99
    if name in DEEP_RAYS_UNCAPPED:
        assert rbf["well"].mean() < 0.99, f"{name} meets the cap: take it out of DEEP_RAYS_UNCAPPED"
    else:
        assert rbf["well"].mean() >= 0.99
    assert pbf["hit"].sum() >= len(pts) // 4 and rbf["hit"].sum() >= len(rays) // 4


# ---- bvh_scene_closest_point over non-finite BLASes (the counterpart of test_query_extremes' scene rays) ------------------------------------------------------------

def non_finite_scene_points(pkg):
    """(meshes, instances, 256 points, root boxes as stage E makes them) of test_query_extremes' scene: the points are ladder_points on that scene with the base
    mesh in every instance (the special meshes' own extents are NaN or infinite)"""
    if not _NON_FINITE:
        ms = [mesh(pkg, name) for name in SCENE_BLASES]
        inst = non_finite_scene_instances(pkg)
        base = inst.copy(); base["blas"] = SCENE_BLASES.index("base")
        # (the twelve near instances and the one at 2^20 apart: a point of the bounds of all thirteen is about 2^19 from a unit box, where the f32 dist2 is
        # coarser than the box's growth — ill-conditioned by definition, and by nothing that the non-finite BLASes do)
        pts = np.concatenate([ladder_points(pkg, ms, base[:SCENE_FAR], 192, 4244), ladder_points(pkg, ms, base[SCENE_FAR:], 64, 4245)])
        roots = []
        for t in ms:
            b = stage_e_boxes(t)
            roots.append(np.concatenate([b["min"].min(axis=0), b["max"].max(axis=0)]).astype(F32))
        _NON_FINITE.append((ms, inst, pts, roots))
    return _NON_FINITE[0]


def test_non_finite_scene_points_are_well_conditioned(pkg):
    ms, inst, pts, roots = non_finite_scene_points(pkg)
    bf = scene_point_brute_force(pkg, pts, ms, inst, roots)
    answered = set(bf["closest"]["instance"][bf["hit"]].tolist())
    print(f"non-finite BLASes: points well {bf['well'].mean():.4f}, hits {bf['hit'].sum()} of {len(pts)}, {len(answered)} of {len(inst)} instances answer")
    assert bf["well"].mean() >= 0.99 and bf["hit"].sum() >= len(pts) // 4 and (~bf["hit"]).sum() >= 20
    assert len(answered) == len(inst)
