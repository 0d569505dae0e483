"""CPU: bvh_scene_closest_point in the C ABI, the library and the Python binding; the numpy restatement of its maths (include/bvh_mi355x.h: the scale bound s2,
the object-space point and slack, the cull rule) and the two-level point brute force that the GPU tests (tests/test_gpu_scene_point.py) compare against; and the
check that the cull rule never loses a well-conditioned query's answer where an object-space rule without s2 and e does."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_point_query import E_INVALID, WELL_GROW, closest_formula, point_brute_force, point_ok, tri_arrays
from test_query import QUERY_GROW
from test_scene import identity, instance_inverse, make_instances, mat34, rot, tris_root_box, world_box, xf_points

F32 = np.float32
F64 = np.float64
ONE_M20 = F32(1.0) - F32(2.0 ** -20)


# ---- the numpy restatements ---------------------------------------------------------------------------------------------------------------------------------

def scene_s2(w):
    """world_to_object (k, 12) float32 -> the scale bound s2 (k,) float32, in the header's operation order (k_instance_boxes)"""
    w = np.asarray(w, dtype=F32).reshape(-1, 12).astype(F64)
    rows = [w[:, 4 * i: 4 * i + 3] for i in range(3)]
    with np.errstate(all="ignore"):
        lam = np.zeros(len(w))
        for i in range(3):
            S = [np.abs((rows[i][:, 0] * rows[j][:, 0] + rows[i][:, 1] * rows[j][:, 1]) + rows[i][:, 2] * rows[j][:, 2]) for j in range(3)]
            lam = np.maximum(lam, (S[0] + S[1]) + S[2])
        return ((1.0 - 2.0 ** -10) / lam).astype(F32)


def object_points(w, p):
    """(p' = W p, the slack e) in f32 in the header's order; w (12,), p (m, 3)"""
    w = np.asarray(w, dtype=F32); p = np.asarray(p, dtype=F32)
    a = np.abs(p); aw = np.abs(w)
    with np.errstate(all="ignore"):
        r = [((aw[4 * i] * a[:, 0] + aw[4 * i + 1] * a[:, 1]) + aw[4 * i + 2] * a[:, 2]) + aw[4 * i + 3] for i in range(3)]
        e = F32(2.0 ** -20) * np.maximum(np.maximum(r[0], r[1]), r[2])
    return xf_points(w, p), e.astype(F32)


def grown_dist2(lo, hi, p, extra):
    """box_dist_pass's f32 squared distance from p (m, 3) to the boxes lo / hi (m, 3) grown by QUERY_GROW * max|coordinate| + extra (m,)"""
    lo, hi, p = (np.asarray(x, dtype=F32) for x in (lo, hi, p))
    with np.errstate(all="ignore"):
        g = F32(QUERY_GROW) * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1) + np.asarray(extra, dtype=F32)
        d = np.fmax(np.fmax((lo - g[:, None]) - p, p - (hi + g[:, None])), F32(0.0))
        return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)


def scene_culls(lo, hi, pprime, e, s2, best):
    """the cull rule inside an instance, f32: True where the box is culled"""
    lb = grown_dist2(lo, hi, pprime, e)
    with np.errstate(all="ignore"):
        return (np.asarray(s2, dtype=F32) * lb) * ONE_M20 > np.asarray(best, dtype=F32)


def object_rule_culls(lo, hi, pprime, best):
    """what the cull rule must not be: bvh_closest_point's rule on the object-space point against the world-space best (no s2, no e)"""
    lb = grown_dist2(lo, hi, pprime, np.zeros(len(pprime), dtype=F32))
    with np.errstate(all="ignore"):
        return lb * ONE_M20 > np.asarray(best, dtype=F32)


def world_culls(wbox, p, best):
    """the top-level rule on one instance's world box (box_dist_pass, negated)"""
    m = len(p)
    lb = grown_dist2(np.broadcast_to(wbox[:3], (m, 3)), np.broadcast_to(wbox[3:], (m, 3)), p, np.zeros(m, dtype=F32))
    with np.errstate(all="ignore"):
        return ~(lb * ONE_M20 <= np.asarray(best, dtype=F32))


def active_instances(instances, n_blas):
    w, active = instance_inverse(instances["object_to_world"])
    return w, active & (instances["blas"] < n_blas)


def scene_miss_records(pkg, points):
    out = np.zeros(len(points), dtype=pkg.INSTANCE_POINT_HIT)
    with np.errstate(all="ignore"):
        out["dist2"] = points["radius"].astype(F32) * points["radius"].astype(F32)
    out["prim"] = pkg.INVALID; out["instance"] = pkg.INVALID
    return out


def world_triangles(m, tris):
    return tuple(xf_points(m, v) for v in tri_arrays(tris))


def scene_point_brute_force(pkg, points, blas_tris, instances, root_boxes=None, chunk_elems=1 << 21):
    """every query against every world triangle of every active instance.  Returns dict: closest (INSTANCE_POINT_HIT: the accepted candidate with the smallest
    (dist2, instance, prim)), hit, well (the header's two conditions on the answer; a miss is well-conditioned)"""
    n_blas = len(blas_tris)
    if root_boxes is None:
        root_boxes = [tris_root_box(t) for t in blas_tris]
    w, active = active_instances(instances, n_blas)
    s2 = scene_s2(w)
    m = len(points)
    out = scene_miss_records(pkg, points)
    with np.errstate(all="ignore"):
        r2 = points["radius"].astype(F32) * points["radius"].astype(F32)
    ok = point_ok(points)
    p = np.ascontiguousarray(points["point"], dtype=F32)
    cur = np.where(ok, r2, -np.inf).astype(F64)                        # (best dist2 so far: an equal dist2 of a later instance does not replace)
    has_any = np.zeros(m, dtype=bool)
    for k in np.nonzero(active)[0]:
        tris = blas_tris[int(instances["blas"][k])]
        V1, V2, V3 = world_triangles(instances["object_to_world"][k], tris)
        step = max(1, chunk_elems // max(len(tris), 1))
        for s in range(0, m, step):
            sl = slice(s, s + step)
            q, d2, u, v, _ = closest_formula(p[sl, None, :], V1[None], V2[None], V3[None])
            with np.errstate(invalid="ignore"):
                acc = (d2 <= r2[sl, None]) & ok[sl, None]
            mn = np.where(acc, d2, np.inf).min(axis=1)
            cand = acc & (d2 == mn[:, None])
            has = cand.any(axis=1)
            best = cand.argmax(axis=1)                                   # the smallest prim among equal dist2
            rows = np.arange(len(mn))
            better = has & ((mn < cur[sl]) | ~has_any[sl])              # (the first accepted candidate may sit at dist2 == r2)
            o = out[sl]
            o["point"][better] = q[rows, best][better]; o["dist2"][better] = d2[rows, best][better]
            o["u"][better] = u[rows, best][better]; o["v"][better] = v[rows, best][better]
            o["prim"][better] = best[better]; o["instance"][better] = k
            out[sl] = o
            cur[sl] = np.where(better, mn, cur[sl]); has_any[sl] |= better
    well = np.ones(m, dtype=bool)
    hit = out["prim"] != pkg.INVALID
    for k in np.unique(out["instance"][hit]):
        idx = np.nonzero(hit & (out["instance"] == k))[0]
        b = int(instances["blas"][k]); tris = blas_tris[b]
        v1, v2, v3 = tri_arrays(tris)
        j = out["prim"][idx]
        lo = np.minimum(np.minimum(v1[j], v2[j]), v3[j]).astype(F64); hi = np.maximum(np.maximum(v1[j], v2[j]), v3[j]).astype(F64)
        _, e = object_points(w[k], p[idx])
        W = w[k].astype(F64).reshape(3, 4)
        ps = p[idx].astype(F64) @ W[:, :3].T + W[:, 3]
        g = (WELL_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1) + 0.5 * e.astype(F64))[:, None]
        dd = np.maximum(np.maximum((lo - g) - ps, ps - (hi + g)), 0.0)
        d2 = out["dist2"][idx].astype(F64)
        c1 = F64(s2[k]) * (dd * dd).sum(axis=1) <= d2
        wb = world_box(instances["object_to_world"][k], root_boxes[b]).astype(F64)
        gw = WELL_GROW * np.abs(wb).max()
        dw = np.maximum(np.maximum((wb[:3] - gw) - p[idx].astype(F64), p[idx].astype(F64) - (wb[3:] + gw)), 0.0)
        c2 = (dw * dw).sum(axis=1) <= d2
        well[idx] = c1 & c2
    return {"closest": out, "hit": hit, "well": well}


def scene_point_recompute(pkg, points, blas_tris, instances, hits):
    """per record: a hit must be an accepted candidate of its (instance, prim) with bit-equal point / dist2 / u / v; a miss must be the exact miss record"""
    _, active = active_instances(instances, len(blas_tris))
    hit = hits["prim"] != pkg.INVALID
    good = np.zeros(len(points), dtype=bool)
    miss = scene_miss_records(pkg, points)
    good[~hit] = (hits[~hit].view(np.uint8).reshape(-1, 32) == miss[~hit].view(np.uint8).reshape(-1, 32)).all(axis=1)
    for k in np.unique(hits["instance"][hit]):
        if k >= len(instances) or not active[k]:
            continue
        tris = blas_tris[int(instances["blas"][k])]
        idx = np.nonzero(hit & (hits["instance"] == k))[0]
        idx = idx[hits["prim"][idx] < len(tris)]
        j = hits["prim"][idx]
        V1, V2, V3 = world_triangles(instances["object_to_world"][k], tris[j])
        pr = points[idx]
        q, d2, u, v, _ = closest_formula(pr["point"].astype(F32), V1, V2, V3)
        with np.errstate(invalid="ignore"):
            r2 = pr["radius"].astype(F32) * pr["radius"].astype(F32)
            acc = (d2 <= r2) & point_ok(pr)
        h = hits[idx]
        same = (q.view(np.uint32) == h["point"].view(np.uint32)).all(axis=1) & (d2.view(np.uint32) == h["dist2"].view(np.uint32)) & \
               (u.view(np.uint32) == h["u"].view(np.uint32)) & (v.view(np.uint32) == h["v"].view(np.uint32))
        good[idx] = acc & same
    return good


def scene_below(pkg, got, ref):
    """closest answers lexicographically below the brute force's (dist2, instance, prim), or hits where the brute force has none"""
    g = got["prim"] != pkg.INVALID
    r = ref["prim"] != pkg.INVALID
    lt = (got["dist2"] < ref["dist2"]) | ((got["dist2"] == ref["dist2"]) & ((got["instance"] < ref["instance"]) |
                                                                              ((got["instance"] == ref["instance"]) & (got["prim"] < ref["prim"]))))
    return g & ((r & lt) | ~r)


# ---- inputs shared with the GPU tests -------------------------------------------------------------------------------------------------------------------------

def shear_matrix(rng):
    """rotation x diag(0.25 .. 4) x shear x rotation"""
    S = np.eye(3); S[0, 1], S[0, 2], S[1, 2] = rng.uniform(-1.0, 1.0, 3)
    R1 = rot(rng.integers(3), rng.uniform(0, 2 * np.pi)) @ rot(rng.integers(3), rng.uniform(0, 2 * np.pi))
    R2 = rot(rng.integers(3), rng.uniform(0, 2 * np.pi)) @ rot(rng.integers(3), rng.uniform(0, 2 * np.pi))
    return R1 @ np.diag(rng.uniform(0.25, 4.0, 3)) @ S @ R2


def instance_set(pkg, rng, kind, n_inst, n_blas=1):
    """n_inst active instances: "rigid" (rotations, translations within +-3), "aniso" (rotation x diag(0.25 .. 4) x rotation), "shear" (with a shear between) and
    "far" (rigid, translations up to 4096)"""
    mats = []
    for _ in range(n_inst):
        R1 = rot(rng.integers(3), rng.uniform(0, 2 * np.pi)) @ rot(rng.integers(3), rng.uniform(0, 2 * np.pi))
        R2 = rot(rng.integers(3), rng.uniform(0, 2 * np.pi)) @ rot(rng.integers(3), rng.uniform(0, 2 * np.pi))
        t = rng.uniform(-4096.0, 4096.0, 3) if kind == "far" else rng.uniform(-3.0, 3.0, 3)
        A = {"rigid": R1, "far": R1, "aniso": R1 @ np.diag(rng.uniform(0.25, 4.0, 3)) @ R2}[kind] if kind != "shear" else shear_matrix(rng)
        mats.append(mat34(A, t))
    return make_instances(pkg, mats, np.arange(n_inst) % n_blas)


def flat_world_tris(pkg, blas_tris, inst):
    """(world triangles of the active instances concatenated in instance order, instance of each, prim of each)"""
    _, active = active_instances(inst, len(blas_tris))
    parts, ks, js = [], [], []
    for k in np.nonzero(active)[0]:
        t = blas_tris[int(inst["blas"][k])]
        wt = np.zeros(len(t), dtype=pkg.meshgen.TRIANGLE)
        wt["v1"], wt["v2"], wt["v3"] = world_triangles(inst["object_to_world"][k], t)
        parts.append(wt); ks.append(np.full(len(t), k)); js.append(np.arange(len(t)))
    return np.concatenate(parts), np.concatenate(ks), np.concatenate(js)


def near_surface_points(pkg, wtris, m, rng, radius=np.inf):
    """points at offsets 1e-4 .. 3 (log-uniform) in random directions from random points of random world triangles"""
    t = rng.integers(0, len(wtris), m)
    b = rng.dirichlet((1.0, 1.0, 1.0), size=m)
    on = wtris["v1"][t].astype(F64) * b[:, :1] + wtris["v2"][t].astype(F64) * b[:, 1:2] + wtris["v3"][t].astype(F64) * b[:, 2:]
    d = rng.normal(size=(m, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    off = 10.0 ** rng.uniform(-4.0, np.log10(3.0), m)
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    pts["point"] = (on + d * off[:, None]).astype(F32); pts["radius"] = radius
    return pts


def scene_points(pkg, wtris, m, seed, bounded=True):
    """the GPU tests' queries: half near-surface, half uniform in the scene bounds (grown by a tenth); bounded: a third with finite radii and a few dead
    queries, otherwise every radius infinite"""
    rng = np.random.default_rng(seed)
    pts = near_surface_points(pkg, wtris, m, rng)
    v = np.concatenate([wtris["v1"], wtris["v2"], wtris["v3"]]).astype(F64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = hi - lo
    h = m // 2
    pts["point"][h:] = (lo - 0.1 * ext + rng.random((m - h, 3)) * 1.2 * ext).astype(F32)
    if not bounded:
        return pts
    fin = rng.random(m) < 1.0 / 3.0
    pts["radius"][fin] = (10.0 ** rng.uniform(-4.0, 0.0, m))[fin] * np.where(rng.random(m) < 0.5, 0.5, 2.0)[fin]
    dead = rng.choice(m, 8, replace=False)
    pts["point"][dead[0], 0] = np.nan; pts["point"][dead[1], 2] = np.nan
    pts["radius"][dead[2]] = np.nan; pts["radius"][dead[3]] = -1.0; pts["radius"][dead[4]] = -np.inf; pts["radius"][dead[5]] = -0.5
    pts["radius"][dead[6]] = 0.0; pts["radius"][dead[7]] = -0.0                                          # (live: radius 0 accepts dist2 0 only)
    return pts


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------------------

class CInstancePointHit(C.Structure):
    _fields_ = [("point", C.c_float * 3), ("dist2", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim_idx", C.c_uint32), ("instance_idx", C.c_uint32)]


def test_header_declares_the_type_and_the_entry_point(pkg):
    types = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh", "types.h")).read(), flags=re.S)
    assert re.search(r"typedef struct\s*\{\s*bvh_float3 point;\s*float dist2;\s*float u, v;\s*uint32_t prim_idx, instance_idx;\s*\}\s*bvh_instance_point_hit;", types)
    assert re.search(r"static_assert\(sizeof\(bvh_instance_point_hit\) == 32", types)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+bvh_scene_closest_point\s*\(\s*bvh_scene\s*\*\s*\w+\s*,\s*const bvh_point_query\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*"
                     r"bvh_instance_point_hit\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text


def test_library_exports_the_symbol_and_sizes_match(pkg, tmp_path):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_scene_closest_point") and "bvh_scene_closest_point" in pkg.EXPORTS
    assert pkg.lib().bvh_abi_version() == 4
    assert pkg.INSTANCE_POINT_HIT.itemsize == 32 and C.sizeof(CInstancePointHit) == 32
    offs = [pkg.INSTANCE_POINT_HIT.fields[name][1] for name in pkg.INSTANCE_POINT_HIT.names]
    assert offs == [getattr(CInstancePointHit, f[0]).offset for f in CInstancePointHit._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "bvh_mi355x.h"\nint main(void) { printf("%zu", sizeof(bvh_instance_point_hit)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["g++", "-std=c++17", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout == "32"


def test_binding_and_errors_without_a_device(pkg):
    assert callable(getattr(pkg.Scene, "closest_point"))
    L = pkg.lib()
    assert L.bvh_scene_closest_point(None, 16, 1, 64, 0) == E_INVALID
    assert L.bvh_scene_closest_point(None, None, 0, None, 0) == E_INVALID


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------------------------------

def test_s2_hand_cases():
    """s2 is computed from world_to_object: M = identity gives lambda 1; M = diag(0.25, 1, 1) has W = diag(4, 1, 1) and lambda 16 (world distances along x are
    a quarter of the object ones); M = diag(4, 1, 1) has W = diag(0.25, 1, 1) and lambda 1 (no direction shrinks)"""
    def s2_of(M):
        w, active = instance_inverse(M)
        assert active.all()
        return scene_s2(w)[0]
    assert s2_of(identity()) == F32(1.0 - 2.0 ** -10)
    assert s2_of(mat34(np.diag([0.25, 1.0, 1.0]))) == F32((1.0 - 2.0 ** -10) / 16.0)
    assert s2_of(mat34(np.diag([4.0, 1.0, 1.0]))) == F32(1.0 - 2.0 ** -10)
    assert s2_of(mat34(2.0 * rot(2, 0.5) @ rot(0, 1.0), (5.0, -7.0, 9.0))) == pytest.approx(4.0, rel=2e-3)       # rotation x uniform scale: tight


def test_s2_bounds_world_distances_from_below():
    """|M x - p|^2 >= s2 |x - W p|^2 on random points (f64, from the stored f32 matrices), and s2 is within 3x of the tight bound sigma_min(A)^2"""
    rng = np.random.default_rng(1)
    mats = np.array([mat34(shear_matrix(rng), rng.uniform(-3, 3, 3)) for _ in range(64)])
    w, active = instance_inverse(mats)
    assert active.all()
    s2 = scene_s2(w).astype(F64)
    for k in range(len(mats)):
        M = mats[k].astype(F64).reshape(3, 4); W = w[k].astype(F64).reshape(3, 4)
        x = rng.normal(size=(200, 3)) * 3; p = rng.normal(size=(200, 3)) * 3
        lhs = ((x @ M[:, :3].T + M[:, 3] - p) ** 2).sum(axis=1)
        rhs = s2[k] * ((x - (p @ W[:, :3].T + W[:, 3])) ** 2).sum(axis=1)
        assert (lhs >= rhs).all()
        smin2 = np.linalg.svd(M[:, :3], compute_uv=False).min() ** 2
        assert smin2 / 3.0 * (1.0 - 2.0 ** -9) <= s2[k] <= smin2


def test_world_space_metric_hand_case(pkg):
    """under M = diag(4, 1, 1) a triangle at object x = 1 and one at object y = 2, queried from the origin: the second is the answer (world dist2 4, not 16)
    though the first is nearer in object space"""
    tri = np.zeros(2, dtype=pkg.meshgen.TRIANGLE)
    tri["v1"][0] = (1, -1, -1); tri["v2"][0] = (1, 3, -1); tri["v3"][0] = (1, -1, 3)
    tri["v1"][1] = (-1, 2, -1); tri["v2"][1] = (3, 2, -1); tri["v3"][1] = (-1, 2, 3)
    inst = make_instances(pkg, [mat34(np.diag([4.0, 1.0, 1.0]))], [0])
    pts = np.zeros(1, dtype=pkg.POINT_QUERY); pts["radius"] = np.inf
    bf = scene_point_brute_force(pkg, pts, [tri], inst)
    c = bf["closest"][0]
    assert c["prim"] == 1 and c["instance"] == 0 and c["dist2"] == F32(4.0) and tuple(c["point"]) == (0.0, 2.0, 0.0)
    assert bf["well"].all() and scene_point_recompute(pkg, pts, [tri], inst, bf["closest"]).all()
    # in object space the order is the other way round
    obj = point_brute_force(pkg, pts, tri)["closest"][0]
    assert obj["prim"] == 0 and obj["dist2"] == F32(1.0)
    # the cull rule keeps the answer's leaf at best = 4
    w, _ = instance_inverse(inst["object_to_world"])
    pp, e = object_points(w[0], pts["point"])
    v1, v2, v3 = tri_arrays(tri)
    lo, hi = np.minimum(np.minimum(v1, v2), v3), np.maximum(np.maximum(v1, v2), v3)
    s2 = scene_s2(w)
    assert not scene_culls(lo[1:], hi[1:], pp, e, s2, F32(4.0)).any()
    # radius 1.5: both triangles are out of reach in world space (the first is within 1.5 in object space only)
    pts["radius"] = 1.5
    assert not scene_point_brute_force(pkg, pts, [tri], inst)["hit"].any()
    bad = bf["closest"].copy(); bad["instance"][0] = 5
    assert not scene_point_recompute(pkg, pts, [tri], inst, bad)[0]


def test_dead_queries_and_inactive_instances(pkg):
    tri = pkg.meshgen.uniform(20, 3)
    inst = make_instances(pkg, [mat34(np.zeros((3, 3))), identity(), identity()], [0, 0, 7])
    pts = np.zeros(5, dtype=pkg.POINT_QUERY); pts["point"] = 0.5; pts["radius"] = (np.inf, -1.0, np.nan, 1e-6, np.inf)
    pts["point"][4, 1] = np.nan
    bf = scene_point_brute_force(pkg, pts, [tri], inst)
    c = bf["closest"]
    assert list(bf["hit"]) == [True, False, False, False, False] and c["instance"][0] == 1
    assert c["dist2"][1] == F32(1.0) and np.isnan(c["dist2"][2]) and c["dist2"][3] == F32(1e-6) * F32(1e-6)
    assert (c["instance"][1:] == pkg.INVALID).all() and (c["prim"][1:] == pkg.INVALID).all()
    assert scene_point_recompute(pkg, pts, [tri], inst, c).all()


# ---- the brute force against the flattened scene ---------------------------------------------------------------------------------------------------------------

def test_two_level_brute_force_equals_flattened(pkg):
    rng = np.random.default_rng(4)
    meshes = [pkg.meshgen.uniform(40, 1), pkg.meshgen.uniform(25, 2)]
    inst = instance_set(pkg, rng, "shear", 6, n_blas=2)
    inst = np.concatenate([inst, inst[:2]])                           # two coincident pairs: every answer on them ties on dist2
    inst["object_to_world"][3][5] = np.nan                          # and an inactive one
    flat, ks, js = flat_world_tris(pkg, meshes, inst)
    pts = scene_points(pkg, flat, 400, 5)
    got = scene_point_brute_force(pkg, pts, meshes, inst)
    ref = point_brute_force(pkg, pts, flat)["closest"]
    g = got["closest"]
    hit = ref["prim"] != pkg.INVALID
    assert hit.sum() > 200 and (~hit).sum() > 20
    assert np.array_equal(got["hit"], hit)
    for f in ("point", "dist2", "u", "v"):
        assert np.array_equal(g[f].view(np.uint32), ref[f].view(np.uint32))
    assert np.array_equal(g["instance"][hit], ks[ref["prim"][hit]]) and np.array_equal(g["prim"][hit], js[ref["prim"][hit]])
    assert (g["instance"][~hit] == pkg.INVALID).all()
    assert np.isin(g["instance"][hit], [0, 1]).sum() > 20 and not np.isin(g["instance"][hit], [3, 6, 7]).any()     # ties to the lower instance; 3 is inactive
    assert scene_point_recompute(pkg, pts, meshes, inst, g).all()
    assert not scene_below(pkg, g, g).any()


# ---- the cull rule is conservative ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rigid", "aniso", "shear", "far"])
def test_cull_rule_keeps_the_true_leaf(pkg, kind):
    """on well-conditioned queries neither the top-level rule nor the rule inside the instance culls the true answer's boxes with best = the answer's dist2
    (every ancestor's box contains the leaf's and grows by at least as much, and best never drops below the answer's dist2); the object-space rule without s2
    and e does lose it, on the anisotropic and the far-offset sets"""
    rng = np.random.default_rng({"rigid": 1, "aniso": 2, "shear": 3, "far": 4}[kind])
    mesh = pkg.meshgen.uniform(600, 17)
    inst = instance_set(pkg, rng, kind, 8)
    flat, _, _ = flat_world_tris(pkg, [mesh], inst)
    pts = near_surface_points(pkg, flat, 3000, rng)
    bf = scene_point_brute_force(pkg, pts, [mesh], inst)
    c, well = bf["closest"], bf["well"]
    assert bf["hit"].all()
    print(f"{kind}: {well.sum()} of {len(well)} well-conditioned")
    assert well.mean() >= 0.99
    w, _ = instance_inverse(inst["object_to_world"])
    s2 = scene_s2(w)
    v1, v2, v3 = tri_arrays(mesh)
    lo, hi = np.minimum(np.minimum(v1, v2), v3), np.maximum(np.maximum(v1, v2), v3)
    root = tris_root_box(mesh)
    culled = np.zeros(len(pts), dtype=bool); naive = np.zeros(len(pts), dtype=bool)
    for k in range(len(inst)):
        idx = np.nonzero(c["instance"] == k)[0]
        j = c["prim"][idx]
        pp, e = object_points(w[k], pts["point"][idx])
        culled[idx] = scene_culls(lo[j], hi[j], pp, e, np.full(len(idx), s2[k]), c["dist2"][idx]) | \
                      scene_culls(np.broadcast_to(root[:3], (len(idx), 3)), np.broadcast_to(root[3:], (len(idx), 3)), pp, e, np.full(len(idx), s2[k]), c["dist2"][idx]) | \
                      world_culls(world_box(inst["object_to_world"][k], root), pts["point"][idx], c["dist2"][idx])
        naive[idx] = object_rule_culls(lo[j], hi[j], pp, c["dist2"][idx])
    print(f"{kind}: the rule culls {np.count_nonzero(culled & well)} true leaves, the object-space rule {naive.mean():.4f} of them")
    assert not (culled & well).any()
    if kind != "rigid":
        assert naive.any(), "the object-space rule loses nothing on this set: the exact tests would not discriminate"
