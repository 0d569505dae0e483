"""CPU: bvh_closest_tris in the C ABI, the library, the Python binding and the C++ mirror; the numpy restatement of its candidate — segseg_formula (Ericson's
ClosestPtSegmentSegment in float32, operation for operation as the header states it) and tri_tri_formula (the crossing test, the six point-triangle terms and
the nine edge pairs, lowest index on ties) — with rule cases whose answers are exact, the formula checked against an f64 restatement of the same decomposition,
and the brute force that the GPU tests (tests/test_gpu_closest_tris.py) compare against."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_intersect_tris import as_triangles, crosses64, proper64, stage_e_boxes, xyz
from test_point_query import closest_f64, closest_formula, random_triangles

E_INVALID = -10001
F32 = np.float32
F64 = np.float64
WELL_GROW = 2.0 ** -17                  # the growth of either stage-E box in the well-conditioned test (the kernels grow every box by twice that)
CROSSING = 15                           # the feature of a proper crossing
EDGES = ((0, 1), (1, 2), (2, 0))        # edge i = (v[i], v[i + 1]): (v1,v2), (v2,v3), (v3,v1)
# test_formula_against_f64: the largest errors measured on this file's seeds (see the test), and the bounds — 4x the measured value: headroom for other seeds
# (the relative error of dist2 at a separation d is about 2 * 2^-24 * scale / d, so ~1e-4 at the test's floor d = 1e-3 * scale; the sliver kind's distance
# error is tri_closest's own on a sliver 5e-4 away — its interior branch's 1 / ((va + vb) + vc) — and has a bound of its own)
MEASURED_REL = {"random": 7.07e-5, "sliver": 5.47e-5, "collinear": 1.03e-4, "zero_area": 6.11e-5}
MEASURED_ABS = {"random": 8.20e-8, "sliver": 7.37e-6, "collinear": 7.81e-8, "zero_area": 3.35e-7}


class CTriHit(C.Structure):
    _fields_ = [("dist2", C.c_float), ("prim_idx", C.c_uint32), ("feature", C.c_uint32), ("reserved", C.c_uint32)]


# ---- the formula ---------------------------------------------------------------------------------------------------------------------------------------------

def segseg_formula(p1, q1, p2, q2):
    """Ericson's ClosestPtSegmentSegment (Real-Time Collision Detection, 5.1.9) in float32, operation for operation as the header states it: the squared
    distance between the clamped points of segments (p1, q1) and (p2, q2); arguments broadcast over a leading shape with a trailing axis of 3"""
    p1, q1, p2, q2 = (np.asarray(x, dtype=F32) for x in (p1, q1, p2, q2))
    zero, one = F32(0.0), F32(1.0)
    with np.errstate(all="ignore"):
        P1 = [p1[..., k] for k in range(3)]; Q1 = [q1[..., k] for k in range(3)]; P2 = [p2[..., k] for k in range(3)]; Q2 = [q2[..., k] for k in range(3)]
        def sub(x, y): return [x[k] - y[k] for k in range(3)]
        def dot(x, y): return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]
        def clamp(x): return np.where(x < zero, zero, np.where(x > one, one, x)).astype(F32)       # (a NaN passes through)
        d1, d2, r = sub(Q1, P1), sub(Q2, P2), sub(P1, P2)
        a, e, f = dot(d1, d1), dot(d2, d2), dot(d2, r)
        c = dot(d1, r)
        b = dot(d1, d2)
        denom = a * e - b * b
        # the general branch: both segments have a length
        s_g = np.where(denom != zero, clamp((b * f - c * e) / denom), zero).astype(F32)
        t_g = (b * s_g + f) / e
        s_lo, s_hi = clamp(-c / a), clamp((b - c) / a)
        s_gen = np.where(t_g < zero, s_lo, np.where(t_g > one, s_hi, s_g)).astype(F32)
        t_gen = np.where(t_g < zero, zero, np.where(t_g > one, one, t_g)).astype(F32)
        both = (a <= zero) & (e <= zero)
        first = ~both & (a <= zero)                                  # the first segment is a point
        second = ~both & ~first & (e <= zero)                        # the second segment is a point
        s = np.where(both | first, zero, np.where(second, clamp(-c / a), s_gen)).astype(F32)
        t = np.where(both | second, zero, np.where(first, clamp(f / e), t_gen)).astype(F32)
        w = [(P1[k] + d1[k] * s) - (P2[k] + d2[k] * t) for k in range(3)]
        return ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]).astype(F32)


def boxes_overlap(x, y):
    """box_overlap of the two stage-E boxes, pair by pair: comparisons only; an inverted box overlaps nothing"""
    bx, by = stage_e_boxes(x), stage_e_boxes(y)
    with np.errstate(invalid="ignore"):
        return ((bx["min"] <= by["max"]) & (by["min"] <= bx["max"]) & (bx["min"] <= bx["max"]) & (by["min"] <= by["max"])).all(axis=1)


def fifteen_terms(x, y):
    """the 15 float32 terms of dist2(X_k, Y_k), (15, m): 0..2 X's vertices against Y, 3..5 Y's vertices against X, 6 + 3 i + j edge i of X against edge j of Y"""
    x, y = xyz(x), xyz(y)
    terms = np.empty((15, len(x)), dtype=F32)
    for k in range(3):
        terms[k] = closest_formula(x[:, k], y[:, 0], y[:, 1], y[:, 2])[1]
        terms[3 + k] = closest_formula(y[:, k], x[:, 0], x[:, 1], x[:, 2])[1]
    for i, (i0, i1) in enumerate(EDGES):
        for j, (j0, j1) in enumerate(EDGES):
            terms[6 + 3 * i + j] = segseg_formula(x[:, i0], x[:, i1], y[:, j0], y[:, j1])
    return terms


def tri_tri_formula(x, y):
    """(dist2 f32[m], feature u32[m]) of the pairs (X_k, Y_k), the header's dist2(X, Y) step by step: a NaN coordinate on either side gives NaN (never
    accepted); a proper crossing of two triangles whose stage-E boxes overlap gives 0 and feature 15; otherwise the smallest of the 15 terms, the minimum
    starting at +inf and replaced by strictly smaller terms in index order.  x, y: (m, 3, 3) arrays or TRIANGLE records"""
    x, y = xyz(x), xyz(y)
    terms = fifteen_terms(x, y)
    d = np.full(len(x), np.inf, dtype=F32); feat = np.zeros(len(x), dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        for k in range(15):
            lt = terms[k] < d
            d = np.where(lt, terms[k], d).astype(F32); feat = np.where(lt, k, feat).astype(np.uint32)
    cross = boxes_overlap(x, y)
    if cross.any():
        idx = np.nonzero(cross)[0]
        x64, y64 = x[idx].astype(F64), y[idx].astype(F64)
        with np.errstate(invalid="ignore", over="ignore"):
            cross[idx] = proper64(x64) & proper64(y64) & crosses64(x[idx], y[idx])
    d = np.where(cross, F32(0.0), d).astype(F32); feat = np.where(cross, CROSSING, feat).astype(np.uint32)
    nan = np.isnan(x).any(axis=(1, 2)) | np.isnan(y).any(axis=(1, 2))
    d = np.where(nan, F32(np.nan), d).astype(F32); feat = np.where(nan, 0, feat).astype(np.uint32)
    return d, feat


def segseg_f64(p1, q1, p2, q2):
    """the squared distance of two segments in f64, vectorised: the minimum over the four end-point-to-segment distances and, where the two lines' closest
    points fall inside both segments, the distance between the lines — an independent route to the same value (no clamping cascade)"""
    p1, q1, p2, q2 = (np.asarray(v, dtype=F64) for v in (p1, q1, p2, q2))

    def pt_seg(p, a, b):
        d = b - a; dd = (d * d).sum(axis=-1)
        with np.errstate(all="ignore"):
            t = np.where(dd > 0, ((p - a) * d).sum(axis=-1) / np.where(dd > 0, dd, 1.0), 0.0)
        t = np.clip(t, 0.0, 1.0)
        w = p - (a + t[..., None] * d)
        return (w * w).sum(axis=-1)
    best = np.minimum(np.minimum(pt_seg(p1, p2, q2), pt_seg(q1, p2, q2)), np.minimum(pt_seg(p2, p1, q1), pt_seg(q2, p1, q1)))
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, b = (d1 * d1).sum(-1), (d2 * d2).sum(-1), (d1 * d2).sum(-1)
    c, f = (d1 * r).sum(-1), (d2 * r).sum(-1)
    den = a * e - b * b
    with np.errstate(all="ignore"):
        ok = den > 1e-14 * a * e
        s = np.where(ok, (b * f - c * e) / np.where(ok, den, 1.0), -1.0)
        t = np.where(ok, (a * f - b * c) / np.where(ok, den, 1.0), -1.0)
    inside = ok & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    w = (p1 + s[..., None] * d1) - (p2 + t[..., None] * d2)
    return np.where(inside, np.minimum(best, (w * w).sum(-1)), best)


def tri_tri_f64(x, y):
    """the same decomposition in f64, one pair: 0 on a proper crossing (crosses64 is already f64), otherwise the smallest of six independent f64 point-triangle
    distances (test_point_query.closest_f64) and nine f64 segment distances (segseg_f64)"""
    x, y = np.asarray(x, dtype=F32).reshape(3, 3), np.asarray(y, dtype=F32).reshape(3, 3)
    if crosses64(x[None], y[None])[0]:
        return 0.0
    x64, y64 = x.astype(F64), y.astype(F64)
    best = np.inf
    for k in range(3):
        w = closest_f64(x64[k], *y64) - x64[k]; best = min(best, float(w @ w))
        w = closest_f64(y64[k], *x64) - y64[k]; best = min(best, float(w @ w))
    for i0, i1 in EDGES:
        for j0, j1 in EDGES:
            best = min(best, float(segseg_f64(x64[i0], x64[i1], y64[j0], y64[j1])))
    return best


# ---- the brute force -----------------------------------------------------------------------------------------------------------------------------------------

def pair_matrix(queries, tris, chunk_elems=1 << 19):
    """(dist2 f32[m, n], feature u8[m, n]): tri_tri_formula of every query triangle against every tree triangle (radius-independent: computed once per input)"""
    q, t = xyz(queries), xyz(tris)
    m, n = len(q), len(t)
    d2 = np.empty((m, n), dtype=F32); feat = np.empty((m, n), dtype=np.uint8)
    step = max(1, chunk_elems // max(n, 1))
    for s in range(0, m, step):
        qq = q[s:s + step]
        k = len(qq)
        d, f = tri_tri_formula(np.repeat(qq, n, axis=0), np.tile(t, (k, 1, 1)))
        d2[s:s + k] = d.reshape(k, n); feat[s:s + k] = f.reshape(k, n)
    return d2, feat


def radius2(radius):
    with np.errstate(all="ignore"):
        return F32(radius) * F32(radius)


def miss_records(pkg, m, radius):
    out = np.zeros(m, dtype=pkg.TRI_HIT)
    out["dist2"] = radius2(radius); out["prim"] = pkg.INVALID
    return out


def query_ok(queries, radius):
    """live queries: no NaN coordinate, and the call's radius >= 0 (a NaN radius fails the comparison)"""
    with np.errstate(invalid="ignore"):
        return ~np.isnan(xyz(queries)).any(axis=(1, 2)) & bool(F32(radius) >= 0)


def box_gap2_f64(bq, bt):
    """the f64 squared distance between stage-E boxes bq[k] and bt[k], each grown on every axis by WELL_GROW * its largest |coordinate|"""
    qlo, qhi, tlo, thi = (a.astype(F64) for a in (bq["min"], bq["max"], bt["min"], bt["max"]))
    gq = WELL_GROW * np.maximum(np.abs(qlo), np.abs(qhi)).max(axis=1, keepdims=True)
    gt = WELL_GROW * np.maximum(np.abs(tlo), np.abs(thi)).max(axis=1, keepdims=True)
    gap = np.maximum(np.maximum((tlo - gt) - (qhi + gq), (qlo - gq) - (thi + gt)), 0.0)
    return (gap * gap).sum(axis=1)


def tris_brute_force(pkg, queries, tris, radius, pairs=None):
    """every query triangle against every tree triangle.  Returns dict: closest (TRI_HIT records: the smallest (dist2, prim) among the accepted candidates, miss =
    {r2, INVALID, 0, 0}), hit (bool), well (bool: well-conditioned — the f64 squared distance between the two grown stage-E boxes of the answer's pair is <= its
    dist2; a miss is well-conditioned), n_acc.  pairs: pair_matrix(queries, tris), when the caller keeps it across radii"""
    d2, feat = pairs if pairs is not None else pair_matrix(queries, tris)
    m = len(d2)
    r2 = radius2(radius)
    out = miss_records(pkg, m, radius)
    with np.errstate(invalid="ignore"):
        acc = (d2 <= r2) & query_ok(queries, radius)[:, None]
    mn = np.where(acc, d2, np.inf).min(axis=1)
    cand = acc & (d2 == mn[:, None])
    has = cand.any(axis=1)
    best = cand.argmax(axis=1)                                         # the smallest prim among equal dist2
    rows = np.arange(m)
    out["dist2"] = np.where(has, d2[rows, best], out["dist2"])
    out["prim"] = np.where(has, best, pkg.INVALID)
    out["feature"] = np.where(has, feat[rows, best], 0)
    well = np.ones(m, dtype=bool)
    if has.any():
        bq, bt = stage_e_boxes(xyz(queries)[has]), stage_e_boxes(xyz(tris)[best[has]])
        well[has] = box_gap2_f64(bq, bt) <= out["dist2"][has].astype(F64)
    return {"closest": out, "hit": has, "well": well, "n_acc": acc.sum(axis=1)}


def recompute_tris(pkg, queries, tris, radius, hits):
    """per record: a hit must be an accepted candidate of its prim with bit-equal dist2, the same feature and reserved 0; a miss must be the exact miss record"""
    q, t = xyz(queries), xyz(tris)
    hit = hits["prim"] != pkg.INVALID
    good = np.zeros(len(q), dtype=bool)
    miss = miss_records(pkg, len(q), radius)
    good[~hit] = (hits[~hit].view(np.uint8).reshape(-1, 16) == miss[~hit].view(np.uint8).reshape(-1, 16)).all(axis=1)
    idx = np.nonzero(hit)[0]
    pr = hits["prim"][idx]
    inr = pr < len(t)
    idx, pr = idx[inr], pr[inr]
    if len(idx):
        d, f = tri_tri_formula(q[idx], t[pr])
        with np.errstate(invalid="ignore"):
            acc = (d <= radius2(radius)) & query_ok(q[idx], radius)
        h = hits[idx]
        good[idx] = acc & (d.view(np.uint32) == h["dist2"].view(np.uint32)) & (f == h["feature"]) & (h["reserved"] == 0)
    return good


def below(pkg, got, ref):
    """closest answers lexicographically below the brute force's (dist2, prim), or hits where the brute force has none"""
    g = got["prim"] != pkg.INVALID
    r = ref["prim"] != pkg.INVALID
    lt = (got["dist2"] < ref["dist2"]) | ((got["dist2"] == ref["dist2"]) & (got["prim"] < ref["prim"]))
    return g & ((r & lt) | ~r)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_tri_hit_and_entry_point(pkg):
    types = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh", "types.h")).read(), flags=re.S)
    assert re.search(r"typedef struct\s*\{\s*float dist2;\s*uint32_t prim_idx;\s*uint32_t feature;\s*uint32_t reserved;\s*\}\s*bvh_tri_hit;", types)
    assert re.search(r"static_assert\(sizeof\(bvh_tri_hit\) == 16", types)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+bvh_closest_tris\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*const bvh_result\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,\s*"
                     r"const bvh_build_input\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*float\s+\w+\s*,\s*bvh_tri_hit\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text
    full = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    assert "their stage-E boxes overlap exactly" in full and "ClosestPtSegmentSegment" in full       # the contract is in the header


def test_library_exports_closest_tris_and_sizes_match(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_closest_tris") and "bvh_closest_tris" in pkg.EXPORTS
    assert C.sizeof(CTriHit) == 16 and pkg.TRI_HIT.itemsize == 16
    assert [pkg.TRI_HIT.fields[name][1] for name in pkg.TRI_HIT.names] == [getattr(CTriHit, f[0]).offset for f in CTriHit._fields_]
    f = pkg.lib().bvh_closest_tris
    assert len(f.argtypes) == 8 and f.argtypes[5] is C.c_float and f.restype is C.c_int
    assert pkg.lib().bvh_abi_version() == 4


def test_closest_tris_errors_without_a_device(pkg):
    lib = pkg.lib()
    assert lib.bvh_closest_tris(None, None, None, None, 0, 1.0, None, 0) == E_INVALID
    r = pkg.Result(); r.n_leaves = 4; r.layout = 0; r.d_nodes = 64; r.d_tris = 1 << 20
    q = pkg.BuildInput(pkg.TRI_PADDED64, 30, 1 << 21, None, None, 0, 0)
    assert lib.bvh_closest_tris(None, C.byref(r), None, C.byref(q), 4, 1.0, 4096, 0) == E_INVALID          # NULL ctx
    assert lib.bvh_closest_tris(None, C.byref(r), None, None, 4, 1.0, 4096, 0) == E_INVALID                # NULL ctx and queries
    assert lib.bvh_closest_tris(None, C.byref(r), None, C.byref(q), 1 << 30, 1.0, 4096, 0) == E_INVALID    # too many queries
    assert lib.bvh_closest_tris(None, C.byref(r), None, C.byref(q), 0, 1.0, 4096, 2) == E_INVALID          # NULL ctx comes before n_queries == 0


def test_builder_classes_have_closest_tris_and_distance_to(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "closest_tris")) and callable(getattr(cls, "distance_to"))
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().closest_tris(np.zeros(4, dtype=pkg.meshgen.TRIANGLE))           # no tree yet
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().distance_to(np.zeros(4, dtype=pkg.meshgen.TRIANGLE))


def test_cpp_mirror_closest_tris_compiles(tmp_path):
    src = tmp_path / "closest_tris_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> void ask(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_build_input* q, uint32_t n, bvh_tri_hit* h) {
    B bvh; bvh.build(ctx, a); bvh.closestTris(ctx, q, n, 0.5f, h, BVH_QUERY_CLOSEST); bvh.closestTris(ctx, q, n, 0.5f, h, BVH_QUERY_ANY);
}
void all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_build_input* q, uint32_t n, bvh_tri_hit* h) {
    ask<BvhConstruction::TwoPassLbvh>(ctx, a, q, n, h); ask<BvhConstruction::SinglePassLbvh>(ctx, a, q, n, h);
    ask<BvhConstruction::PLOCNew>(ctx, a, q, n, h); ask<BvhConstruction::HPLOC>(ctx, a, q, n, h);
}
static_assert(sizeof(bvh_tri_hit) == 16, "size");
""")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------------------------

UNIT = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]
NAN = float("nan")


def one(x, y):
    d, f = tri_tri_formula(np.asarray(x, dtype=F32).reshape(1, 3, 3), np.asarray(y, dtype=F32).reshape(1, 3, 3))
    return float(d[0]), int(f[0])


def moved(t, dx=0.0, dy=0.0, dz=0.0):
    return [(x + dx, y + dy, z + dz) for x, y, z in t]


@pytest.mark.parametrize("h", [0.5, 0.25, 3.0])
def test_parallel_triangles_offset_along_the_normal(h):
    d, f = one(moved(UNIT, dz=h), UNIT)
    assert d == h * h and f == 0                                      # every vertex term ties at h*h: the lowest index wins
    d, f = one(UNIT, moved(UNIT, dz=h))
    assert d == h * h and f == 0


def test_a_shared_vertex_is_exactly_zero():
    other = [(0.0, 0.0, 0.0), (-1.0, 0.0, 1.0), (0.0, -1.0, 1.0)]
    assert one(other, UNIT) == (0.0, 0)                               # X's v1 lies on Y's v1
    rolled = [other[1], other[2], other[0]]
    assert one(rolled, UNIT) == (0.0, 2)                              # ... now it is X's v3: terms 0 and 1 are positive


def test_a_shared_edge_is_exactly_zero():
    wing = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, -1.0, 1.0)]      # shares the edge (0,0,0)-(1,0,0)
    assert one(wing, UNIT) == (0.0, 0)
    assert one(UNIT, wing) == (0.0, 0)


def test_identical_triangles_are_exactly_zero_and_not_a_crossing():
    t = [(0.5, -2.0, 1.0), (3.0, 0.25, -1.0), (-1.5, 1.0, 2.0)]
    assert one(t, t) == (0.0, 0)


def test_a_proper_crossing_with_all_terms_positive_is_feature_15():
    floor = [(0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0)]
    blade = [(1.0, 1.0, -1.0), (1.0, 1.0, 1.0), (1.5, 1.5, 3.0)]     # its edge (v1, v2) passes through the floor's interior at (1, 1, 0)
    terms = fifteen_terms(np.array(blade, dtype=F32).reshape(1, 3, 3), np.array(floor, dtype=F32).reshape(1, 3, 3))
    assert (terms > 0).all()
    assert one(blade, floor) == (0.0, CROSSING) and one(floor, blade) == (0.0, CROSSING)
    # the same blade lifted off the floor: no crossing, the distance is its lowest vertex's height
    assert one(moved(blade, dz=1.5), floor) == (0.25, 0)


def test_two_skew_edges_give_the_edge_pair_feature():
    # X's edge 1 (v2, v3) runs along x at height 1 over Y's edge 2 (v3, v1), which runs along y: the minimum 1 is attained only between the two edges
    x = [(0.0, 10.0, 5.0), (-1.0, 0.0, 1.0), (1.0, 0.0, 1.0)]
    y = [(0.0, 1.0, 0.0), (10.0, 0.0, -5.0), (0.0, -1.0, 0.0)]
    d, f = one(x, y)
    assert d == 1.0 and f == 6 + 3 * 1 + 2
    d, f = one(y, x)
    assert d == 1.0 and f == 6 + 3 * 2 + 1
    assert float(segseg_formula(x[1], x[2], y[2], y[0])) == 1.0


def test_a_vertex_over_a_face_interior_gives_the_vertex_feature():
    big = [(-4.0, -4.0, 0.0), (8.0, -4.0, 0.0), (-4.0, 8.0, 0.0)]
    tip = [(5.0, 5.0, 9.0), (6.0, 5.0, 9.0), (0.25, 0.5, 2.0)]       # v3 hangs over the face's interior
    assert one(tip, big) == (4.0, 2)
    assert one(big, tip) == (4.0, 5)                                  # the same vertex, now Y's: feature 3 + 2


def test_degenerate_queries_are_ordinary_candidates():
    point = [(0.25, 0.25, 2.0)] * 3
    assert one(point, UNIT) == (4.0, 0)
    segment = [(0.25, 0.25, 1.0), (0.25, 0.25, 3.0), (0.25, 0.25, 3.0)]
    assert one(segment, UNIT) == (1.0, 0)
    # a segment THROUGH the triangle's interior is not a crossing (a zero-area triangle is not proper) and no vertex or edge of either touches the other:
    # the 15 terms do not see it — the contract's known blind spot for degenerate queries
    through = [(0.25, 0.25, -1.0), (0.25, 0.25, 1.0), (0.25, 0.25, 1.0)]
    d, f = one(through, UNIT)
    assert d > 0 and f != CROSSING
    assert one(point, point) == (0.0, 0)                              # two points: the segment formula's first branch, and before it the vertex term


@pytest.mark.parametrize("which", ["x", "y"])
def test_a_nan_vertex_is_never_accepted(which):
    bad = [(0.0, 0.0, 1.0), (1.0, NAN, 1.0), (0.0, 1.0, 1.0)]
    d, f = one(bad, UNIT) if which == "x" else one(UNIT, bad)
    assert np.isnan(d) and f == 0                                     # although the terms of the clean vertices and of the clean edge are finite
    terms = fifteen_terms(np.array(UNIT, dtype=F32).reshape(1, 3, 3), np.array(bad, dtype=F32).reshape(1, 3, 3))
    assert np.isfinite(terms).any()
    with np.errstate(invalid="ignore"):
        assert not (d <= F32(np.inf))


def test_the_lowest_index_wins_on_tied_terms():
    # X's v2 and v3 both at height 2 over the face, v1 higher: terms 1 and 2 tie, and so do the edge terms of edge (v2, v3)
    big = [(-4.0, -4.0, 0.0), (8.0, -4.0, 0.0), (-4.0, 8.0, 0.0)]
    x = [(0.0, 0.0, 5.0), (0.5, 0.5, 2.0), (1.0, 0.5, 2.0)]
    assert one(x, big) == (4.0, 1)
    # a vertex term and an edge term tie at 0 on a shared vertex: the vertex term has the lower index
    assert one([(1.0, 0.0, 0.0), (2.0, 0.0, 1.0), (2.0, 1.0, 1.0)], UNIT) == (0.0, 0)


def test_segseg_branches():
    z = (0.0, 0.0, 0.0)
    assert float(segseg_formula(z, z, (3.0, 4.0, 0.0), (3.0, 4.0, 0.0))) == 25.0                    # two points
    assert float(segseg_formula(z, z, (1.0, -1.0, 0.0), (1.0, 1.0, 0.0))) == 1.0                    # a point and a segment
    assert float(segseg_formula((1.0, -1.0, 0.0), (1.0, 1.0, 0.0), z, z)) == 1.0                    # a segment and a point
    assert float(segseg_formula((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 2.0), (1.0, 0.0, 2.0))) == 4.0      # parallel: denom == 0, s = 0
    assert float(segseg_formula((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (3.0, 0.0, 0.0), (5.0, 0.0, 0.0))) == 4.0      # collinear, apart: t < 0, s clamps to 1
    assert float(segseg_formula((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (-5.0, 0.0, 0.0), (-3.0, 0.0, 0.0))) == 9.0    # ... on the other side: t > 1
    assert float(segseg_formula((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 1.0, 0.0))) == 0.0    # crossing segments
    assert np.isnan(segseg_formula((NAN, 0.0, 0.0), (1.0, 0.0, 0.0), z, (0.0, 1.0, 0.0)))


# ---- the formula against f64 ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["random", "sliver", "collinear", "zero_area"])
def test_formula_against_f64(kind):
    """tri_tri_formula against tri_tri_f64 on the triangle kinds of test_point_query.random_triangles (X of the named kind against a Y of every kind, Y moved
    by 1e-3, 0.3 or 3 units).  Two figures, each bounded by 4x what this file's seeds measured (MEASURED_*): on pairs at least 1e-3 of their coordinates' scale
    apart the relative error of dist2, and on every pair the error of the distance over the scale (a relative error is meaningless at contact).  As in
    test_point_query, a collinear triangle that rounding sends to tri_closest's interior branch answers a point of its line, not of its segment: pairs whose
    winning term is such a point-triangle term are exempt (counted, at most 5 %)."""
    rng = np.random.default_rng({"random": 31, "sliver": 32, "collinear": 33, "zero_area": 34}[kind])
    m = 600
    xa = np.stack(random_triangles(rng, m, kind), axis=1)
    yk = rng.integers(0, 4, m)
    ya = np.empty_like(xa)
    for k, name in enumerate(("random", "sliver", "collinear", "zero_area")):
        sel = yk == k
        ya[sel] = np.stack(random_triangles(rng, int(sel.sum()), name), axis=1)
    shift = rng.normal(size=(m, 3)) * rng.choice([1e-3, 0.3, 3.0], size=(m, 1))
    ya = (ya.astype(F64) - ya.astype(F64).mean(axis=1, keepdims=True) + xa.astype(F64).mean(axis=1, keepdims=True) + shift[:, None, :]).astype(F32)
    d, feat = tri_tri_formula(xa, ya)
    assert np.isfinite(d).all() and (d >= 0).all()
    # the exemption: the winner is a point-triangle term of a collinear / zero-area triangle evaluated in the interior branch
    exempt = np.zeros(m, dtype=bool)
    for i in range(m):
        if feat[i] < 6:
            tri, p = (ya[i], xa[i][feat[i]]) if feat[i] < 3 else (xa[i], ya[i][feat[i] - 3])
            flat = not proper64(tri[None].astype(F64))[0] or kind == "collinear" or yk[i] == 2
            exempt[i] = flat and closest_formula(p, tri[0], tri[1], tri[2])[4] == 6
    assert exempt.mean() <= 0.05, exempt.mean()
    rel_max, abs_max = 0.0, 0.0
    for i in np.nonzero(~exempt)[0]:
        ref = tri_tri_f64(xa[i], ya[i])
        scale = float(max(np.abs(np.stack([xa[i], ya[i]])).max(), 1.0))
        abs_max = max(abs_max, abs(np.sqrt(F64(d[i])) - np.sqrt(ref)) / scale)
        if np.sqrt(ref) >= 1e-3 * scale:
            rel_max = max(rel_max, abs(F64(d[i]) - ref) / ref)
    print(f"{kind}: largest relative error of dist2 {rel_max:.3e}, largest distance error / scale {abs_max:.3e}")
    assert rel_max <= 4 * MEASURED_REL[kind], (kind, rel_max)
    assert abs_max <= 4 * MEASURED_ABS[kind], (kind, abs_max)


# ---- the brute force -----------------------------------------------------------------------------------------------------------------------------------------

def plates(pkg, zs):
    t = np.zeros(len(zs), dtype=pkg.meshgen.TRIANGLE)
    for i, z in enumerate(zs):
        t["v1"][i] = (-1, -1, z); t["v2"][i] = (3, -1, z); t["v3"][i] = (-1, 3, z)
    return t


def test_brute_force_tie_break_and_acceptance(pkg):
    # prims 0 and 1 coincide (a tie at equal dist2); prim 2 is nearer; prim 3 lies farther
    tri = plates(pkg, (2.0, 2.0, 1.0, 3.0))
    q = as_triangles(pkg, np.array([moved(UNIT, dz=0.0), moved(UNIT, dz=2.5), moved(UNIT, dz=0.0), [(NAN, 0, 0), (1, 0, 0), (0, 1, 0)]], dtype=F32))
    pairs = pair_matrix(q, tri)
    bf = tris_brute_force(pkg, q, tri, np.inf, pairs)
    c = bf["closest"]
    assert list(c["prim"]) == [2, 0, 2, pkg.INVALID] and list(c["dist2"][:3]) == [1.0, 0.25, 1.0] and list(c["feature"]) == [0, 0, 0, 0]
    assert list(bf["n_acc"]) == [4, 4, 4, 0] and bf["well"].all() and list(bf["hit"]) == [True, True, True, False]
    assert np.isinf(c["dist2"][3])                                    # the miss record carries r2
    assert recompute_tris(pkg, q, tri, np.inf, c).all()
    # dist2 1 <= r2 1: accepted (<=); just below: nothing, and the miss carries r2
    assert list(tris_brute_force(pkg, q, tri, 1.0, pairs)["closest"]["prim"]) == [2, 0, 2, pkg.INVALID]
    r = float(np.nextafter(F32(1.0), F32(0.0)))
    lo = tris_brute_force(pkg, q, tri, r, pairs)
    assert not lo["hit"][0] and lo["closest"]["dist2"][0] == F32(r) * F32(r) and list(lo["n_acc"]) == [0, 3, 0, 0]
    # a negative radius: every query misses, dist2 is still radius * radius; a NaN radius: NaN
    neg = tris_brute_force(pkg, q, tri, -1.0, pairs)
    assert not neg["hit"].any() and (neg["closest"]["dist2"] == 1.0).all() and recompute_tris(pkg, q, tri, -1.0, neg["closest"]).all()
    nan = tris_brute_force(pkg, q, tri, np.nan, pairs)
    assert not nan["hit"].any() and np.isnan(nan["closest"]["dist2"]).all() and recompute_tris(pkg, q, tri, np.nan, nan["closest"]).all()
    # what recompute_tris and below must catch
    bad = c.copy(); bad["reserved"][0] = 1
    assert not recompute_tris(pkg, q, tri, np.inf, bad)[0]
    bad = c.copy(); bad["feature"][0] = 1
    assert not recompute_tris(pkg, q, tri, np.inf, bad)[0]
    bad = c.copy(); bad["prim"][0] = 3                                # prim 3's dist2 is 9, not 1
    assert not recompute_tris(pkg, q, tri, np.inf, bad)[0]
    assert not below(pkg, c, c).any()
    lower = c.copy(); lower["prim"][1] = 0; lower["dist2"][1] = F32(0.125)
    assert below(pkg, lower, c)[1]


def test_brute_force_reports_crossings_and_the_well_conditioned_flag(pkg):
    tri = plates(pkg, (0.0, 5.0))
    blade = [(0.5, 0.5, -1.0), (0.5, 0.5, 1.0), (0.75, 0.75, 3.0)]
    q = as_triangles(pkg, np.array([blade, moved(blade, dz=1.5)], dtype=F32))
    bf = tris_brute_force(pkg, q, tri, np.inf)
    assert list(bf["closest"]["prim"]) == [0, 0] and list(bf["closest"]["feature"]) == [CROSSING, 0] and list(bf["closest"]["dist2"]) == [0.0, 0.25]
    assert bf["well"].all()
    # the grown boxes' gap is what the flag compares with dist2: 0.5 between the plate's box at z = 0 and the lifted blade's at z in [0.5, 4.5]
    bq, bt = stage_e_boxes(xyz(q)[1:]), stage_e_boxes(xyz(tri)[:1])
    gap2 = float(box_gap2_f64(bq, bt)[0])
    assert 0.24 < gap2 < 0.25                                         # 0.5 less the two growths, squared
