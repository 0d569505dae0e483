"""CPU: bvh_closest_point in the C ABI, the library, the Python binding and the C++ mirror, and the numpy restatement of its candidate formula and brute force
that the GPU point-query tests (tests/test_gpu_point_query.py) compare against — the formula itself checked against an independent f64 closest point."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

E_INVALID = -10001
# a query is well-conditioned when the f64 squared distance from its point to the closest answer's triangle box, grown on every axis by
# WELL_GROW * that box's largest |coordinate|, is <= the answer's dist2 (the kernels grow every box by twice that)
WELL_GROW = 2.0 ** -17
F32 = np.float32
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "interior")


class CPointQuery(C.Structure):
    _fields_ = [("point", C.c_float * 3), ("radius", C.c_float)]


class CPointHit(C.Structure):
    _fields_ = [("point", C.c_float * 3), ("dist2", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim_idx", C.c_uint32), ("reserved", C.c_uint32)]


def closest_formula(p, a, b, c):
    """Ericson's ClosestPtPointTriangle (Real-Time Collision Detection, 5.1.5) in float32, operation for operation as the header states it; arguments broadcast
    over a leading shape with a trailing axis of 3.  Returns (q (..., 3), dist2, u, v, region) with region an index into REGIONS."""
    p, a, b, c = (np.asarray(x, dtype=F32) for x in (p, a, b, c))
    shape = np.broadcast_shapes(p.shape, a.shape, b.shape, c.shape)[:-1]
    with np.errstate(all="ignore"):
        P = [p[..., k] for k in range(3)]; A = [a[..., k] for k in range(3)]; B = [b[..., k] for k in range(3)]; Cc = [c[..., k] for k in range(3)]
        def sub(x, y): return [x[k] - y[k] for k in range(3)]
        def dot(x, y): return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]
        ab, ac, ap, bp, cp = sub(B, A), sub(Cc, A), sub(P, A), sub(P, B), sub(P, Cc)
        d1, d2 = dot(ab, ap), dot(ac, ap)
        d3, d4 = dot(ab, bp), dot(ac, bp)
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        t_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = e43 / (e43 + e56)
        denom = F32(1.0) / ((va + vb) + vc)
        tv, tw = vb * denom, vc * denom
        cand = [
            (A, F32(0.0), F32(0.0)),
            (B, F32(1.0), F32(0.0)),
            ([A[k] + t_ab * ab[k] for k in range(3)], t_ab, F32(0.0)),
            (Cc, F32(0.0), F32(1.0)),
            ([A[k] + w_ac * ac[k] for k in range(3)], F32(0.0), w_ac),
            ([B[k] + w_bc * (Cc[k] - B[k]) for k in range(3)], F32(1.0) - w_bc, w_bc),
            ([(A[k] + ab[k] * tv) + ac[k] * tw for k in range(3)], tv, tw),
        ]
        conds = [
            (d1 <= 0) & (d2 <= 0),
            (d3 >= 0) & (d4 <= d3),
            (vc <= 0) & (d1 >= 0) & (d3 <= 0),
            (d6 >= 0) & (d5 <= d6),
            (vb <= 0) & (d2 >= 0) & (d6 <= 0),
            (va <= 0) & (e43 >= 0) & (e56 >= 0),
            np.ones(shape, dtype=bool),
        ]
        region = np.full(shape, 6, dtype=np.int64)
        taken = np.zeros(shape, dtype=bool)
        for r, cond in enumerate(conds[:6]):
            m = np.broadcast_to(cond, shape) & ~taken
            region[m] = r; taken |= m
        q = np.zeros(shape + (3,), dtype=F32); u = np.zeros(shape, dtype=F32); v = np.zeros(shape, dtype=F32)
        for r, (qq, uu, vv) in enumerate(cand):
            m = region == r
            for k in range(3):
                q[..., k] = np.where(m, np.broadcast_to(qq[k], shape), q[..., k])
            u = np.where(m, np.broadcast_to(uu, shape), u).astype(F32); v = np.where(m, np.broadcast_to(vv, shape), v).astype(F32)
        dx, dy, dz = q[..., 0] - P[0], q[..., 1] - P[1], q[..., 2] - P[2]
        d2s = (dx * dx + dy * dy) + dz * dz
    return q, d2s.astype(F32), u, v, region


def closest_f64(p, a, b, c):
    """an independent f64 closest point of triangle (a, b, c) to p (one point, one triangle): the projection onto the plane when it falls inside, otherwise the
    nearest of the three edge segments (clamped); degenerate triangles take the segments only"""
    p, a, b, c = (np.asarray(x, dtype=np.float64) for x in (p, a, b, c))

    def seg(x, y):
        d = y - x; dd = d @ d
        t = 0.0 if dd == 0 else min(max((p - x) @ d / dd, 0.0), 1.0)
        return x + t * d
    best = min((seg(a, b), seg(a, c), seg(b, c)), key=lambda q: (q - p) @ (q - p))
    n = np.cross(b - a, c - a); nn = n @ n
    if nn > 1e-24 * max((b - a) @ (b - a), (c - a) @ (c - a)) ** 2:
        q = p - ((p - a) @ n / nn) * n
        inside = all(np.cross(y - x, q - x) @ n >= 0 for x, y in ((a, b), (b, c), (c, a)))
        if inside and (q - p) @ (q - p) < (best - p) @ (best - p):
            best = q
    return best


def point_ok(points):
    x = points["point"]
    with np.errstate(invalid="ignore"):
        return ~np.isnan(x).any(axis=1) & (points["radius"] >= 0)


def tri_arrays(tris):
    return (np.ascontiguousarray(tris["v1"], dtype=F32), np.ascontiguousarray(tris["v2"], dtype=F32), np.ascontiguousarray(tris["v3"], dtype=F32))


def miss_records(pkg, points):
    out = np.zeros(len(points), dtype=pkg.POINT_HIT)
    with np.errstate(all="ignore"):
        out["dist2"] = points["radius"].astype(F32) * points["radius"].astype(F32)
    out["prim"] = pkg.INVALID
    return out


def point_brute_force(pkg, points, tris, chunk_elems=1 << 21):
    """every query against every triangle.  Returns dict: closest (POINT_HIT records: smallest (dist2, prim) among the accepted candidates, miss = {0, 0, 0, r2,
    0, 0, INVALID, 0}), hit (bool), well (bool: well-conditioned), tie (bool: another accepted prim has exactly the closest dist2), n_acc."""
    v1, v2, v3 = tri_arrays(tris)
    n, m = len(tris), len(points)
    lo = np.minimum(np.minimum(v1, v2), v3).astype(np.float64); hi = np.maximum(np.maximum(v1, v2), v3).astype(np.float64)
    g = WELL_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True)
    glo, ghi = lo - g, hi + g
    out = miss_records(pkg, points)
    with np.errstate(all="ignore"):
        r2 = points["radius"].astype(F32) * points["radius"].astype(F32)
    ok = point_ok(points)
    well = np.ones(m, dtype=bool); tie = np.zeros(m, dtype=bool); n_acc = np.zeros(m, dtype=np.int64)
    step = max(1, chunk_elems // max(n, 1))
    for s in range(0, m, step):
        pr = points[s:s + step]
        p = np.ascontiguousarray(pr["point"], dtype=F32)
        q, d2, u, v, _ = closest_formula(p[:, None, :], v1[None], v2[None], v3[None])
        with np.errstate(invalid="ignore"):
            acc = (d2 <= r2[s:s + step, None]) & ok[s:s + step, None]
        n_acc[s:s + step] = acc.sum(axis=1)
        mn = np.where(acc, d2, np.inf).min(axis=1)
        cand = acc & (d2 == mn[:, None])
        has = cand.any(axis=1)
        best = cand.argmax(axis=1)                                     # the smallest prim among equal dist2
        rows = np.arange(len(pr))
        o = out[s:s + step]
        o["point"] = np.where(has[:, None], q[rows, best], 0)
        o["dist2"] = np.where(has, d2[rows, best], o["dist2"])
        o["u"] = np.where(has, u[rows, best], 0); o["v"] = np.where(has, v[rows, best], 0)
        o["prim"] = np.where(has, best, pkg.INVALID)
        out[s:s + step] = o
        tie[s:s + step] = has & (cand.sum(axis=1) > 1)
        # well-conditioned: f64 squared distance from the point to the winner's grown box <= the winner's dist2
        bi = best[has]
        pp = p[has].astype(np.float64)
        dd = np.maximum(np.maximum(glo[bi] - pp, pp - ghi[bi]), 0.0)
        box_d2 = (dd * dd).sum(axis=1)
        w = np.ones(len(pr), dtype=bool)
        w[has] = box_d2 <= d2[rows, best][has].astype(np.float64)
        well[s:s + step] = w
    return {"closest": out, "hit": out["prim"] != pkg.INVALID, "well": well, "tie": tie, "n_acc": n_acc}


def recompute_points(pkg, points, tris, hits):
    """per record: a hit must be an accepted candidate of its prim with bit-equal point / dist2 / u / v and reserved 0; a miss must be the exact miss record"""
    v1, v2, v3 = tri_arrays(tris)
    hit = hits["prim"] != pkg.INVALID
    good = np.zeros(len(points), dtype=bool)
    miss = miss_records(pkg, points)
    good[~hit] = (hits[~hit].view(np.uint8).reshape(-1, 32) == miss[~hit].view(np.uint8).reshape(-1, 32)).all(axis=1)
    idx = np.nonzero(hit)[0]
    pr = hits["prim"][idx]
    inr = pr < len(tris)
    idx, pr = idx[inr], pr[inr]
    p = points[idx]
    q, d2, u, v, _ = closest_formula(p["point"].astype(F32), v1[pr], v2[pr], v3[pr])
    with np.errstate(invalid="ignore"):
        r2 = p["radius"].astype(F32) * p["radius"].astype(F32)
        acc = (d2 <= r2) & point_ok(p)
    h = hits[idx]
    same = (q.view(np.uint32) == h["point"].view(np.uint32)).all(axis=1) & (d2.view(np.uint32) == h["dist2"].view(np.uint32)) & \
           (u.view(np.uint32) == h["u"].view(np.uint32)) & (v.view(np.uint32) == h["v"].view(np.uint32)) & (h["reserved"] == 0)
    good[idx] = acc & same
    return good


def below(pkg, got, ref):
    """closest answers lexicographically below the brute force's (dist2, prim), or hits where the brute force has none"""
    g = got["prim"] != pkg.INVALID
    r = ref["prim"] != pkg.INVALID
    lt = (got["dist2"] < ref["dist2"]) | ((got["dist2"] == ref["dist2"]) & (got["prim"] < ref["prim"]))
    return g & ((r & lt) | ~r)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_point_query_types_and_entry_point(pkg):
    types = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh", "types.h")).read(), flags=re.S)
    assert re.search(r"typedef struct\s*\{\s*bvh_float3 point;\s*float radius;\s*\}\s*bvh_point_query;", types)
    assert re.search(r"typedef struct\s*\{\s*bvh_float3 point;\s*float dist2;\s*float u, v;\s*uint32_t prim_idx, reserved;\s*\}\s*bvh_point_hit;", types)
    assert re.search(r"static_assert\(sizeof\(bvh_point_query\) == 16", types) and re.search(r"static_assert\(sizeof\(bvh_point_hit\) == 32", types)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+bvh_closest_point\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*const bvh_result\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,\s*"
                     r"const bvh_point_query\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*bvh_point_hit\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text


def test_library_exports_closest_point_and_sizes_match(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_closest_point") and "bvh_closest_point" in pkg.EXPORTS
    assert C.sizeof(CPointQuery) == 16 and C.sizeof(CPointHit) == 32
    assert pkg.POINT_QUERY.itemsize == 16 and pkg.POINT_HIT.itemsize == 32
    for dt, cs in ((pkg.POINT_QUERY, CPointQuery), (pkg.POINT_HIT, CPointHit)):
        offs = [dt.fields[name][1] for name in dt.names]
        assert offs == [getattr(cs, f[0]).offset for f in cs._fields_]
    assert pkg.lib().bvh_abi_version() == 4


def test_closest_point_errors_without_a_device(pkg):
    lib = pkg.lib()
    assert lib.bvh_closest_point(None, None, None, None, 0, None, 0) == E_INVALID
    r = pkg.Result(); r.n_leaves = 4; r.layout = 0; r.d_nodes = 64; r.d_tris = 64
    assert lib.bvh_closest_point(None, C.byref(r), None, 256, 4, 4096, 0) == E_INVALID
    assert lib.bvh_closest_point(None, C.byref(r), None, 256, 0, 4096, 1) == E_INVALID


def test_builder_classes_have_closest_point(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "closest_point"))
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().closest_point(np.zeros(4, dtype=pkg.POINT_QUERY))    # no tree yet


def test_cpp_mirror_closest_point_compiles(tmp_path):
    src = tmp_path / "point_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> void ask(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_point_query* q, uint32_t n, bvh_point_hit* h) {
    B bvh; bvh.build(ctx, a); bvh.closestPoint(ctx, q, n, h, BVH_QUERY_CLOSEST); bvh.closestPoint(ctx, q, n, h, BVH_QUERY_ANY);
}
void all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_point_query* q, uint32_t n, bvh_point_hit* h) {
    ask<BvhConstruction::TwoPassLbvh>(ctx, a, q, n, h); ask<BvhConstruction::SinglePassLbvh>(ctx, a, q, n, h);
    ask<BvhConstruction::PLOCNew>(ctx, a, q, n, h); ask<BvhConstruction::HPLOC>(ctx, a, q, n, h);
}
static_assert(sizeof(bvh_point_query) == 16 && sizeof(bvh_point_hit) == 32, "sizes");
""")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the formula ----------------------------------------------------------------------------------------------------------------------------------------

UNIT = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
# (point, region, closest point, (u, v)) on the unit right triangle a = origin, b = x, c = y: one case per region, all exact in f32
REGION_CASES = [
    ((-1.0, -1.0, 1.0), "A", (0.0, 0.0, 0.0), (0.0, 0.0)),
    ((2.0, -0.5, 0.0), "B", (1.0, 0.0, 0.0), (1.0, 0.0)),
    ((0.5, -1.0, 0.0), "AB", (0.5, 0.0, 0.0), (0.5, 0.0)),
    ((-0.5, 2.0, 0.0), "C", (0.0, 1.0, 0.0), (0.0, 1.0)),
    ((-1.0, 0.25, 3.0), "AC", (0.0, 0.25, 0.0), (0.0, 0.25)),
    ((1.0, 1.0, 0.0), "BC", (0.5, 0.5, 0.0), (0.5, 0.5)),
    ((0.25, 0.25, 2.0), "interior", (0.25, 0.25, 0.0), (0.25, 0.25)),
]


@pytest.mark.parametrize("case", REGION_CASES, ids=[c[1] for c in REGION_CASES])
def test_formula_regions_exact(case):
    p, region, want, uv = case
    q, d2, u, v, r = closest_formula(np.array(p), *(np.array(x) for x in UNIT))
    assert REGIONS[int(r)] == region
    assert q.tolist() == list(want) and (float(u), float(v)) == uv
    d = np.array(p, dtype=np.float64) - np.array(want)
    assert float(d2) == float(d @ d)


def test_formula_vertices_and_edges_are_exact():
    a, b, c = (np.array(x, dtype=F32) for x in ((0.5, -2.0, 1.0), (3.0, 0.25, -1.0), (-1.5, 1.0, 2.0)))
    for p, uv in ((a, (0.0, 0.0)), (b, (1.0, 0.0)), (c, (0.0, 1.0))):
        q, d2, u, v, _ = closest_formula(p, a, b, c)
        assert q.tobytes() == p.tobytes() and float(d2) == 0.0 and (float(u), float(v)) == uv


def random_triangles(rng, m, kind):
    a = rng.normal(size=(m, 3))
    if kind == "random":
        b, c = a + rng.normal(size=(m, 3)), a + rng.normal(size=(m, 3))
    elif kind == "sliver":                                          # one short side, or one very flat angle
        e = rng.normal(size=(m, 3)); f = rng.normal(size=(m, 3))
        b = a + e
        c = np.where(rng.random((m, 1)) < 0.5, a + 1e-3 * f, a + 0.5 * e + 1e-3 * f)
    elif kind == "collinear":
        e = rng.normal(size=(m, 3))
        b, c = a + e, a + rng.uniform(-1.5, 1.5, (m, 1)) * e
    else:                                                           # zero area: two or three equal vertices
        b = np.where(rng.random((m, 1)) < 0.5, a, a + rng.normal(size=(m, 3)))
        c = a.copy()
    return a.astype(F32), b.astype(F32), c.astype(F32)


@pytest.mark.parametrize("kind", ["random", "sliver", "collinear", "zero_area"])
def test_formula_against_f64_closest_point(kind):
    """within 1e-6 of the coordinates' scale of an independent f64 closest point, except on collinear triangles that rounding sends to the interior branch
    (va, vb, vc rounding noise around 0: Ericson's formula then answers a point of the triangle's line, not of its segment — DESIGN.md §8e)"""
    rng = np.random.default_rng({"random": 1, "sliver": 2, "collinear": 3, "zero_area": 4}[kind])
    m, tol = 3000, 1e-6
    a, b, c = random_triangles(rng, m, kind)
    p = (a + rng.normal(size=(m, 3)) * rng.choice([1e-3, 0.3, 3.0], size=(m, 1))).astype(F32)
    q, d2, u, v, region = closest_formula(p, a, b, c)
    assert np.isfinite(d2).all() and (d2 >= 0).all()
    exempt = (region == REGIONS.index("interior")) if kind == "collinear" else np.zeros(m, dtype=bool)
    assert exempt.mean() <= 0.05
    for i in np.nonzero(~exempt)[0]:
        ref = closest_f64(p[i], a[i], b[i], c[i])
        dref = float(np.linalg.norm(ref - p[i].astype(np.float64)))
        scale = float(max(np.abs(np.stack([a[i], b[i], c[i], p[i]])).max(), 1.0))
        assert abs(np.sqrt(np.float64(d2[i])) - dref) <= tol * scale, (kind, i, REGIONS[region[i]], float(np.sqrt(d2[i])), dref)
        # dist2 is the squared distance to the reported point, and the weights reproduce that point
        dq = q[i].astype(np.float64) - p[i]
        assert abs(dq @ dq - d2[i]) <= 1e-5 * max(dq @ dq, 1e-30) + 1e-30
        w = a[i].astype(np.float64) + u[i] * (b[i].astype(np.float64) - a[i]) + v[i] * (c[i].astype(np.float64) - a[i])
        assert np.abs(w - q[i]).max() <= tol * scale
        assert 0 <= u[i] <= 1 and 0 <= v[i] <= 1 and u[i] + v[i] <= 1 + 1e-6
    if kind == "random":
        assert set(region.tolist()) == set(range(7)), "every region is reached"


def test_formula_nan_vertex_is_never_accepted(pkg):
    a, b, c = (np.array(x, dtype=F32) for x in UNIT)
    b = b.copy(); b[1] = np.nan
    _, d2, _, _, _ = closest_formula(np.array((0.2, 0.2, 0.0)), a, b, c)
    assert np.isnan(d2)


# ---- the brute force ---------------------------------------------------------------------------------------------------------------------------------------

def test_brute_force_tie_break_and_acceptance(pkg):
    # prims 0 and 1 coincide (a tie at equal dist2); prim 2 is nearer; prim 3 lies farther
    tri = np.zeros(4, dtype=pkg.meshgen.TRIANGLE)
    for i, z in enumerate((2.0, 2.0, 1.0, 3.0)):
        tri["v1"][i] = (-1, -1, z); tri["v2"][i] = (3, -1, z); tri["v3"][i] = (-1, 3, z)
    pts = np.zeros(7, dtype=pkg.POINT_QUERY)
    pts["point"] = (0.25, 0.25, 0.0); pts["radius"] = np.inf
    pts["point"][1] = (0.25, 0.25, 2.5)                              # equidistant from prims 0 / 1 (0.25) and prim 3 (0.25): smallest prim wins
    pts["radius"][2] = 1.0                                          # dist2 1 <= r2 1: accepted (<=)
    pts["radius"][3] = np.nextafter(F32(1.0), F32(0.0))             # r2 < 1: nothing accepted; the miss carries r2
    pts["radius"][4] = -1.0                                         # negative radius: a miss whose dist2 is still radius * radius
    pts["point"][5] = (np.nan, 0.0, 0.0)
    pts["radius"][6] = np.nan
    bf = point_brute_force(pkg, pts, tri)
    c = bf["closest"]
    assert list(c["prim"]) == [2, 0, 2, pkg.INVALID, pkg.INVALID, pkg.INVALID, pkg.INVALID]
    assert list(bf["tie"]) == [False, True, False, False, False, False, False]
    assert list(bf["n_acc"]) == [4, 4, 1, 0, 0, 0, 0]
    assert c["dist2"][0] == F32(1.0) and c["dist2"][1] == F32(0.25) and tuple(c["point"][1]) == (0.25, 0.25, 2.0)
    assert c["dist2"][3] == pts["radius"][3] * pts["radius"][3] and c["dist2"][4] == F32(1.0) and np.isnan(c["dist2"][6])
    assert bf["well"].all()
    assert recompute_points(pkg, pts, tri, c).all()
    bad = c.copy(); bad["reserved"][0] = 1
    assert not recompute_points(pkg, pts, tri, bad)[0]
    assert not below(pkg, c, c).any()
    lower = c.copy(); lower["prim"][1] = 0; lower["dist2"][1] = F32(0.125)
    assert below(pkg, lower, c)[1]


def test_brute_force_on_a_shared_vertex_picks_the_smallest_prim(pkg):
    # a fan of triangles around the origin: a query on the shared vertex is at dist2 0 from all of them
    k = 6
    ang = np.linspace(0, 2 * np.pi, k + 1)
    tri = np.zeros(k, dtype=pkg.meshgen.TRIANGLE)
    for i in range(k):
        tri["v1"][i] = (np.cos(ang[i]), np.sin(ang[i]), 0.0); tri["v2"][i] = (0, 0, 0); tri["v3"][i] = (np.cos(ang[i + 1]), np.sin(ang[i + 1]), 0.0)
    pts = np.zeros(2, dtype=pkg.POINT_QUERY)
    pts["radius"] = (0.0, np.inf)
    bf = point_brute_force(pkg, pts, tri)
    assert list(bf["closest"]["prim"]) == [0, 0] and bf["tie"].all() and (bf["closest"]["dist2"] == 0).all()
    assert (bf["closest"]["u"] == 1).all() and (bf["closest"]["v"] == 0).all()       # the shared vertex is v2
