"""CPU: bvh_intersect in the C ABI, the library, the Python binding and the C++ mirror, and the numpy brute-force reference the GPU query tests
(tests/test_gpu_query.py) compare against — itself checked against the oracle's CPU traversal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

E_INVALID = -10001
# every box grows on every axis by QUERY_GROW * its largest |coordinate|; a ray is well-conditioned when every accepted hit's point lies in its
# triangle's box grown by half that
QUERY_GROW = 2.0 ** -16
F32 = np.float32


class CRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("direction", C.c_float * 3), ("tmin", C.c_float), ("tmax", C.c_float)]


class CHit(C.Structure):
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim_idx", C.c_uint32)]


def tri_vertices(tris):
    """TRIANGLE records -> (v1, v2, v3) float32 arrays of shape (n, 3)"""
    return (np.ascontiguousarray(tris["v1"], dtype=F32), np.ascontiguousarray(tris["v2"], dtype=F32), np.ascontiguousarray(tris["v3"], dtype=F32))


def tri_formula(o, d, v0, v1, v2):
    """intersectTriangle (reference src/Common.h:516-531) in float32, operation for operation; arguments broadcast over a leading shape with a trailing axis of 3.
    Returns (it, iu, iv, iw)."""
    with np.errstate(all="ignore"):
        def add(a, b): return [a[k] + b[k] for k in range(3)]
        def cross(a, b): return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        def dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
        ov = [o[..., k] for k in range(3)]; dv = [d[..., k] for k in range(3)]
        a0 = [v0[..., k] for k in range(3)]; a1 = [v1[..., k] for k in range(3)]; a2 = [v2[..., k] for k in range(3)]
        p0 = [a0[k] - ov[k] for k in range(3)]; p1 = [a1[k] - ov[k] for k in range(3)]; p2 = [a2[k] - ov[k] for k in range(3)]
        e0 = [a2[k] - a0[k] for k in range(3)]; e1 = [a0[k] - a1[k] for k in range(3)]; e2 = [a1[k] - a2[k] for k in range(3)]
        nrm = cross(e1, e0)
        u = dot(cross(add(p0, p2), e0), dv); v = dot(cross(add(p1, p0), e1), dv); w = dot(cross(add(p2, p1), e2), dv)
        tt = dot(p0, nrm) * F32(2.0); den = dot(nrm, dv) * F32(2.0)
        return tt / den, u / den, v / den, w / den


def accepted(it, iu, iv, iw, tmin, tmax):
    with np.errstate(invalid="ignore"):
        return (iu > 0) & (iv > 0) & (iw > 0) & (tmin < it) & (it < tmax)


def ray_ok(rays):
    o, d = rays["origin"], rays["direction"]
    with np.errstate(invalid="ignore"):
        return ~(np.isnan(o).any(axis=1) | np.isnan(d).any(axis=1)) & (rays["tmin"] < rays["tmax"])


def brute_force(rays, tris, chunk_elems=1 << 22):
    """every ray against every triangle.  Returns dict: closest (HIT records: smallest (t, prim), miss = {tmax, 0, 0, INVALID}), hit (bool), well (bool:
    well-conditioned), tie (bool: another prim has exactly the closest t), n_acc (accepted hits per ray)."""
    from bvh_pkg import load
    pkg = load()
    v0, v1, v2 = tri_vertices(tris)
    n, m = len(tris), len(rays)
    lo = np.minimum(np.minimum(v0, v1), v2).astype(np.float64); hi = np.maximum(np.maximum(v0, v1), v2).astype(np.float64)
    g = 0.5 * QUERY_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True)
    glo, ghi = lo - g, hi + g
    out = np.zeros(m, dtype=pkg.HIT)
    out["t"] = rays["tmax"]; out["prim"] = pkg.INVALID
    well = np.ones(m, dtype=bool); tie = np.zeros(m, dtype=bool); n_acc = np.zeros(m, dtype=np.int64)
    ok = ray_ok(rays)
    step = max(1, chunk_elems // max(n, 1))
    for s in range(0, m, step):
        r = rays[s:s + step]
        o = np.ascontiguousarray(r["origin"], dtype=F32)[:, None, :]; d = np.ascontiguousarray(r["direction"], dtype=F32)[:, None, :]
        it, iu, iv, iw = tri_formula(o, d, v0[None], v1[None], v2[None])
        acc = accepted(it, iu, iv, iw, r["tmin"][:, None], r["tmax"][:, None]) & ok[s:s + step, None]
        n_acc[s:s + step] = acc.sum(axis=1)
        tk = np.where(acc, it, np.inf)
        best = tk.argmin(axis=1)                                       # first (smallest) prim among equal t
        rows = np.arange(len(r))
        has = acc[rows, best]
        bt = tk[rows, best]
        out["t"][s:s + step] = np.where(has, bt, r["tmax"])
        out["u"][s:s + step] = np.where(has, iu[rows, best], 0)
        out["v"][s:s + step] = np.where(has, iv[rows, best], 0)
        out["prim"][s:s + step] = np.where(has, best, pkg.INVALID)
        tie[s:s + step] = has & ((tk == bt[:, None]).sum(axis=1) > 1)
        # well-conditioned: every accepted hit's point (f64) inside its prim's box grown by half the kernel's growth
        ri, pi = np.nonzero(acc)
        if ri.size:
            p = r["origin"][ri].astype(np.float64) + it[ri, pi].astype(np.float64)[:, None] * r["direction"][ri].astype(np.float64)
            inside = ((p >= glo[pi]) & (p <= ghi[pi])).all(axis=1)
            bad = np.zeros(len(r), dtype=bool); np.logical_or.at(bad, ri, ~inside)
            well[s:s + step] &= ~bad
    return {"closest": out, "hit": out["prim"] != pkg.INVALID, "well": well, "tie": tie, "n_acc": n_acc}


def recompute(rays, tris, hits):
    """per reported hit: is it an accepted hit of that prim with bit-equal t / u / v?  (misses: True iff the record is the miss record)"""
    from bvh_pkg import load
    pkg = load()
    v0, v1, v2 = tri_vertices(tris)
    hit = hits["prim"] != pkg.INVALID
    good = np.zeros(len(rays), dtype=bool)
    miss_ok = (hits["t"].view(np.uint32) == rays["tmax"].view(np.uint32)) & (hits["u"] == 0) & (hits["v"] == 0)
    good[~hit] = miss_ok[~hit]
    idx = np.nonzero(hit)[0]
    p = hits["prim"][idx]
    inr = p < len(tris)
    idx, p = idx[inr], p[inr]
    r = rays[idx]
    it, iu, iv, iw = tri_formula(r["origin"].astype(F32), r["direction"].astype(F32), v0[p], v1[p], v2[p])
    acc = accepted(it, iu, iv, iw, r["tmin"], r["tmax"]) & ray_ok(r)
    same = (it.view(np.uint32) == hits["t"][idx].view(np.uint32)) & (iu.view(np.uint32) == hits["u"][idx].view(np.uint32)) & \
           (iv.view(np.uint32) == hits["v"][idx].view(np.uint32))
    good[idx] = acc & same
    return good


def header_text():
    return open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()


def test_header_declares_query_types_and_entry_point(pkg):
    types = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh", "types.h")).read(), flags=re.S)
    assert re.search(r"typedef struct BVH_ALIGNAS\(32\)\s*\{\s*bvh_float3 origin, direction;\s*float tmin, tmax;\s*\}\s*bvh_ray;", types)
    assert re.search(r"typedef struct\s*\{\s*float t, u, v;\s*uint32_t prim_idx;\s*\}\s*bvh_hit;", types)
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert re.search(r"BVH_QUERY_CLOSEST\s*=\s*0\s*,\s*BVH_QUERY_ANY\s*=\s*1", text)
    assert re.search(r"\bint\s+bvh_intersect\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*const bvh_result\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,\s*"
                     r"const bvh_ray\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*bvh_hit\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text


def test_library_exports_intersect_and_sizes_match(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_intersect") and "bvh_intersect" in pkg.EXPORTS
    assert C.sizeof(CRay) == 32 and C.sizeof(CHit) == 16
    assert pkg.RAY.itemsize == 32 and pkg.HIT.itemsize == 16
    for dt, cs in ((pkg.RAY, CRay), (pkg.HIT, CHit)):
        offs = [dt.fields[name][1] for name in dt.names]
        assert offs == [getattr(cs, f[0]).offset for f in cs._fields_]
    assert (pkg.QUERY_CLOSEST, pkg.QUERY_ANY) == (0, 1)


def test_intersect_errors_without_a_device(pkg):
    lib = pkg.lib()
    assert lib.bvh_intersect(None, None, None, None, 0, None, 0) == E_INVALID
    r = pkg.Result(); r.n_leaves = 4; r.layout = 0; r.d_nodes = 64; r.d_tris = 64
    assert lib.bvh_intersect(None, C.byref(r), None, 256, 4, 4096, 0) == E_INVALID


def test_builder_classes_have_intersect(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "intersect"))
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().intersect(np.zeros(4, dtype=pkg.RAY))                # no tree yet


def test_cpp_mirror_intersect_compiles(tmp_path):
    src = tmp_path / "query_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> void shoot(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_ray* r, uint32_t n, bvh_hit* h) {
    B bvh; bvh.build(ctx, a); bvh.intersect(ctx, r, n, h, BVH_QUERY_CLOSEST); bvh.intersect(ctx, r, n, h, BVH_QUERY_ANY);
}
void all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_ray* r, uint32_t n, bvh_hit* h) {
    shoot<BvhConstruction::TwoPassLbvh>(ctx, a, r, n, h); shoot<BvhConstruction::SinglePassLbvh>(ctx, a, r, n, h);
    shoot<BvhConstruction::PLOCNew>(ctx, a, r, n, h); shoot<BvhConstruction::HPLOC>(ctx, a, r, n, h);
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_brute_force_picks_smallest_t_then_smallest_prim(pkg):
    # two coincident triangles (a tie) and one nearer: the nearer wins; without it the smaller index wins the tie
    tri = np.zeros(3, dtype=pkg.meshgen.TRIANGLE)
    for i, z in enumerate((2.0, 2.0, 1.0)):
        tri["v1"][i] = (-1, -1, z); tri["v2"][i] = (3, -1, z); tri["v3"][i] = (-1, 3, z)
    rays = np.zeros(3, dtype=pkg.RAY)
    rays["origin"] = (0.25, 0.25, 0.0); rays["direction"] = (0.0, 0.0, 1.0); rays["tmax"] = 100.0
    rays["tmin"][1] = 1.5                                               # window past the nearer one: a tie of prims 0 and 1
    rays["tmax"][2] = 1.0                                               # t < tmax is strict: the hit at t = 1 is cut off
    bf = brute_force(rays, tri)
    assert list(bf["closest"]["prim"]) == [2, 0, pkg.INVALID]
    assert list(bf["tie"]) == [False, True, False] and bf["closest"]["t"][2] == np.float32(1.0)
    assert list(bf["n_acc"]) == [3, 2, 0]


def identity_transform(pkg):
    xf = np.zeros(1, dtype=pkg.TRANSFORMATION)
    xf["scale"][0] = (1.0, 1.0, 1.0); xf["quat"][0] = (0.0, 0.0, 0.0, 1.0)
    return xf


def to_u8(f):
    return np.clip(f.astype(F32), F32(0.0), F32(4294967040.0)).astype(np.uint32).astype(np.uint8)


@pytest.mark.parametrize("name", ["cornell32", "cornell82"])
@pytest.mark.parametrize("algo", [1, 2])
def test_brute_force_matches_oracle_traversal(pkg, orc, name, algo):
    """the brute force's closest hits coloured like the reference's image equal the oracle's while-while traversal of the oracle's tree (identity transform) in every
    pixel whose ray is well-conditioned and has no exact-t tie between two prims"""
    tris = pkg.meshgen.load_tri(os.path.join(GOLDEN, name + ".tri")); n = len(tris)
    W = 128
    cam, _ = pkg.cornell_view()
    rays = orc.generate_rays(cam, W, W)
    t = orc.build_tree(algo, tris)
    onodes = t["nodes"] if t["layout"] == 0 else orc.ploc_to_lbvh_layout(t["nodes"], t["leaves"])
    img, overflow = orc.trace_while(rays, tris, onodes, identity_transform(pkg), t["root"], W, n - 1)
    assert overflow == 0
    bf = brute_force(rays, tris)
    c = bf["closest"]
    assert bf["hit"].sum() > W * W // 4, "the view must see geometry"
    mine = np.zeros((W * W, 4), dtype=np.uint8)
    h = bf["hit"]
    u, v = c["u"].astype(F32), c["v"].astype(F32)
    mine[h, 0] = to_u8(u[h] * F32(255)); mine[h, 1] = to_u8(v[h] * F32(255))
    mine[h, 2] = to_u8((F32(1) - u[h] - v[h]) * F32(255)); mine[h, 3] = 255
    keep = bf["well"] & ~bf["tie"]
    excluded = np.count_nonzero(~keep)
    assert excluded <= W * W // 100, f"{excluded} pixels excluded"
    diff = (mine != img.reshape(-1, 4)).any(axis=1) & keep
    assert not diff.any(), f"{diff.sum()} pixels differ (first {np.nonzero(diff)[0][:8]})"
