"""CPU: bvh_knn in the C ABI, the library, the Python binding and the C++ mirror, and the numpy brute force (every query against every triangle, the k smallest
(dist2, prim) among the accepted candidates) that the GPU tests (tests/test_gpu_knn.py) compare against, with the per-entry recomputation and the
lexicographic "below" check they use on every query."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_point_query import E_INVALID, F32, WELL_GROW, closest_formula, point_brute_force, point_ok, tri_arrays

PAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


class CKnnHit(C.Structure):
    _fields_ = [("dist2", C.c_float), ("prim_idx", C.c_uint32)]


def r2_of(points):
    with np.errstate(all="ignore"):
        return points["radius"].astype(F32) * points["radius"].astype(F32)


def keys_of(d2, prim):
    """the u64 whose order is the contract's lexicographic (dist2, prim) order for dist2 >= 0: (bits of dist2) << 32 | prim"""
    return (np.ascontiguousarray(d2, dtype=F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(prim).astype(np.uint64)


def knn_brute_force(pkg, points, tris, k, chunk_elems=1 << 21):
    """every query against every triangle.  Returns dict: hits (KNN_HIT [m, k]: the min(k, accepted) accepted candidates with the smallest (dist2, prim) in
    ascending order, then {r2, INVALID}), counts (u32 [m]), well (bool: every listed entry meets DESIGN.md §8e's box condition; entry_well [m, k] has it per
    slot), kth_tie (bool: the first excluded accepted candidate has exactly the k-th entry's dist2)."""
    v1, v2, v3 = tri_arrays(tris)
    n, m = len(tris), len(points)
    lo = np.minimum(np.minimum(v1, v2), v3).astype(np.float64); hi = np.maximum(np.maximum(v1, v2), v3).astype(np.float64)
    g = WELL_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True)
    glo, ghi = lo - g, hi + g
    r2 = r2_of(points)
    ok = point_ok(points)
    hits = np.zeros((m, k), dtype=pkg.KNN_HIT)
    hits["dist2"] = r2[:, None]; hits["prim"] = pkg.INVALID
    counts = np.zeros(m, dtype=np.uint32); entry_well = np.ones((m, k), dtype=bool); kth_tie = np.zeros(m, dtype=bool)
    kk = min(k, n)
    prims = np.arange(n, dtype=np.uint64)
    step = max(1, chunk_elems // max(n, 1))
    for s in range(0, m, step):
        p = np.ascontiguousarray(points["point"][s:s + step], dtype=F32)
        c = len(p)
        _, d2, _, _, _ = closest_formula(p[:, None, :], v1[None], v2[None], v3[None])
        with np.errstate(invalid="ignore"):
            acc = (d2 <= r2[s:s + step, None]) & ok[s:s + step, None]
        key = np.where(acc, keys_of(d2, 0).reshape(c, n) | prims[None], PAD_KEY)
        order = np.argsort(key, axis=1, kind="stable")[:, :min(kk + 1, n)]
        rows = np.arange(c)[:, None]
        sel = acc[rows, order]
        lst, lsel = order[:, :kk], sel[:, :kk]
        h = hits[s:s + step]
        h["dist2"][:, :kk] = np.where(lsel, d2[rows, lst], h["dist2"][:, :kk])
        h["prim"][:, :kk] = np.where(lsel, lst, pkg.INVALID)
        hits[s:s + step] = h
        counts[s:s + step] = lsel.sum(axis=1)
        pp = p.astype(np.float64)[:, None, :]
        bd = np.maximum(np.maximum(glo[lst] - pp, pp - ghi[lst]), 0.0)
        entry_well[s:s + step, :kk] = ~lsel | ((bd * bd).sum(axis=2) <= d2[rows, lst].astype(np.float64))
        if n > kk:
            kth_tie[s:s + step] = sel[:, kk] & (d2[rows[:, 0], order[:, kk]] == d2[rows[:, 0], order[:, kk - 1]])
    return {"hits": hits, "counts": counts, "well": entry_well.all(axis=1), "entry_well": entry_well, "kth_tie": kth_tie}


def truncate(pkg, bf, k):
    """the brute force for a smaller k from one computed with a larger: the lists' first k slots"""
    big = bf["hits"]
    assert 1 <= k < big.shape[1]
    hits = np.ascontiguousarray(big[:, :k])
    nxt = big[:, k]
    return {"hits": hits, "counts": np.minimum(bf["counts"], k).astype(np.uint32), "well": bf["entry_well"][:, :k].all(axis=1),
            "entry_well": bf["entry_well"][:, :k], "kth_tie": (nxt["prim"] != pkg.INVALID) & (nxt["dist2"] == hits["dist2"][:, k - 1])}


def recompute_knn(pkg, points, tris, hits, counts=None):
    """per query: the entries before the first INVALID are accepted candidates of their prims with bit-equal dist2, strictly ascending in (dist2, prim); every
    slot from there on is exactly {r2, INVALID}; counts (when given) is the number of entries"""
    v1, v2, v3 = tri_arrays(tris)
    m, k = hits.shape
    valid = hits["prim"] != pkg.INVALID
    cnt = valid.sum(axis=1)
    good = (valid == (np.arange(k)[None] < cnt[:, None])).all(axis=1)                # the entries form a prefix
    r2 = r2_of(points)
    pad_ok = ~valid & (hits["dist2"].view(np.uint32) == r2.view(np.uint32)[:, None])
    good &= (valid | pad_ok).all(axis=1)
    if counts is not None:
        good &= np.asarray(counts) == cnt
    qi, sj = np.nonzero(valid)
    pr = hits["prim"][qi, sj]
    inr = pr < len(tris)
    bad_q = np.unique(qi[~inr]); good[bad_q] = False
    qi, sj, pr = qi[inr], sj[inr], pr[inr]
    p = points[qi]
    _, d2, _, _, _ = closest_formula(p["point"].astype(F32), v1[pr], v2[pr], v3[pr])
    with np.errstate(invalid="ignore"):
        acc = (d2 <= r2[qi]) & point_ok(p)
    entry_ok = acc & (d2.view(np.uint32) == hits["dist2"][qi, sj].view(np.uint32))
    np.logical_and.at(good, qi, entry_ok)
    key = np.where(valid, keys_of(hits["dist2"].reshape(-1), hits["prim"].reshape(-1)).reshape(m, k), PAD_KEY)
    if k > 1:
        good &= ((key[:, 1:] > key[:, :-1]) | ~valid[:, 1:]).all(axis=1)
    return good


def below(pkg, got, ref):
    """lists lexicographically below the brute force's: at the first place where the two differ, got's (dist2, prim) is the smaller (an unused slot counts as
    above every entry)"""
    m, k = ref.shape
    kg = np.where(got["prim"] != pkg.INVALID, keys_of(got["dist2"].reshape(-1), got["prim"].reshape(-1)).reshape(m, k), PAD_KEY)
    kr = np.where(ref["prim"] != pkg.INVALID, keys_of(ref["dist2"].reshape(-1), ref["prim"].reshape(-1)).reshape(m, k), PAD_KEY)
    diff = kg != kr
    first = diff.argmax(axis=1)
    rows = np.arange(m)
    return diff.any(axis=1) & (kg[rows, first] < kr[rows, first])


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_knn_types_and_entry_point(pkg):
    raw = open(os.path.join(ROOT, "include", "bvh", "types.h")).read()
    assert "bvh_knn_hit 8 B" in raw.split("#ifndef")[0]                               # listed in the head comment
    types = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"typedef struct\s*\{\s*float dist2;\s*uint32_t prim_idx;\s*\}\s*bvh_knn_hit;", types)
    assert re.search(r"static_assert\(sizeof\(bvh_knn_hit\) == 8", types)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    assert re.search(r"#define\s+BVH_KNN_MAX_K\s+32\b", text)
    assert re.search(r"\bint\s+bvh_knn\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*const bvh_result\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,\s*"
                     r"const bvh_point_query\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*bvh_knn_hit\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text


def test_library_exports_knn_and_sizes_match(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_knn") and "bvh_knn" in pkg.EXPORTS
    assert C.sizeof(CKnnHit) == 8 and pkg.KNN_HIT.itemsize == 8 and pkg.KNN_MAX_K == 32
    assert [pkg.KNN_HIT.fields[name][1] for name in pkg.KNN_HIT.names] == [getattr(CKnnHit, f[0]).offset for f in CKnnHit._fields_]
    assert pkg.lib().bvh_abi_version() == 4


def test_knn_errors_without_a_device(pkg):
    lib = pkg.lib()
    assert lib.bvh_knn(None, None, None, None, 0, 1, None, None) == E_INVALID
    r = pkg.Result(); r.n_leaves = 4; r.layout = 0; r.d_nodes = 64; r.d_tris = 64
    assert lib.bvh_knn(None, C.byref(r), None, 256, 4, 8, 4096, None) == E_INVALID
    for k in (0, 33):
        assert lib.bvh_knn(None, C.byref(r), None, 256, 4, k, 4096, None) == E_INVALID


def test_builder_classes_have_knn(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "knn"))
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().knn(np.zeros(4, dtype=pkg.POINT_QUERY), 4)           # no tree yet


def test_cpp_mirror_knn_compiles(tmp_path):
    src = tmp_path / "knn_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> void ask(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_point_query* q, uint32_t n, bvh_knn_hit* h, uint32_t* c) {
    B bvh; bvh.build(ctx, a); bvh.knn(ctx, q, n, 8, h, c); bvh.knn(ctx, q, n, BVH_KNN_MAX_K, h, nullptr);
}
void all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_point_query* q, uint32_t n, bvh_knn_hit* h, uint32_t* c) {
    ask<BvhConstruction::TwoPassLbvh>(ctx, a, q, n, h, c); ask<BvhConstruction::SinglePassLbvh>(ctx, a, q, n, h, c);
    ask<BvhConstruction::PLOCNew>(ctx, a, q, n, h, c); ask<BvhConstruction::HPLOC>(ctx, a, q, n, h, c);
}
static_assert(sizeof(bvh_knn_hit) == 8 && BVH_KNN_MAX_K == 32, "sizes");
""")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the brute force ---------------------------------------------------------------------------------------------------------------------------------------

def slabs(pkg, zs):
    tri = np.zeros(len(zs), dtype=pkg.meshgen.TRIANGLE)
    for i, z in enumerate(zs):
        tri["v1"][i] = (-1, -1, z); tri["v2"][i] = (3, -1, z); tri["v3"][i] = (-1, 3, z)
    return tri


def test_brute_force_ties_acceptance_and_padding(pkg):
    # test_point_query's coincident triangles: prims 0 and 1 coincide at z = 2, prim 2 at z = 1 is nearer to the origin side, prim 3 at z = 3
    tri = slabs(pkg, (2.0, 2.0, 1.0, 3.0))
    pts = np.zeros(8, dtype=pkg.POINT_QUERY)
    pts["point"] = (0.25, 0.25, 0.0); pts["radius"] = np.inf
    pts["point"][1] = (0.25, 0.25, 2.5)                              # dist2 0.25 to prims 0, 1 and 3; 2.25 to prim 2
    pts["radius"][2] = 2.0                                          # r2 4: prims 2 (1) and 0, 1 (4 <= 4) accepted, prim 3 (9) not
    pts["radius"][3] = np.nextafter(F32(2.0), F32(0.0))             # r2 < 4: only prim 2
    pts["radius"][4] = 0.0                                          # nothing at distance 0
    pts["radius"][5] = -1.0
    pts["point"][6] = (np.nan, 0.0, 0.0)
    pts["radius"][7] = np.nan
    INV = pkg.INVALID
    bf = knn_brute_force(pkg, pts, tri, 3)
    h = bf["hits"]
    assert h["prim"].tolist() == [[2, 0, 1], [0, 1, 3], [2, 0, 1], [2, INV, INV], [INV] * 3, [INV] * 3, [INV] * 3, [INV] * 3]
    assert h["dist2"][0].tolist() == [1.0, 4.0, 4.0] and h["dist2"][1].tolist() == [0.25, 0.25, 0.25]
    assert h["dist2"][3].tolist() == [1.0, float(r2_of(pts)[3]), float(r2_of(pts)[3])]       # the padding carries r2
    assert h["dist2"][4].tolist() == [0.0] * 3 and h["dist2"][5].tolist() == [1.0] * 3 and np.isnan(h["dist2"][7]).all()
    assert bf["counts"].tolist() == [3, 3, 3, 1, 0, 0, 0, 0]
    assert bf["kth_tie"].tolist() == [False, False, False, False, False, False, False, False] and bf["well"].all()
    # a tie exactly at place k: with k = 2 the list ends inside the coincident pair (query 0) or inside the three-way tie (query 1): the smaller prims stay
    bf2 = knn_brute_force(pkg, pts, tri, 2)
    assert bf2["hits"]["prim"][:3].tolist() == [[2, 0], [0, 1], [2, 0]] and bf2["kth_tie"].tolist()[:4] == [True, True, True, False]
    bf1 = knn_brute_force(pkg, pts, tri, 1)
    assert bf1["hits"]["prim"][:, 0].tolist() == [2, 0, 2, 2, INV, INV, INV, INV] and bf1["kth_tie"].tolist()[:2] == [False, True]
    # k = 1 is bvh_closest_point's (dist2, prim)
    pq = point_brute_force(pkg, pts, tri)["closest"]
    assert bf1["hits"]["prim"][:, 0].tolist() == pq["prim"].tolist()
    assert bf1["hits"]["dist2"][:, 0].tobytes() == pq["dist2"].tobytes()
    # k > n: short lists
    bf8 = knn_brute_force(pkg, pts, tri, 8)
    assert bf8["counts"].tolist() == [4, 4, 3, 1, 0, 0, 0, 0] and bf8["hits"]["prim"][0].tolist() == [2, 0, 1, 3] + [INV] * 4
    assert not bf8["kth_tie"].any()
    for kk, want in ((3, bf), (2, bf2), (1, bf1)):                     # the smaller k from the larger brute force
        t = truncate(pkg, bf8, kk)
        assert all(t[f].tobytes() == want[f].tobytes() for f in ("hits", "counts", "well", "kth_tie")), kk
    for b in (bf, bf2, bf1, bf8):
        assert recompute_knn(pkg, pts, tri, b["hits"], b["counts"]).all()
        assert not below(pkg, b["hits"], b["hits"]).any()


def test_brute_force_on_a_shared_vertex_orders_by_prim(pkg):
    # test_point_query's fan around the origin: a query on the shared vertex is at dist2 0 from all six triangles
    f = 6
    ang = np.linspace(0, 2 * np.pi, f + 1)
    tri = np.zeros(f, dtype=pkg.meshgen.TRIANGLE)
    for i in range(f):
        tri["v1"][i] = (np.cos(ang[i]), np.sin(ang[i]), 0.0); tri["v2"][i] = (0, 0, 0); tri["v3"][i] = (np.cos(ang[i + 1]), np.sin(ang[i + 1]), 0.0)
    pts = np.zeros(2, dtype=pkg.POINT_QUERY)
    pts["radius"] = (0.0, np.inf)
    bf = knn_brute_force(pkg, pts, tri, 4)
    assert bf["hits"]["prim"].tolist() == [[0, 1, 2, 3]] * 2 and (bf["hits"]["dist2"] == 0).all() and bf["kth_tie"].all() and bf["counts"].tolist() == [4, 4]
    assert recompute_knn(pkg, pts, tri, bf["hits"], bf["counts"]).all()


def test_recompute_and_below_catch_tampered_lists(pkg):
    tri = slabs(pkg, (1.0, 2.0, 2.0, 3.0, 5.0))
    pts = np.zeros(3, dtype=pkg.POINT_QUERY)
    pts["point"] = (0.25, 0.25, 0.0); pts["radius"] = (np.inf, 2.5, np.inf)
    bf = knn_brute_force(pkg, pts, tri, 4)
    ref, cnt = bf["hits"], bf["counts"]
    assert ref["prim"].tolist() == [[0, 1, 2, 3], [0, 1, 2, pkg.INVALID], [0, 1, 2, 3]] and cnt.tolist() == [4, 3, 4]
    assert recompute_knn(pkg, pts, tri, ref, cnt).all() and not below(pkg, ref, ref).any()

    def tampered(fn):
        h = ref.copy(); fn(h); return h
    cases = {
        "dist2 one ulp off": tampered(lambda h: h["dist2"].__setitem__((0, 0), np.nextafter(F32(1.0), F32(2.0)))),
        "wrong prim for the dist2": tampered(lambda h: h["prim"].__setitem__((0, 0), 4)),
        "tie in the wrong order": tampered(lambda h: h["prim"].__setitem__((0, slice(1, 3)), (2, 1))),
        "an entry twice": tampered(lambda h: h.__setitem__((0, 2), h[0, 1])),
        "not accepted": tampered(lambda h: h.__setitem__((1, 3), ref[0, 3])),
        "padding dist2": tampered(lambda h: h["dist2"].__setitem__((1, 3), 0.0)),
        "a hole": tampered(lambda h: h.__setitem__((0, 1), np.array((np.inf, pkg.INVALID), dtype=pkg.KNN_HIT))),
        "prim out of range": tampered(lambda h: h["prim"].__setitem__((0, 3), 77)),
    }
    for what, h in cases.items():
        good = recompute_knn(pkg, pts, tri, h, cnt)
        assert not good[:2].all() and good[2], what
    wrong_counts = cnt.copy(); wrong_counts[1] = 4
    assert recompute_knn(pkg, pts, tri, ref, wrong_counts).tolist() == [True, False, True]
    # below: a smaller key at the first difference; a missing entry (shorter list) or a larger key is not below
    lower = ref.copy(); lower["dist2"][0, 1] = 3.0
    assert below(pkg, lower, ref).tolist() == [True, False, False]
    lower = ref.copy(); lower["prim"][0, 2] = 1
    assert below(pkg, lower, ref).tolist() == [True, False, False]
    higher = ref.copy(); higher[0, 1:3] = ref[0, 2:4]; higher[0, 3] = (np.inf, pkg.INVALID)      # prim 1 skipped: above
    assert not below(pkg, higher, ref).any()
    extra = ref.copy(); extra[1, 3] = ref[0, 3]                                                # an entry where the truth has none: below
    assert below(pkg, extra, ref).tolist() == [False, True, False]


def test_point_clouds_as_degenerate_triangles(pkg):
    """v1 == v2 == v3: region A answers, dist2 is the plain f32 (dx*dx + dy*dy) + dz*dz of point sets, ties by index"""
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-2, 2, (500, 3)).astype(F32)
    cloud[100] = cloud[7]                                           # a duplicate point: an exact tie
    tri = np.zeros(len(cloud), dtype=pkg.meshgen.TRIANGLE)
    tri["v1"] = tri["v2"] = tri["v3"] = cloud
    q = rng.uniform(-2, 2, (64, 3)).astype(F32); q[0] = cloud[7]
    pts = np.zeros(len(q), dtype=pkg.POINT_QUERY); pts["point"] = q; pts["radius"] = np.inf
    bf = knn_brute_force(pkg, pts, tri, 16)
    d = cloud[None] - q[:, None]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == F32
    order = np.lexsort((np.broadcast_to(np.arange(len(cloud)), d2.shape), d2), axis=1)[:, :16]
    assert bf["hits"]["prim"].tolist() == order.tolist()
    assert bf["hits"]["dist2"].tobytes() == np.take_along_axis(d2, order, axis=1).tobytes()
    assert bf["hits"]["prim"][0, :2].tolist() == [7, 100] and (bf["counts"] == 16).all() and bf["well"].all()
