"""CPU: bvh_radius_search in the C ABI, the library, the Python binding and the C++ mirror; the numpy brute force (every query against every triangle, all
accepted candidates in ascending (dist2, prim) order) and the checker that the GPU tests (tests/test_gpu_radius.py) use on every answer, pinned by tampered
slices and hand-made cases; and what the brute force alone says of the GPU tests' inputs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_point_query import make_points
from test_gpu_query import mesh
from test_knn import keys_of, r2_of, slabs
from test_point_query import E_INVALID, F32, WELL_GROW, closest_formula, point_ok, tri_arrays

RADIUS_SORTED = 1
RADIUS_MESHES = [f"uniform_{n}" for n in (2, 3, 63, 64, 65, 1000)] + ["sponza_1000", "cornell32", "cornell82", "cornell382"]
KNN_HIT = np.dtype([("dist2", "<f4"), ("prim", "<u4")])


def slice_queries(offsets):
    """the query index of every record of a compressed-row answer"""
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets.astype(np.int64)))


def host_sort(offsets, hits):
    """every slice in ascending (dist2, prim) order"""
    return hits[np.lexsort((keys_of(hits["dist2"], hits["prim"]), slice_queries(offsets)))]


def radius_brute_force(pkg, points, tris, chunk_elems=1 << 21, workers=1):
    """every query against every triangle.  Returns dict: offsets (u32 [m + 1]), hits (KNN_HIT, every slice ALL the accepted candidates in ascending
    (dist2, prim) order), counts (i64 [m]), well (bool [m]: every accepted triangle meets DESIGN.md §8e's box condition), tie (bool [m]: two records of the
    slice have exactly the same dist2).  workers > 1: the chunks of queries on that many threads (numpy releases the interpreter lock)."""
    v1, v2, v3 = tri_arrays(tris)
    n, m = len(tris), len(points)
    lo = np.minimum(np.minimum(v1, v2), v3).astype(np.float64); hi = np.maximum(np.maximum(v1, v2), v3).astype(np.float64)
    g = WELL_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True)
    glo, ghi = lo - g, hi + g
    r2 = r2_of(points)
    ok = point_ok(points)
    step = max(1, chunk_elems // max(n, 1))

    def chunk(s):
        p = np.ascontiguousarray(points["point"][s:s + step], dtype=F32)
        _, d2, _, _, _ = closest_formula(p[:, None, :], v1[None], v2[None], v3[None])
        with np.errstate(invalid="ignore"):
            acc = (d2 <= r2[s:s + step, None]) & ok[s:s + step, None]
        qi, pr = np.nonzero(acc)
        dd = d2[qi, pr]
        order = np.lexsort((keys_of(dd, pr), qi))
        qi, pr, dd = qi[order], pr[order], dd[order]
        rec = np.zeros(len(qi), dtype=pkg.KNN_HIT); rec["dist2"] = dd; rec["prim"] = pr
        pp = p.astype(np.float64)[qi]
        bd = np.maximum(np.maximum(glo[pr] - pp, pp - ghi[pr]), 0.0)
        well = np.ones(len(p), dtype=bool); tie = np.zeros(len(p), dtype=bool)
        np.logical_and.at(well, qi, (bd * bd).sum(axis=1) <= dd.astype(np.float64))
        if len(qi) > 1:
            tie[qi[1:][(qi[1:] == qi[:-1]) & (dd[1:] == dd[:-1])]] = True
        return rec, acc.sum(axis=1), well, tie
    starts = range(0, m, step)
    if workers > 1 and len(starts) > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(workers) as pool:
            parts = list(pool.map(chunk, starts))
    else:
        parts = [chunk(s) for s in starts]
    counts = np.concatenate([x[1] for x in parts]).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)
    offsets = np.zeros(m + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(counts)
    hits = np.concatenate([x[0] for x in parts]) if parts else np.zeros(0, dtype=pkg.KNN_HIT)
    well = np.concatenate([x[2] for x in parts]) if parts else np.zeros(0, dtype=bool)
    tie = np.concatenate([x[3] for x in parts]) if parts else np.zeros(0, dtype=bool)
    return {"offsets": offsets, "hits": hits, "counts": counts, "well": well, "tie": tie}


def check_radius(points, tris, ref, offsets, hits, sorted_, what=""):
    """the GPU tests' checker.  Every query: the offsets are a scan from 0 up to len(hits); each record recomputes bit for bit as an accepted candidate of its
    primitive; no primitive appears twice in a slice; each slice is a subset of the brute force's; a sorted answer is strictly ascending in the key
    (dist2, prim).  Well-conditioned queries: the slice equals the truth — the counts are equal, a sorted fill is byte-equal to the brute force's slice and an
    unsorted one is after a host sort (compared as sets)."""
    n, m = len(tris), len(points)
    off = offsets.astype(np.int64)
    assert len(off) == m + 1 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(hits), f"{what}: offsets are not a scan of the slices"
    q = slice_queries(offsets)
    prim = hits["prim"].astype(np.int64)
    assert (prim < n).all(), f"{what}: a primitive index out of range"
    v1, v2, v3 = tri_arrays(tris)
    p = points[q]
    _, d2, _, _, _ = closest_formula(np.ascontiguousarray(p["point"], dtype=F32), v1[prim], v2[prim], v3[prim])
    with np.errstate(invalid="ignore"):
        acc = (d2 <= r2_of(points)[q]) & point_ok(p)
    same = d2.view(np.uint32) == np.ascontiguousarray(hits["dist2"]).view(np.uint32)
    assert (acc & same).all(), f"{what}: {np.count_nonzero(~(acc & same))} records are not accepted candidates of their prims with a bit-equal dist2"
    key = q * n + prim
    assert len(np.unique(key)) == len(key), f"{what}: a primitive appears twice in a slice"
    ref_q = slice_queries(ref["offsets"])
    ref_key = ref_q * n + ref["hits"]["prim"].astype(np.int64)
    assert np.isin(key, ref_key).all(), f"{what}: a slice is not a subset of the true set"
    if sorted_ and len(hits) > 1:
        nxt = q[1:] == q[:-1]
        k = keys_of(hits["dist2"], hits["prim"])
        asc = k[1:] > k[:-1]
        assert asc[nxt].all(), f"{what}: {np.count_nonzero(~asc & nxt)} slices are not strictly ascending in (dist2, prim)"
    well = ref["well"]
    counts, ref_counts = np.diff(off), np.diff(ref["offsets"].astype(np.int64))
    assert (counts == ref_counts)[well].all(), f"{what}: counts differ on {np.count_nonzero((counts != ref_counts) & well)} well-conditioned queries"
    got = hits if sorted_ else host_sort(offsets, hits)
    mine, theirs = got[well[q]], ref["hits"][well[ref_q]]
    assert mine.tobytes() == theirs.tobytes(), f"{what}: the {'sorted' if sorted_ else 'host-sorted'} slices of the well-conditioned queries differ from the brute force"


_REF = {}


def radius_reference(pkg, name):
    """(points, brute force) per mesh, computed once and shared with tests/test_gpu_radius.py; the points are the point-query tests' generator's"""
    if name not in _REF:
        tris = mesh(pkg, name)
        pts = make_points(pkg, tris, 512, 11 + len(tris))
        _REF[name] = (pts, radius_brute_force(pkg, pts, tris))
    return _REF[name]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_radius_search_and_the_flag():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    assert re.search(r"#define\s+BVH_RADIUS_SORTED\s+1u", text)
    assert re.search(r"\bint\s+bvh_radius_search\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*const bvh_result\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,\s*"
                     r"const bvh_point_query\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*bvh_knn_hit\s*\*\s*\w+\s*,\s*"
                     r"uint64_t\s+\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text
    assert "bvh_radius_search" in open(os.path.join(ROOT, "include", "bvh", "types.h")).read().split("#ifndef")[0]     # bvh_knn_hit's second user


def test_library_exports_radius_search(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_radius_search") and "bvh_radius_search" in pkg.EXPORTS
    assert pkg.RADIUS_SORTED == RADIUS_SORTED and pkg.KNN_HIT == KNN_HIT and pkg.KNN_HIT.itemsize == 8
    assert pkg.lib().bvh_abi_version() == 4


def test_radius_search_errors_without_a_device(pkg):
    lib = pkg.lib()
    assert lib.bvh_radius_search(None, None, None, None, 0, 0, None, None, 0, None) == E_INVALID
    r = pkg.Result(); r.n_leaves = 4; r.layout = 0; r.d_nodes = 64; r.d_tris = 64
    assert lib.bvh_radius_search(None, C.byref(r), None, 256, 4, RADIUS_SORTED, 4096, 8192, 16, None) == E_INVALID
    for flags in (2, 3, 0x80000000):                                     # (a bad flag bit on a live ctx: tests/test_gpu_radius.py)
        assert lib.bvh_radius_search(None, C.byref(r), None, 256, 4, flags, 4096, 8192, 16, None) == E_INVALID


def test_builder_classes_have_radius_search(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "radius_search"))
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().radius_search(np.zeros(4, dtype=pkg.POINT_QUERY))    # no tree yet


def test_cpp_mirror_radius_search_compiles(tmp_path):
    src = tmp_path / "radius_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> uint64_t ask(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_point_query* q, uint32_t n, uint32_t* off, bvh_knn_hit* h, uint64_t cap) {
    B bvh; bvh.build(ctx, a);
    uint64_t counted = 0, total = 0;
    bvh.radiusSearch(ctx, q, n, 0u, off, h, cap);
    bvh.radiusSearch(ctx, q, n, BVH_RADIUS_SORTED, off, nullptr, 0, &counted);
    bvh.radiusSearch(ctx, q, n, BVH_RADIUS_SORTED, off, h, cap, &total);
    return counted + total;
}
uint64_t all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_point_query* q, uint32_t n, uint32_t* off, bvh_knn_hit* h, uint64_t cap) {
    return ask<BvhConstruction::TwoPassLbvh>(ctx, a, q, n, off, h, cap) + ask<BvhConstruction::SinglePassLbvh>(ctx, a, q, n, off, h, cap) +
           ask<BvhConstruction::PLOCNew>(ctx, a, q, n, off, h, cap) + ask<BvhConstruction::HPLOC>(ctx, a, q, n, off, h, cap);
}
static_assert(BVH_RADIUS_SORTED == 1u && sizeof(bvh_knn_hit) == 8, "flag and record");
""")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the brute force and the checker ---------------------------------------------------------------------------------------------------------------------

def slices(bf):
    o = bf["offsets"]
    return [bf["hits"]["prim"][o[i]:o[i + 1]].tolist() for i in range(len(o) - 1)]


def test_slabs_with_exact_ties_are_ordered_by_prim(pkg):
    # test_knn's parallel slabs: prims 0 and 1 coincide at z = 2, prim 2 at z = 1, prim 3 at z = 3
    tri = slabs(pkg, (2.0, 2.0, 1.0, 3.0))
    pts = np.zeros(5, dtype=pkg.POINT_QUERY)
    pts["point"] = (0.25, 0.25, 0.0); pts["radius"] = np.inf
    pts["point"][1] = (0.25, 0.25, 2.5)                              # dist2 0.25 to prims 0, 1 and 3; 2.25 to prim 2
    pts["radius"][2] = 2.0                                          # r2 4: prims 2 (1) and 0, 1 (4 <= 4) accepted, prim 3 (9) not
    pts["radius"][3] = np.nextafter(F32(2.0), F32(0.0))             # r2 < 4: only prim 2
    pts["radius"][4] = 0.5                                          # nothing within 0.5
    bf = radius_brute_force(pkg, pts, tri)
    assert slices(bf) == [[2, 0, 1, 3], [0, 1, 3, 2], [2, 0, 1], [2], []]
    assert bf["offsets"].tolist() == [0, 4, 8, 11, 12, 12] and bf["offsets"].dtype == np.uint32
    assert bf["hits"]["dist2"].tolist() == [1.0, 4.0, 4.0, 9.0, 0.25, 0.25, 0.25, 2.25, 1.0, 4.0, 4.0, 1.0]
    assert bf["tie"].tolist() == [True, True, True, False, False] and bf["well"].all() and bf["counts"].tolist() == [4, 4, 3, 1, 0]
    check_radius(pts, tri, bf, bf["offsets"], bf["hits"], True)
    rev = bf["hits"].copy()
    for i in range(5):
        a, b = bf["offsets"][i], bf["offsets"][i + 1]
        rev[a:b] = bf["hits"][a:b][::-1]
    check_radius(pts, tri, bf, bf["offsets"], rev, False)             # unsorted slices are compared as sets
    assert host_sort(bf["offsets"], rev).tobytes() == bf["hits"].tobytes()


def test_radius_zero_on_a_shared_vertex_finds_every_incident_triangle(pkg):
    f = 6
    ang = np.linspace(0, 2 * np.pi, f + 1)
    tri = np.zeros(f + 1, dtype=pkg.meshgen.TRIANGLE)
    for i in range(f):
        tri["v1"][i] = (np.cos(ang[i]), np.sin(ang[i]), 0.0); tri["v2"][i] = (0, 0, 0); tri["v3"][i] = (np.cos(ang[i + 1]), np.sin(ang[i + 1]), 0.0)
    tri["v1"][f] = (5, 5, 5); tri["v2"][f] = (6, 5, 5); tri["v3"][f] = (5, 6, 5)        # away from the fan
    pts = np.zeros(3, dtype=pkg.POINT_QUERY)
    pts["radius"] = (0.0, -0.0, np.inf)
    bf = radius_brute_force(pkg, pts, tri)
    assert slices(bf) == [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6]]      # dist2 0 <= r2 0 is accepted; -0.0 is a radius of 0
    assert (bf["hits"]["dist2"][:12] == 0).all() and bf["tie"].all() and bf["well"].all()
    check_radius(pts, tri, bf, bf["offsets"], bf["hits"], True)


def test_dead_queries_and_nan_triangles_accept_nothing(pkg):
    tri = slabs(pkg, (1.0, 2.0, 3.0))
    tri["v2"][1, 0] = np.nan                                        # a NaN vertex: dist2 is NaN, never accepted, not even by an infinite radius
    pts = np.zeros(8, dtype=pkg.POINT_QUERY)
    pts["point"] = (0.25, 0.25, 0.0)
    pts["radius"] = (np.inf, -1.0, -np.inf, np.nan, -0.0, 10.0, np.inf, np.inf)
    pts["point"][6] = (np.nan, 0.25, 0.0); pts["point"][7] = (0.25, 0.25, np.nan)
    bf = radius_brute_force(pkg, pts, tri)
    assert slices(bf) == [[0, 2], [], [], [], [], [0, 2], [], []]
    assert bf["offsets"].tolist() == [0, 2, 2, 2, 2, 2, 4, 4, 4] and bf["well"].all() and not bf["tie"].any()
    check_radius(pts, tri, bf, bf["offsets"], bf["hits"], True)
    with pytest.raises(AssertionError):                             # a record of a dead query is no accepted candidate
        off = bf["offsets"].copy(); off[2:] += 1
        check_radius(pts, tri, bf, off, np.insert(bf["hits"], 2, bf["hits"][0]), True)


def test_point_clouds_as_degenerate_triangles(pkg):
    """v1 == v2 == v3: region A answers, dist2 is the plain f32 (dx*dx + dy*dy) + dz*dz of point sets, ties by index"""
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-2, 2, (500, 3)).astype(F32)
    cloud[100] = cloud[7]                                           # a duplicate point: an exact tie
    tri = np.zeros(len(cloud), dtype=pkg.meshgen.TRIANGLE)
    tri["v1"] = tri["v2"] = tri["v3"] = cloud
    q = rng.uniform(-2, 2, (64, 3)).astype(F32); q[0] = cloud[7]
    pts = np.zeros(len(q), dtype=pkg.POINT_QUERY); pts["point"] = q; pts["radius"] = 0.75
    bf = radius_brute_force(pkg, pts, tri)
    d = cloud[None] - q[:, None]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == F32
    r2 = F32(0.75) * F32(0.75)
    want = []
    for i in range(len(q)):
        inside = np.nonzero(d2[i] <= r2)[0]
        want.append(inside[np.lexsort((inside, d2[i][inside]))].tolist())
    assert slices(bf) == want and bf["counts"].min() >= 1 and bf["counts"].max() > 8
    assert want[0][:2] == [7, 100] and bf["tie"][0] and bf["well"].all()
    assert bf["hits"]["dist2"].tobytes() == np.concatenate([d2[i][w] for i, w in enumerate(want)]).tobytes()
    check_radius(pts, tri, bf, bf["offsets"], bf["hits"], True)


def test_checker_catches_tampered_slices(pkg):
    tri = slabs(pkg, (1.0, 2.0, 2.0, 3.0, 5.0))
    pts = np.zeros(3, dtype=pkg.POINT_QUERY)
    pts["point"] = (0.25, 0.25, 0.0); pts["radius"] = (np.inf, 2.5, np.inf)
    bf = radius_brute_force(pkg, pts, tri)
    off, ref = bf["offsets"], bf["hits"]
    assert slices(bf) == [[0, 1, 2, 3, 4], [0, 1, 2], [0, 1, 2, 3, 4]] and off.tolist() == [0, 5, 8, 13]
    check_radius(pts, tri, bf, off, ref, True); check_radius(pts, tri, bf, off, ref, False)

    def shifted(at, by):
        o = off.astype(np.int64); o[at:] += by
        return o.astype(np.uint32)
    swapped = ref.copy(); swapped[[1, 2]] = ref[[2, 1]]                 # the tie (dist2 4, prims 1 and 2) in the wrong order
    far = ref.copy(); far[[0, 4]] = ref[[4, 0]]
    flipped = ref.copy(); flipped["dist2"].view(np.uint32)[6] ^= 1      # one mantissa bit
    foreign = ref.copy(); foreign["prim"][5] = 3                        # a record whose dist2 belongs to another prim
    outside = np.insert(ref, 8, ref[3])                                 # prim 3 (dist2 9) in the slice of radius 2.5
    cases = {
        "a dropped record": (shifted(1, -1), np.delete(ref, 3), (True, False)),
        "a dropped slice": (shifted(2, -3), np.delete(ref, [5, 6, 7]), (True, False)),
        "a duplicated record": (shifted(1, 1), np.insert(ref, 2, ref[1]), (True, False)),
        "a record twice in place of another": (off, np.concatenate([ref[:3], ref[2:3], ref[4:]]), (True, False)),
        "a tie out of order": (off, swapped, (True,)),
        "records out of order": (off, far, (True,)),
        "a flipped dist2 bit": (off, flipped, (True, False)),
        "a foreign prim": (off, foreign, (True, False)),
        "a record beyond the radius": (shifted(2, 1), outside, (True, False)),
        "a prim out of range": (off, np.concatenate([ref[:12], np.array([(25.0, 77)], dtype=ref.dtype)]), (True, False)),
        "offsets that do not end at the total": (shifted(3, 1), ref, (True, False)),
        "offsets that do not start at 0": (shifted(0, 1), ref, (True, False)),
    }
    for what, (o, h, modes) in cases.items():
        for sorted_ in modes:
            with pytest.raises(AssertionError):
                check_radius(pts, tri, bf, o, h, sorted_, what)
    check_radius(pts, tri, bf, off, swapped, False); check_radius(pts, tri, bf, off, far, False)      # order is not checked on an unsorted answer
    # a query that is not well-conditioned may miss records, but still must not invent, repeat or misorder any
    loose = dict(bf); loose["well"] = np.array([False, True, True])
    check_radius(pts, tri, loose, shifted(1, -1), np.delete(ref, 3), True)
    with pytest.raises(AssertionError):
        check_radius(pts, tri, loose, off, swapped, True)
    with pytest.raises(AssertionError):
        check_radius(pts, tri, loose, off, flipped, True)


# ---- the GPU tests' inputs, by the brute force alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", RADIUS_MESHES)
def test_inputs_are_well_conditioned_and_cover_the_cases(pkg, name):
    n = len(mesh(pkg, name))
    pts, bf = radius_reference(pkg, name)
    c = bf["counts"]
    assert bf["well"].all(), f"{name}: {np.count_nonzero(~bf['well'])} of {len(pts)} queries are not well-conditioned"
    empty, full = int((c == 0).sum()), int((c == n).sum())
    partial = int(((c > 0) & (c < n)).sum())
    print(f"{name}: n {n}, empty {empty}, full {full}, partial {partial}, longest {int(c.max())}, ties {int(bf['tie'].sum())}, total {int(c.sum())}")
    assert empty >= 100 and full >= 100 and partial >= 150, (name, empty, full, partial)
    if n >= 63:
        assert (c > 32).sum() >= 100, f"{name}: no slices beyond bvh_knn's cap"
    if name.startswith("cornell"):
        assert bf["tie"].sum() >= 200, (name, int(bf["tie"].sum()))
    check_radius(pts, mesh(pkg, name), bf, bf["offsets"], bf["hits"], True, name)
