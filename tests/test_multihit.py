"""CPU: bvh_intersect_all in the C ABI, the library, the Python binding and the C++ mirror, and the numpy brute force (every ray against every triangle, ALL
accepted hits per ray in ascending (t, prim) order, compressed-row form) with the checker the GPU tests (tests/test_gpu_multihit.py) use."""
import ctypes as C
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT
from test_query import E_INVALID, F32, QUERY_GROW, accepted, brute_force, header_text, ray_ok, tri_formula, tri_vertices

HITS_SORTED = 1


def all_hits_brute_force(rays, tris, chunk_elems=1 << 22, workers=1):
    """every ray against every triangle.  Returns dict: offsets (u32[m + 1]) and hits (HIT records; ray i's slice hits[offsets[i]:offsets[i + 1]] holds ALL its
    accepted hits in ascending (t, prim) order), n_acc (accepted hits per ray), well (bool: every accepted hit of the ray meets DESIGN.md §8b's condition, as
    test_query.brute_force).  workers > 1 spreads the ray chunks over threads (numpy releases the GIL)."""
    from bvh_pkg import load
    pkg = load()
    v0, v1, v2 = tri_vertices(tris)
    n, m = len(tris), len(rays)
    lo = np.minimum(np.minimum(v0, v1), v2).astype(np.float64); hi = np.maximum(np.maximum(v0, v1), v2).astype(np.float64)
    g = 0.5 * QUERY_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True)
    glo, ghi = lo - g, hi + g
    ok = ray_ok(rays)
    step = max(1, chunk_elems // max(n, 1))

    tile = max(1, chunk_elems // step)                            # triangles per evaluation: a chunk of rays meets the mesh tile by tile

    def chunk(s):
        r = rays[s:s + step]
        o = np.ascontiguousarray(r["origin"], dtype=F32)[:, None, :]; d = np.ascontiguousarray(r["direction"], dtype=F32)[:, None, :]
        found = []
        for k in range(0, n, tile):
            it, iu, iv, iw = tri_formula(o, d, v0[None, k:k + tile], v1[None, k:k + tile], v2[None, k:k + tile])
            acc = accepted(it, iu, iv, iw, r["tmin"][:, None], r["tmax"][:, None]) & ok[s:s + step, None]
            ri, pi = np.nonzero(acc)
            found.append((ri, pi + k, it[ri, pi], iu[ri, pi], iv[ri, pi]))
        ri, pi, t, u, v = (np.concatenate([f[j] for f in found]) for j in range(5))
        order = np.lexsort((pi, t, ri))                           # by ray, then t, then prim
        ri, pi, t = ri[order], pi[order], t[order]
        rec = np.zeros(len(ri), dtype=pkg.HIT)
        rec["t"] = t; rec["u"] = u[order]; rec["v"] = v[order]; rec["prim"] = pi
        bad = np.zeros(len(r), dtype=bool)
        if ri.size:                                               # well-conditioned: every accepted hit's point (f64) inside its prim's box grown by half the kernel's growth
            p = r["origin"][ri].astype(np.float64) + t.astype(np.float64)[:, None] * r["direction"][ri].astype(np.float64)
            inside = ((p >= glo[pi]) & (p <= ghi[pi])).all(axis=1)
            np.logical_or.at(bad, ri, ~inside)
        return rec, np.bincount(ri, minlength=len(r)), ~bad

    starts = list(range(0, m, step))
    if workers > 1:
        with ThreadPoolExecutor(max_workers=workers) as ex:
            parts = list(ex.map(chunk, starts))
    else:
        parts = [chunk(s) for s in starts]
    n_acc = np.concatenate([p[1] for p in parts]).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)
    well = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, dtype=bool)
    hits = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, dtype=pkg.HIT)
    offsets = np.zeros(m + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(n_acc)
    return {"offsets": offsets, "hits": hits, "n_acc": n_acc, "well": well}


def slice_rays(offsets):
    """the ray index of every record of a compressed-row answer"""
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets.astype(np.int64)))


def host_sort(offsets, hits):
    """every slice in ascending (t, prim) order"""
    return hits[np.lexsort((hits["prim"], hits["t"], slice_rays(offsets)))]


def check_all_hits(rays, tris, ref, offsets, hits, sorted_, what=""):
    """the GPU tests' checker.  Every ray: the offsets are a scan from 0 up to len(hits); each record is an accepted hit of its primitive with bit-equal
    t / u / v; no primitive appears twice in a slice; each slice is a subset of the brute force's; a sorted answer is strictly ascending in (t, prim).
    Well-conditioned rays: the counts are equal (the offsets word for word up to the first ray that is not), a sorted fill is byte-equal to the brute force's
    slice and an unsorted one is after a host sort."""
    n, m = len(tris), len(rays)
    off = offsets.astype(np.int64)
    assert len(off) == m + 1 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(hits), f"{what}: offsets are not a scan of the slices"
    ray = slice_rays(offsets)
    prim = hits["prim"].astype(np.int64)
    assert (prim < n).all(), f"{what}: a primitive index out of range"
    v0, v1, v2 = tri_vertices(tris)
    r = rays[ray]
    it, iu, iv, iw = tri_formula(np.ascontiguousarray(r["origin"], dtype=F32), np.ascontiguousarray(r["direction"], dtype=F32), v0[prim], v1[prim], v2[prim])
    acc = accepted(it, iu, iv, iw, r["tmin"], r["tmax"]) & ray_ok(r)
    same = (it.view(np.uint32) == hits["t"].view(np.uint32)) & (iu.view(np.uint32) == hits["u"].view(np.uint32)) & (iv.view(np.uint32) == hits["v"].view(np.uint32))
    assert (acc & same).all(), f"{what}: {np.count_nonzero(~(acc & same))} records are not accepted hits of their prims with bit-equal t / u / v"
    key = ray * n + prim
    assert len(np.unique(key)) == len(key), f"{what}: a primitive appears twice in a slice"
    ref_key = slice_rays(ref["offsets"]) * n + ref["hits"]["prim"].astype(np.int64)
    assert np.isin(key, ref_key).all(), f"{what}: a slice is not a subset of the true set"
    if sorted_ and len(hits) > 1:
        nxt = ray[1:] == ray[:-1]
        t, p = hits["t"], hits["prim"]
        asc = (t[1:] > t[:-1]) | ((t[1:] == t[:-1]) & (p[1:] > p[:-1]))
        assert asc[nxt].all(), f"{what}: {np.count_nonzero(~asc & nxt)} slices are not strictly ascending in (t, prim)"
    well = ref["well"]
    counts, ref_counts = np.diff(off), np.diff(ref["offsets"].astype(np.int64))
    assert (counts == ref_counts)[well].all(), f"{what}: counts differ on {np.count_nonzero((counts != ref_counts) & well)} well-conditioned rays"
    first_bad = m if well.all() else int(np.argmin(well))
    assert offsets[: first_bad + 1].tobytes() == ref["offsets"][: first_bad + 1].tobytes(), f"{what}: offsets differ"
    got = hits if sorted_ else host_sort(offsets, hits)
    mine, theirs = got[well[ray]], ref["hits"][well[slice_rays(ref["offsets"])]]
    assert mine.tobytes() == theirs.tobytes(), f"{what}: the {'sorted' if sorted_ else 'host-sorted'} slices of the well-conditioned rays differ from the brute force"


def test_header_declares_intersect_all_and_the_flag():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert re.search(r"#define\s+BVH_HITS_SORTED\s+1u", text)
    assert re.search(r"\bint\s+bvh_intersect_all\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*const bvh_result\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,\s*"
                     r"const bvh_ray\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*bvh_hit\s*\*\s*\w+\s*,\s*"
                     r"uint64_t\s+\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text


def test_library_exports_intersect_all(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_intersect_all") and "bvh_intersect_all" in pkg.EXPORTS
    assert pkg.HITS_SORTED == HITS_SORTED and pkg.HIT.itemsize == 16


def test_intersect_all_errors_without_a_device(pkg):
    lib = pkg.lib()
    assert lib.bvh_intersect_all(None, None, None, None, 0, 0, None, None, 0, None) == E_INVALID
    r = pkg.Result(); r.n_leaves = 4; r.layout = 0; r.d_nodes = 64; r.d_tris = 64
    assert lib.bvh_intersect_all(None, C.byref(r), None, 256, 4, HITS_SORTED, 4096, 8192, 16, None) == E_INVALID
    for flags in (2, 3, 0x80000000):                                     # (a bad flag bit on a live ctx: tests/test_gpu_multihit.py)
        assert lib.bvh_intersect_all(None, C.byref(r), None, 256, 4, flags, 4096, 8192, 16, None) == E_INVALID


def test_builder_classes_have_intersect_all(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "intersect_all"))
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().intersect_all(np.zeros(4, dtype=pkg.RAY))            # no tree yet


def test_cpp_mirror_intersect_all_compiles(tmp_path):
    src = tmp_path / "multihit_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> uint64_t shoot(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_ray* r, uint32_t n, uint32_t* off, bvh_hit* h, uint64_t cap) {
    B bvh; bvh.build(ctx, a);
    bvh.intersectAllAsync(ctx, r, n, 0u, off, h, cap);
    return bvh.intersectAll(ctx, r, n, BVH_HITS_SORTED, off, nullptr, 0) + bvh.intersectAll(ctx, r, n, BVH_HITS_SORTED, off, h, cap);
}
uint64_t all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_ray* r, uint32_t n, uint32_t* off, bvh_hit* h, uint64_t cap) {
    return shoot<BvhConstruction::TwoPassLbvh>(ctx, a, r, n, off, h, cap) + shoot<BvhConstruction::SinglePassLbvh>(ctx, a, r, n, off, h, cap) +
           shoot<BvhConstruction::PLOCNew>(ctx, a, r, n, off, h, cap) + shoot<BvhConstruction::HPLOC>(ctx, a, r, n, off, h, cap);
}
static_assert(BVH_HITS_SORTED == 1u, "flag");
""")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def slab_stack(pkg):
    """43 parallel unit quads (86 triangles): z = 0 .. 39 plus duplicates at z = 7, 7 and 19 — exact-t ties between prims for rays along z"""
    zs = np.concatenate([np.arange(40), [7, 7, 19]]).astype(np.float32)
    tris = np.zeros(2 * len(zs), dtype=pkg.meshgen.TRIANGLE)
    for k, z in enumerate(zs):
        tris["v1"][2 * k] = (0, 0, z); tris["v2"][2 * k] = (1, 0, z); tris["v3"][2 * k] = (1, 1, z)
        tris["v1"][2 * k + 1] = (0, 0, z); tris["v2"][2 * k + 1] = (1, 1, z); tris["v3"][2 * k + 1] = (0, 1, z)
    return tris


def slab_rays(pkg, m=512, seed=11):
    """m rays from z = -1 along +z with small random tilts; the first quarter exactly axial, the last quarter with a random tmax in [1, 41]"""
    rng = np.random.default_rng(seed)
    rays = np.zeros(m, dtype=pkg.RAY)
    rays["origin"] = np.stack([rng.uniform(0.2, 0.8, m), rng.uniform(0.2, 0.8, m), np.full(m, -1.0)], axis=1)
    rays["direction"] = np.stack([rng.normal(0, 1e-3, m), rng.normal(0, 1e-3, m), np.ones(m)], axis=1)
    rays["direction"][: m // 4, :2] = 0.0
    rays["tmax"] = 1e30
    rays["tmax"][m - m // 4:] = rng.uniform(1.0, 41.0, m // 4)
    return rays


def small_scene(pkg):
    tris = pkg.meshgen.uniform(300, 4)
    rng = np.random.default_rng(2)
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    m = 400
    o = lo - 0.5 * (hi - lo) + rng.random((m, 3)) * 2.0 * (hi - lo)
    d = (lo + rng.random((m, 3)) * (hi - lo)) - o
    rays = np.zeros(m, dtype=pkg.RAY)
    rays["origin"] = o.astype(F32); rays["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    rays["tmax"] = 3.0e38
    rays["tmax"][:50] = rng.random(50) * 2.0
    rays["tmin"][50:60] = 5.0; rays["tmax"][50:60] = 5.0                 # empty windows
    rays["origin"][60, 1] = np.nan
    return tris, rays


def test_helper_agrees_with_the_closest_hit_brute_force(pkg):
    for tris, rays in (small_scene(pkg), (slab_stack(pkg), slab_rays(pkg))):
        ref, bf = all_hits_brute_force(rays, tris, chunk_elems=1 << 14), brute_force(rays, tris)
        assert (ref["n_acc"] == bf["n_acc"]).all() and (ref["well"] == bf["well"]).all()
        assert (np.diff(ref["offsets"].astype(np.int64)) == bf["n_acc"]).all() and ref["offsets"][0] == 0 and ref["offsets"][-1] == len(ref["hits"])
        has = bf["n_acc"] > 0
        assert (has == bf["hit"]).all() and has.any()
        first = ref["hits"][ref["offsets"][:-1][has]]
        assert first.tobytes() == bf["closest"][has].tobytes()
        check_all_hits(rays, tris, ref, ref["offsets"], ref["hits"], True, "the brute force itself")
        threaded = all_hits_brute_force(rays, tris, chunk_elems=1 << 14, workers=4)
        assert threaded["hits"].tobytes() == ref["hits"].tobytes() and threaded["offsets"].tobytes() == ref["offsets"].tobytes()


def test_slab_stack_inputs(pkg):
    """the CPU check of test_gpu_multihit's long-slice inputs: every ray well-conditioned, 1 .. 43 hits per ray, most rays carry all 43, ties ordered by prim"""
    tris, rays = slab_stack(pkg), slab_rays(pkg)
    assert len(tris) == 86 and len(rays) == 512
    assert (rays["direction"][:128, :2] == 0).all() and (rays["tmax"][384:] <= 41).all() and (rays["tmax"][:384] > 1e29).all()
    ref = all_hits_brute_force(rays, tris)
    assert ref["well"].all()
    assert ref["n_acc"].min() >= 1 and ref["n_acc"].max() == 43
    assert np.count_nonzero(ref["n_acc"] == 43) >= 384 - 64
    h, ray = ref["hits"], slice_rays(ref["offsets"])
    tie = (ray[1:] == ray[:-1]) & (h["t"][1:] == h["t"][:-1])
    assert np.count_nonzero(tie) >= 128 * 3 and (h["prim"][1:] > h["prim"][:-1])[tie].all()
    cut = ref["n_acc"][384:] < 43
    assert cut.any() and (h["t"] < rays["tmax"][ray]).all()


def test_checker_catches_tampered_slices(pkg):
    tris, rays = slab_stack(pkg), slab_rays(pkg, 64)
    ref = all_hits_brute_force(rays, tris)
    off, hits = ref["offsets"], ref["hits"]
    check_all_hits(rays, tris, ref, off, hits, True)
    shuffled = hits.copy()
    rng = np.random.default_rng(0)
    for i in range(len(rays)):
        s = shuffled[off[i]:off[i + 1]]; s[:] = s[rng.permutation(len(s))]
    check_all_hits(rays, tris, ref, off, shuffled, False)                # an unsorted answer is fine unsorted ...
    with pytest.raises(AssertionError):
        check_all_hits(rays, tris, ref, off, shuffled, True)             # ... and caught when it claims to be sorted
    a = int(off[5])
    swapped = hits.copy(); swapped[[a, a + 1]] = swapped[[a + 1, a]]
    with pytest.raises(AssertionError):
        check_all_hits(rays, tris, ref, off, swapped, True)
    tie = np.nonzero((slice_rays(off)[1:] == slice_rays(off)[:-1]) & (hits["t"][1:] == hits["t"][:-1]))[0][0]
    tied = hits.copy(); tied[[tie, tie + 1]] = tied[[tie + 1, tie]]      # equal t, prims in the wrong order
    with pytest.raises(AssertionError):
        check_all_hits(rays, tris, ref, off, tied, True)
    dropped = np.delete(hits, a + 2); off2 = off.copy(); off2[6:] -= 1
    for flag in (True, False):
        with pytest.raises(AssertionError):
            check_all_hits(rays, tris, ref, off2, dropped, flag)
    dup = hits.copy(); dup[a + 3] = dup[a + 2]
    for flag in (True, False):
        with pytest.raises(AssertionError):
            check_all_hits(rays, tris, ref, off, dup, flag)
    bit = hits.copy(); bit["t"].view(np.uint32)[a + 4] ^= 1
    for flag in (True, False):
        with pytest.raises(AssertionError):
            check_all_hits(rays, tris, ref, off, bit, flag)
    wrong_ray = hits.copy(); off3 = off.copy(); off3[6] += 1             # ray 6's first record handed to ray 5
    with pytest.raises(AssertionError):
        check_all_hits(rays, tris, ref, off3, wrong_ray, True)
