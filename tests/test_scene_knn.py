"""CPU: bvh_scene_knn in the C ABI, the library and the Python binding; the two-level numpy brute force (every query against every world triangle of every
active instance, the k smallest (dist2, instance, prim) among the accepted candidates) that the GPU tests (tests/test_gpu_scene_knn.py) compare against, with
the per-entry recomputation and the lexicographic "below" check they use on every query; and the GPU tests' inputs, made here so that their premises (at most
1 % of the queries ill-conditioned at k = 32, partial lists, ties at place k) are checked without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_point_query import make_points
from test_gpu_query import caterpillar
from test_gpu_refit import jitter, no_negzero
from test_gpu_scene import MESH_SIZES, scene_instances, world_tris
from test_gpu_scene_point import with_shear
from test_knn import r2_of, slabs
from test_point_query import E_INVALID, WELL_GROW, closest_formula, point_ok, tri_arrays
from test_scene import identity, make_instances, mat34, tris_root_box, world_box
from test_scene_point import (active_instances, instance_set, near_surface_points, object_points, scene_point_brute_force, scene_points, scene_s2,
                              world_triangles)

F32 = np.float32
F64 = np.float64
PAD64 = np.uint64(0xFFFFFFFFFFFFFFFF)
PAD32 = np.uint32(0xFFFFFFFF)


class CInstanceKnnHit(C.Structure):
    _fields_ = [("dist2", C.c_float), ("prim_idx", C.c_uint32), ("instance_idx", C.c_uint32), ("reserved", C.c_uint32)]


# ---- the brute force and the checkers -----------------------------------------------------------------------------------------------------------------------

def scene_knn_padding(pkg, points, k):
    """[m, k] unused slots: {r2, INVALID, INVALID, 0}"""
    hits = np.zeros((len(points), k), dtype=pkg.INSTANCE_KNN_HIT)
    hits["dist2"] = r2_of(points)[:, None]; hits["prim"] = pkg.INVALID; hits["instance"] = pkg.INVALID
    return hits


def _keys(pkg, hits):
    """(u64 (bits of dist2) << 32 | instance, u32 prim) per slot; an unused slot is above every entry.  For dist2 >= 0 comparing the u64 first and the prim on
    a tie is the contract's lexicographic (dist2, instance, prim) order"""
    valid = hits["prim"] != pkg.INVALID
    k64 = (np.ascontiguousarray(hits["dist2"]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | hits["instance"].astype(np.uint64)
    return np.where(valid, k64, PAD64), np.where(valid, hits["prim"], PAD32), valid


def scene_knn_brute_force(pkg, points, blas_tris, instances, k, root_boxes=None, chunk_elems=1 << 21):
    """every query against every world triangle of every active instance, each candidate evaluated exactly as scene_point_brute_force does (f32, the header's
    order).  Returns dict: hits (INSTANCE_KNN_HIT [m, k]: the min(k, accepted) accepted candidates with the smallest (dist2, instance, prim) in ascending
    order, then the padding), counts (u32 [m]), well (bool: every listed entry meets bvh_scene_closest_point's conditions (1) and (2) against its own dist2;
    entry_well [m, k] has it per slot), kth_tie (bool: the first excluded accepted candidate has exactly the k-th entry's dist2)."""
    n_blas = len(blas_tris)
    if root_boxes is None:
        root_boxes = [tris_root_box(t) for t in blas_tris]
    w, active = active_instances(instances, n_blas)
    s2 = scene_s2(w)
    m = len(points)
    r2 = r2_of(points)
    ok = point_ok(points)
    p = np.ascontiguousarray(points["point"], dtype=F32)
    hits = scene_knn_padding(pkg, points, k)
    counts = np.zeros(m, dtype=np.uint32); entry_well = np.ones((m, k), dtype=bool); kth_tie = np.zeros(m, dtype=bool)
    out = {"hits": hits, "counts": counts, "well": entry_well.all(axis=1), "entry_well": entry_well, "kth_tie": kth_tie}
    parts, col_inst, col_prim = [], [], []                            # the candidates in (instance, prim) order
    for i in np.nonzero(active)[0]:
        tris = blas_tris[int(instances["blas"][i])]
        V1, V2, V3 = world_triangles(instances["object_to_world"][i], tris)
        d2i = np.empty((m, len(tris)), dtype=F32)
        step = max(1, chunk_elems // max(len(tris), 1))
        for s in range(0, m, step):
            _, d2i[s:s + step], _, _, _ = closest_formula(p[s:s + step, None, :], V1[None], V2[None], V3[None])
        parts.append(d2i); col_inst.append(np.full(len(tris), i, dtype=np.uint32)); col_prim.append(np.arange(len(tris), dtype=np.uint32))
    if not parts or m == 0:
        return out
    d2 = np.concatenate(parts, axis=1); col_inst = np.concatenate(col_inst); col_prim = np.concatenate(col_prim)
    N = d2.shape[1]
    with np.errstate(invalid="ignore"):
        acc = (d2 <= r2[:, None]) & ok[:, None]                       # (a NaN dist2 is never accepted)
    # the column index ascends with (instance, prim), so (bits of dist2, column) sorts the accepted candidates in the contract's order
    key = np.where(acc, (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(N, dtype=np.uint64)[None], PAD64)
    kk = min(k, N)
    order = np.argsort(key, axis=1, kind="stable")[:, :min(kk + 1, N)]
    rows = np.arange(m)[:, None]
    sel = acc[rows, order]
    lst, lsel = order[:, :kk], sel[:, :kk]
    hits["dist2"][:, :kk] = np.where(lsel, d2[rows, lst], hits["dist2"][:, :kk])
    hits["prim"][:, :kk] = np.where(lsel, col_prim[lst], pkg.INVALID)
    hits["instance"][:, :kk] = np.where(lsel, col_inst[lst], pkg.INVALID)
    counts[:] = lsel.sum(axis=1)
    if N > kk:
        kth_tie[:] = sel[:, kk] & (d2[rows[:, 0], order[:, kk]] == d2[rows[:, 0], order[:, kk - 1]])
    qi, sj = np.nonzero(lsel)
    ci = lst[qi, sj]
    ei, ej, ed2 = col_inst[ci], col_prim[ci], d2[qi, ci].astype(F64)
    for i in np.unique(ei):
        e_sel = np.nonzero(ei == i)[0]
        idx, j = qi[e_sel], ej[e_sel]
        b = int(instances["blas"][i])
        v1, v2, v3 = tri_arrays(blas_tris[b])
        lo = np.minimum(np.minimum(v1[j], v2[j]), v3[j]).astype(F64); hi = np.maximum(np.maximum(v1[j], v2[j]), v3[j]).astype(F64)
        _, e = object_points(w[i], p[idx])
        W = w[i].astype(F64).reshape(3, 4)
        ps = p[idx].astype(F64) @ W[:, :3].T + W[:, 3]
        g = (WELL_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1) + 0.5 * e.astype(F64))[:, None]
        dd = np.maximum(np.maximum((lo - g) - ps, ps - (hi + g)), 0.0)
        c1 = F64(s2[i]) * (dd * dd).sum(axis=1) <= ed2[e_sel]
        wb = world_box(instances["object_to_world"][i], root_boxes[b]).astype(F64)
        gw = WELL_GROW * np.abs(wb).max()
        dw = np.maximum(np.maximum((wb[:3] - gw) - p[idx].astype(F64), p[idx].astype(F64) - (wb[3:] + gw)), 0.0)
        c2 = (dw * dw).sum(axis=1) <= ed2[e_sel]
        entry_well[idx, sj[e_sel]] = c1 & c2
    out["well"] = entry_well.all(axis=1)
    return out


def scene_knn_truncate(pkg, bf, k):
    """the brute force for a smaller k from one computed with a larger: the lists' first k slots"""
    big = bf["hits"]
    assert 1 <= k < big.shape[1]
    hits = np.ascontiguousarray(big[:, :k])
    nxt = big[:, k]
    return {"hits": hits, "counts": np.minimum(bf["counts"], k).astype(np.uint32), "well": bf["entry_well"][:, :k].all(axis=1),
            "entry_well": bf["entry_well"][:, :k], "kth_tie": (nxt["prim"] != pkg.INVALID) & (nxt["dist2"] == hits["dist2"][:, k - 1])}


def scene_knn_recompute(pkg, points, blas_tris, instances, hits, counts=None):
    """per query: the entries before the first unused slot are accepted candidates of their (instance, prim) — an active instance, a prim of its BLAS — with
    bit-equal dist2, strictly ascending in (dist2, instance, prim); every slot from there on is exactly the padding; reserved is 0 everywhere; counts (when
    given) is the number of entries"""
    _, active = active_instances(instances, len(blas_tris))
    m, k = hits.shape
    k64, k32, valid = _keys(pkg, hits)
    cnt = valid.sum(axis=1)
    good = (valid == (np.arange(k)[None] < cnt[:, None])).all(axis=1)                # the entries form a prefix
    r2 = r2_of(points)
    pad_ok = ~valid & (hits["dist2"].view(np.uint32) == r2.view(np.uint32)[:, None]) & (hits["instance"] == pkg.INVALID)
    good &= (valid | pad_ok).all(axis=1) & (hits["reserved"] == 0).all(axis=1)
    if counts is not None:
        good &= np.asarray(counts) == cnt
    qi, sj = np.nonzero(valid)
    ins, pr = hits["instance"][qi, sj], hits["prim"][qi, sj]
    entry_ok = np.zeros(len(qi), dtype=bool)
    ok = point_ok(points)
    for i in np.unique(ins):
        if i >= len(instances) or not active[i]:
            continue
        tris = blas_tris[int(instances["blas"][i])]
        e_sel = np.nonzero((ins == i) & (pr < len(tris)))[0]
        V1, V2, V3 = world_triangles(instances["object_to_world"][i], tris[pr[e_sel]])
        q = qi[e_sel]
        _, d2, _, _, _ = closest_formula(points["point"][q].astype(F32), V1, V2, V3)
        with np.errstate(invalid="ignore"):
            acc = (d2 <= r2[q]) & ok[q]
        entry_ok[e_sel] = acc & (d2.view(np.uint32) == hits["dist2"][q, sj[e_sel]].view(np.uint32))
    np.logical_and.at(good, qi, entry_ok)
    if k > 1:
        asc = (k64[:, 1:] > k64[:, :-1]) | ((k64[:, 1:] == k64[:, :-1]) & (k32[:, 1:] > k32[:, :-1]))
        good &= (asc | ~valid[:, 1:]).all(axis=1)
    return good


def scene_knn_below(pkg, got, ref):
    """lists lexicographically below the brute force's: at the first place where the two differ, got's (dist2, instance, prim) is the smaller (an unused slot
    counts as above every entry)"""
    g64, g32, _ = _keys(pkg, got)
    r64, r32, _ = _keys(pkg, ref)
    diff = (g64 != r64) | (g32 != r32)
    first = diff.argmax(axis=1)
    rows = np.arange(len(ref))
    a64, a32, b64, b32 = g64[rows, first], g32[rows, first], r64[rows, first], r32[rows, first]
    return diff.any(axis=1) & ((a64 < b64) | ((a64 == b64) & (a32 < b32)))


def flat_entries_well(pkg, points, tris, hits):
    """bvh_knn's condition on every listed entry of a one-identity-instance scene's lists: the f64 squared distance from the point to the
    triangle's box grown by 2^-17 * (its largest |coordinate|) is <= the entry's dist2"""
    v1, v2, v3 = tri_arrays(tris)
    valid = hits["prim"] != pkg.INVALID
    j = np.where(valid, hits["prim"], 0)
    lo = np.minimum(np.minimum(v1[j], v2[j]), v3[j]).astype(F64); hi = np.maximum(np.maximum(v1[j], v2[j]), v3[j]).astype(F64)
    g = WELL_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=2, keepdims=True)
    pp = points["point"].astype(F64)[:, None, :]
    bd = np.maximum(np.maximum((lo - g) - pp, pp - (hi + g)), 0.0)
    return (~valid | ((bd * bd).sum(axis=2) <= hits["dist2"].astype(F64))).all(axis=1)


# ---- the GPU tests' inputs (tests/test_gpu_scene_knn.py), made here so that their premises are checked without a device ------------------------------------
EXACT_N_INST = [1, 2, 3, 64]
EXACT_KS = [1, 5, 8, 9, 32]
MAX_K = 32
_CACHE = {}


def cached(key, make):
    """references are computed once per session and shared (never modified) by the tests that need them"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def reference(pkg, pts, blas_tris, inst, k, at=MAX_K):
    """the brute force at k, cut from the one at `at`"""
    big = scene_knn_brute_force(pkg, pts, blas_tris, inst, at)
    return big if k == at else scene_knn_truncate(pkg, big, k)


def inactive_of(n_inst):
    return set() if n_inst < 3 else {n_inst - 1} if n_inst == 3 else {n_inst - 1, n_inst - 2, n_inst - 3}


def exact_inputs(pkg, n_inst, m=1024):
    """test_gpu_scene_point.test_exact_against_brute_force's recipe: four meshes, n_inst instances of every kind, every sixth sheared, the trailing ones
    inactive; m mixed points, a third with finite radii, a few dead.  Returns (meshes, inst, pts, the brute force at k = 32)"""
    def make():
        rng = np.random.default_rng(n_inst)
        meshes = [no_negzero(pkg.meshgen.uniform(n, 31 + n)) for n in MESH_SIZES[n_inst]]
        inst = with_shear(pkg, rng, scene_instances(pkg, rng, n_inst, 4, 1.5), n_inst - len(inactive_of(n_inst)))
        pts = scene_points(pkg, world_tris(pkg, meshes, inst), m, 100 + n_inst)
        return meshes, inst, pts, scene_knn_brute_force(pkg, pts, meshes, inst, MAX_K)
    return cached(("exact", n_inst, m), make)


def kinds_inputs(pkg, kind):
    """test_gpu_scene_point.test_anisotropic_and_far_offset_instances' recipe with a uniform(300) BLAS: 8 sheared or far-offset instances, unbounded queries"""
    def make():
        rng = np.random.default_rng(7 if kind == "shear" else 8)
        mesh = no_negzero(pkg.meshgen.uniform(300, 41))
        inst = instance_set(pkg, rng, kind, 8)
        pts = scene_points(pkg, world_tris(pkg, [mesh], inst), 1024, 9, bounded=False)
        return mesh, inst, pts, scene_knn_brute_force(pkg, pts, [mesh], inst, MAX_K)
    return cached(("kinds", kind), make)


def sponza_inputs(pkg):
    """Sponza-like 20 000 under one identity instance, 512 of test_gpu_point_query's mixed points (on vertices, edges and faces, near the surface, far; finite,
    zero, negative and NaN radii)"""
    def make():
        mesh = no_negzero(pkg.meshgen.sponza_like(20_000, 3))
        inst = make_instances(pkg, [identity()], [0])
        pts = make_points(pkg, mesh, 512, 8)
        return mesh, inst, pts, scene_knn_brute_force(pkg, pts, [mesh], inst, MAX_K)
    return cached(("sponza",), make)


def coincident_inputs(pkg, seed):
    """test_gpu_scene_point's tie setup: a mesh and the same mesh with a far-off extra triangle appended (it stretches that BLAS's world box, so the two
    instances are not walked alike), near-surface points"""
    def make():
        mesh = no_negzero(pkg.meshgen.uniform(120, 12))
        v = np.concatenate([mesh["v1"], mesh["v2"], mesh["v3"]])
        lo, hi = v.min(axis=0), v.max(axis=0)
        extra = np.zeros(1, dtype=pkg.meshgen.TRIANGLE)               # (appended: the prim indices of the shared triangles are the same in both BLASes)
        extra["v1"] = (hi[0] + 50, lo[1], lo[2] - 5); extra["v2"] = (hi[0] + 51, lo[1], lo[2] - 5); extra["v3"] = (hi[0] + 50, lo[1] + 1, lo[2] - 5)
        stretched = no_negzero(np.concatenate([mesh, extra]))
        pts = near_surface_points(pkg, mesh, 1024, np.random.default_rng(seed))
        inst = make_instances(pkg, [identity(), identity()], [0, 1])
        return mesh, stretched, inst, pts
    return cached(("coincident", seed), make)


def builders_inputs(pkg, k=16):
    """test_gpu_scene_point.test_independent_of_builders' recipe, cut to the queries that are well-conditioned at k: every list is then exact whatever built
    the trees.  Returns (mesh, inst, pts, the brute force at k, the fraction of the 1024 points kept)"""
    def make():
        rng = np.random.default_rng(9)
        mesh = no_negzero(pkg.meshgen.uniform(200, 77))
        inst = with_shear(pkg, rng, scene_instances(pkg, rng, 64, 1, 1.2), 61)
        pts = scene_points(pkg, world_tris(pkg, [mesh], inst), 1024, 5)
        well = scene_knn_brute_force(pkg, pts, [mesh], inst, k)["well"]
        pts = np.ascontiguousarray(pts[well])
        return mesh, inst, pts, scene_knn_brute_force(pkg, pts, [mesh], inst, k), well.mean()
    return cached(("builders", k), make)


DEEP_OFFSETS = [(0, 0, 0), (100, 0, 0), (0, 100, 0), (100, 100, 0), (200, 50, 0)]


def deep_inputs(pkg, H):
    """test_gpu_scene_point.test_deep_blas_takes_the_stackless_pass' recipe: test_gpu_query.caterpillar of height H under 5 translated instances and its 500
    points (below the faces, on the face at z = 0, with a radius that culls the far side, among the far triangles)"""
    def make():
        tris, nodes, root, n = caterpillar(pkg, H, 3 + H)
        offs = np.array(DEEP_OFFSETS, dtype=np.float64)
        inst = make_instances(pkg, [mat34(np.eye(3), t) for t in offs], [0] * len(offs))
        rng = np.random.default_rng(H)
        m = 500
        pts = np.zeros(m, dtype=pkg.POINT_QUERY)
        base = offs[rng.integers(0, len(offs), m)]
        pts["point"] = np.stack([base[:, 0] + rng.uniform(-1, 1, m), base[:, 1] + rng.uniform(-1, 1, m), rng.uniform(-3, -0.5, m)], axis=1)
        pts["point"][: m // 6, 2] = 0.0
        pts["radius"] = np.inf
        pts["radius"][m // 2: 3 * m // 4] = 5.0
        pts["point"][3 * m // 4:, 2] = rng.uniform(1000, 1000 + 2 * H, m - 3 * m // 4)
        return tris, nodes, root, n, inst, pts, scene_knn_brute_force(pkg, pts, [tris], inst, 8)
    return cached(("deep", H), make)


def moved_inputs(pkg):
    """test_gpu_scene_point.test_update_after_moves_and_blas_refit's recipe: two meshes, 64 instances as built and as moved (kinds and BLASes change too), the
    first mesh jittered for the refit"""
    def make():
        meshes = [no_negzero(pkg.meshgen.uniform(n, 5 + n)) for n in (150, 120)]
        inst = scene_instances(pkg, np.random.default_rng(21), 64, 2, 1.5)
        rng2 = np.random.default_rng(22)
        moved = with_shear(pkg, rng2, scene_instances(pkg, rng2, 64, 2, 1.7), 61)
        moved["blas"][:8] = 1 - np.minimum(moved["blas"][:8], 1)
        pts = scene_points(pkg, world_tris(pkg, meshes, moved), 1024, 23)
        refit = [jitter(meshes[0], 3, 2e-2), meshes[1]]
        return meshes, inst, moved, pts, refit, scene_knn_brute_force(pkg, pts, meshes, moved, MAX_K), scene_knn_brute_force(pkg, pts, refit, moved, MAX_K)
    return cached(("moved",), make)


def small_inputs(pkg):
    """the scene of the binding and hygiene tests: uniform(100) under an identity and a translated instance, 250 mixed points; the brute force at k = 5"""
    def make():
        mesh = no_negzero(pkg.meshgen.uniform(100, 3))
        inst = make_instances(pkg, [identity(), mat34(np.eye(3), (2.0, 0, 0))], [0, 0])
        pts = scene_points(pkg, world_tris(pkg, [mesh], inst), 250, 4)
        return mesh, inst, pts, scene_knn_brute_force(pkg, pts, [mesh], inst, MAX_K)
    return cached(("small",), make)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_type_and_the_entry_point(pkg):
    raw = open(os.path.join(ROOT, "include", "bvh", "types.h")).read()
    assert "bvh_instance_knn_hit 16 B" in raw.split("#ifndef")[0]                    # listed in the head comment
    types = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"typedef struct\s*\{\s*float dist2;\s*uint32_t prim_idx, instance_idx, reserved;\s*\}\s*bvh_instance_knn_hit;", types)
    assert re.search(r"static_assert\(sizeof\(bvh_instance_knn_hit\) == 16", types)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+bvh_scene_knn\s*\(\s*bvh_scene\s*\*\s*\w+\s*,\s*const bvh_point_query\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*"
                     r"bvh_instance_knn_hit\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text


def test_library_exports_the_symbol_and_sizes_match(pkg, tmp_path):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_scene_knn") and "bvh_scene_knn" in pkg.EXPORTS
    assert pkg.lib().bvh_abi_version() == 4
    assert pkg.INSTANCE_KNN_HIT.itemsize == 16 and C.sizeof(CInstanceKnnHit) == 16
    offs = [pkg.INSTANCE_KNN_HIT.fields[name][1] for name in pkg.INSTANCE_KNN_HIT.names]
    assert offs == [getattr(CInstanceKnnHit, f[0]).offset for f in CInstanceKnnHit._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "bvh_mi355x.h"\nint main(void) { printf("%zu", sizeof(bvh_instance_knn_hit)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["g++", "-std=c++17", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout == "16"


def test_binding_and_errors_without_a_device(pkg):
    assert callable(getattr(pkg.Scene, "knn"))
    L = pkg.lib()
    assert L.bvh_scene_knn(None, 16, 1, 1, 64, None) == E_INVALID
    assert L.bvh_scene_knn(None, None, 0, 1, None, None) == E_INVALID
    for k in (0, 33):
        assert L.bvh_scene_knn(None, 16, 1, k, 64, None) == E_INVALID


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------------------------------

def test_coincident_instances_interleave(pkg):
    """two coincident identity instances of three slabs at z = 1, 2, 3, queried from below: every dist2 comes twice, the lower instance first"""
    tri = slabs(pkg, (1.0, 2.0, 3.0))
    inst = make_instances(pkg, [identity(), identity()], [0, 0])
    pts = np.zeros(1, dtype=pkg.POINT_QUERY); pts["point"] = (0.25, 0.25, 0.0); pts["radius"] = np.inf
    INV = pkg.INVALID
    bf = scene_knn_brute_force(pkg, pts, [tri], inst, 4)
    h = bf["hits"][0]
    assert h["dist2"].tolist() == [1.0, 1.0, 4.0, 4.0] and h["instance"].tolist() == [0, 1, 0, 1] and h["prim"].tolist() == [0, 0, 1, 1]
    assert (h["reserved"] == 0).all() and bf["counts"].tolist() == [4] and bf["kth_tie"].tolist() == [False] and bf["well"].all()
    # the k-th and the (k + 1)-th candidate tie on dist2 and differ only by the instance: the lower instance stays
    bf3 = scene_knn_brute_force(pkg, pts, [tri], inst, 3)
    assert bf3["hits"]["instance"][0].tolist() == [0, 1, 0] and bf3["hits"]["prim"][0].tolist() == [0, 0, 1] and bf3["kth_tie"].tolist() == [True]
    bf1 = scene_knn_brute_force(pkg, pts, [tri], inst, 1)
    assert bf1["hits"]["instance"][0].tolist() == [0] and bf1["kth_tie"].tolist() == [True]
    # k larger than the number of candidates: a short list, then the padding
    bf8 = scene_knn_brute_force(pkg, pts, [tri], inst, 8)
    assert bf8["counts"].tolist() == [6] and bf8["hits"]["prim"][0].tolist() == [0, 0, 1, 1, 2, 2, INV, INV]
    assert bf8["hits"]["instance"][0].tolist() == [0, 1, 0, 1, 0, 1, INV, INV] and np.isinf(bf8["hits"]["dist2"][0, 6:]).all() and not bf8["kth_tie"].any()
    for kk, want in ((4, bf), (3, bf3), (1, bf1)):
        t = scene_knn_truncate(pkg, bf8, kk)
        assert all(t[f].tobytes() == want[f].tobytes() for f in ("hits", "counts", "well", "kth_tie")), kk
    for b in (bf, bf3, bf1, bf8):
        assert scene_knn_recompute(pkg, pts, [tri], inst, b["hits"], b["counts"]).all() and not scene_knn_below(pkg, b["hits"], b["hits"]).any()


def test_acceptance_boundary(pkg):
    """point-like triangles (v1 == v2 == v3) at dist2 exactly 1 and exactly the next float above 1 from the origin; radius 1: the first is in (dist2 == r2),
    the second is out"""
    tri = np.zeros(2, dtype=pkg.meshgen.TRIANGLE)
    for f in ("v1", "v2", "v3"):
        tri[f][0] = (0.0, 0.0, 1.0); tri[f][1] = (2.0 ** -12, 2.0 ** -12, 1.0)
    inst = make_instances(pkg, [identity()], [0])
    pts = np.zeros(2, dtype=pkg.POINT_QUERY); pts["radius"] = (np.inf, 1.0)
    bf = scene_knn_brute_force(pkg, pts, [tri], inst, 2)
    up = np.nextafter(F32(1.0), F32(2.0))
    assert bf["hits"]["dist2"][0].tolist() == [1.0, float(up)] and bf["hits"]["prim"][0].tolist() == [0, 1]
    assert bf["counts"].tolist() == [2, 1] and bf["hits"]["prim"][1].tolist() == [0, pkg.INVALID] and bf["hits"]["dist2"][1].tolist() == [1.0, 1.0]
    assert scene_knn_recompute(pkg, pts, [tri], inst, bf["hits"], bf["counts"]).all()
    over = bf["hits"].copy(); over[1, 1] = bf["hits"][0, 1]            # the candidate one float above r2, reported: not accepted
    assert scene_knn_recompute(pkg, pts, [tri], inst, over).tolist() == [True, False]


def test_dead_queries_and_inactive_instances(pkg):
    tri = pkg.meshgen.uniform(20, 3)
    inst = make_instances(pkg, [mat34(np.zeros((3, 3))), identity(), identity()], [0, 0, 7])
    pts = np.zeros(5, dtype=pkg.POINT_QUERY); pts["point"] = 0.5; pts["radius"] = (np.inf, -1.0, np.nan, 1e-6, np.inf)
    pts["point"][4, 1] = np.nan
    bf = scene_knn_brute_force(pkg, pts, [tri], inst, 3)
    h = bf["hits"]
    assert bf["counts"].tolist() == [3, 0, 0, 0, 0] and (h["instance"][0] == 1).all()               # instance 0 is singular, instance 2 has no BLAS
    assert (h["dist2"][1] == F32(1.0)).all() and np.isnan(h["dist2"][2]).all() and (h["dist2"][3] == F32(1e-6) * F32(1e-6)).all()
    assert (h["instance"][1:] == pkg.INVALID).all() and (h["prim"][1:] == pkg.INVALID).all() and (h["reserved"] == 0).all()
    assert scene_knn_recompute(pkg, pts, [tri], inst, h, bf["counts"]).all()
    for bad_inst in (0, 2, 9):                                        # an answer from an inactive or a missing instance
        bad = h.copy(); bad["instance"][0, 1] = bad_inst
        assert scene_knn_recompute(pkg, pts, [tri], inst, bad).tolist() == [False, True, True, True, True]


def test_recompute_and_below_catch_tampered_lists(pkg):
    tri = slabs(pkg, (1.0, 2.0, 3.0, 5.0))
    inst = make_instances(pkg, [identity(), mat34(np.eye(3), (0.0, 0.0, 0.5)), identity()], [0, 0, 0])   # instances 0 and 2 coincide
    pts = np.zeros(3, dtype=pkg.POINT_QUERY)
    pts["point"] = (0.25, 0.25, 0.0); pts["radius"] = (np.inf, 1.75, np.inf)
    bf = scene_knn_brute_force(pkg, pts, [tri], inst, 5)
    ref, cnt = bf["hits"], bf["counts"]
    INV = pkg.INVALID
    assert ref["dist2"][0].tolist() == [1.0, 1.0, 2.25, 4.0, 4.0] and ref["instance"][0].tolist() == [0, 2, 1, 0, 2] and ref["prim"][0].tolist() == [0, 0, 0, 1, 1]
    assert ref["instance"][1].tolist() == [0, 2, 1, INV, INV] and cnt.tolist() == [5, 3, 5]
    assert scene_knn_recompute(pkg, pts, [tri], inst, ref, cnt).all() and not scene_knn_below(pkg, ref, ref).any()

    def tampered(fn):
        h = ref.copy(); fn(h); return h
    hole = np.array((np.inf, INV, INV, 0), dtype=pkg.INSTANCE_KNN_HIT)
    cases = {
        "a swapped pair": tampered(lambda h: h.__setitem__((0, slice(2, 4)), ref[0, [3, 2]])),
        "a tie in the wrong instance order": tampered(lambda h: h["instance"].__setitem__((0, slice(0, 2)), (2, 0))),
        "a wrong instance for the dist2": tampered(lambda h: h["instance"].__setitem__((0, 0), 1)),
        "a wrong prim for the dist2": tampered(lambda h: h["prim"].__setitem__((0, 2), 1)),
        "dist2 one ulp off": tampered(lambda h: h["dist2"].__setitem__((0, 0), np.nextafter(F32(1.0), F32(2.0)))),
        "an entry twice": tampered(lambda h: h.__setitem__((0, 1), h[0, 0])),
        "a dropped entry (a hole)": tampered(lambda h: h.__setitem__((0, 1), hole)),
        "not accepted": tampered(lambda h: h.__setitem__((1, 3), ref[0, 3])),
        "padding dist2": tampered(lambda h: h["dist2"].__setitem__((1, 3), 0.0)),
        "padding instance": tampered(lambda h: h["instance"].__setitem__((1, 4), 0)),
        "reserved": tampered(lambda h: h["reserved"].__setitem__((0, 4), 1)),
        "prim out of range": tampered(lambda h: h["prim"].__setitem__((0, 4), 77)),
        "instance out of range": tampered(lambda h: h["instance"].__setitem__((0, 4), 3)),
    }
    for what, h in cases.items():
        good = scene_knn_recompute(pkg, pts, [tri], inst, h, cnt)
        assert not good[:2].all() and good[2], what
    # a dropped entry with the rest moved up: every entry is still a candidate in order, so the count gives it away, and the list is above the true one — what
    # only the comparison with the brute force (on well-conditioned queries) sees
    dropped = ref.copy(); dropped[0, 1:4] = ref[0, 2:5]; dropped[0, 4] = hole
    assert scene_knn_recompute(pkg, pts, [tri], inst, dropped, cnt).tolist() == [False, True, True]
    assert scene_knn_recompute(pkg, pts, [tri], inst, dropped).all() and not scene_knn_below(pkg, dropped, ref).any()
    assert dropped.tobytes() != ref.tobytes()
    wrong_counts = cnt.copy(); wrong_counts[1] = 4
    assert scene_knn_recompute(pkg, pts, [tri], inst, ref, wrong_counts).tolist() == [True, False, True]
    # below: a smaller key at the first difference
    lower = ref.copy(); lower["dist2"][0, 2] = 2.0
    assert scene_knn_below(pkg, lower, ref).tolist() == [True, False, False]
    lower = ref.copy(); lower["instance"][0, 1] = 1                                             # (1, 1, 0) < (1, 2, 0)
    assert scene_knn_below(pkg, lower, ref).tolist() == [True, False, False]
    lower = ref.copy(); lower["prim"][0, 4] = 0                                                 # (4, 2, 0) < (4, 2, 1)
    assert scene_knn_below(pkg, lower, ref).tolist() == [True, False, False]
    swapped = ref.copy(); swapped[0, 2:4] = ref[0, [3, 2]]                                        # (4, 0, 1) where the truth has (2.25, 1, 0): above
    assert not scene_knn_below(pkg, swapped, ref).any()
    extra = ref.copy(); extra[1, 3] = ref[0, 3]                                                 # an entry where the truth has none: below
    assert scene_knn_below(pkg, extra, ref).tolist() == [False, True, False]


# ---- against the existing brute force ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rigid", "aniso", "shear", "far"])
def test_k1_equals_the_closest_point_brute_force(pkg, kind):
    rng = np.random.default_rng({"rigid": 11, "aniso": 12, "shear": 13, "far": 14}[kind])
    meshes = [pkg.meshgen.uniform(60, 1), pkg.meshgen.uniform(45, 2)]
    inst = instance_set(pkg, rng, kind, 6, n_blas=2)
    inst = np.concatenate([inst, inst[:2]])                           # two coincident pairs: every answer on them ties on dist2
    inst["object_to_world"][3][5] = np.nan                          # and an inactive one
    pts = scene_points(pkg, world_tris(pkg, meshes, inst), 500, 15)
    big = scene_knn_brute_force(pkg, pts, meshes, inst, 4)
    one = scene_knn_brute_force(pkg, pts, meshes, inst, 1)
    cut = scene_knn_truncate(pkg, big, 1)
    assert all(cut[f].tobytes() == one[f].tobytes() for f in ("hits", "counts", "well", "kth_tie"))
    ref = scene_point_brute_force(pkg, pts, meshes, inst)
    c, h = ref["closest"], one["hits"][:, 0]
    assert ref["hit"].sum() > 200 and (~ref["hit"]).sum() > 20
    assert h["dist2"].tobytes() == c["dist2"].tobytes() and np.array_equal(h["prim"], c["prim"]) and np.array_equal(h["instance"], c["instance"])
    assert np.array_equal(one["counts"], ref["hit"].astype(np.uint32)) and np.array_equal(one["well"], ref["well"])
    assert scene_knn_recompute(pkg, pts, meshes, inst, big["hits"], big["counts"]).all()


# ---- the premises of the GPU tests ----------------------------------------------------------------------------------------------------------------------------
# The GPU tests may exclude at most 1 % of the queries as ill-conditioned: a condition on the inputs, asserted here at k = 32 with the generators and seeds the GPU
# tests use (a set that fails it gets other points, not another cap).

def _premises(pkg, what, bf, k):
    print(f"{what}: {bf['well'].sum()} of {len(bf['well'])} well-conditioned at k = {k}, {np.count_nonzero(bf['counts'] < k)} partial lists, "
          f"{bf['kth_tie'].sum()} ties at place k")
    assert bf["well"].mean() >= 0.99, f"{what}: only {bf['well'].mean():.4f} of the queries are well-conditioned at k = {k}"


@pytest.mark.parametrize("n_inst", EXACT_N_INST)
def test_exact_inputs(pkg, n_inst):
    meshes, inst, pts, bf = exact_inputs(pkg, n_inst)
    _premises(pkg, f"{n_inst} instances", bf, MAX_K)
    assert scene_knn_recompute(pkg, pts, meshes, inst, bf["hits"], bf["counts"]).all()
    assert not set(bf["hits"]["instance"][bf["hits"]["prim"] != pkg.INVALID].tolist()) & inactive_of(n_inst)
    for k in EXACT_KS:
        cut = bf if k == MAX_K else scene_knn_truncate(pkg, bf, k)
        partial = np.count_nonzero((cut["counts"] > 0) & (cut["counts"] < k))
        assert k == 1 or partial > 0, f"k = {k}: no partial list"
        assert (cut["counts"] == k).sum() > len(pts) // 2 and (cut["counts"] == 0).sum() > 20
        if n_inst == 64:                                              # (the identity instances of one BLAS coincide: 0, 20 and 40)
            assert cut["kth_tie"].sum() > 0, f"k = {k}: no list ends inside a tie"
    _, _, pts65, bf65 = exact_inputs(pkg, 3, m=65)                   # the partial last wave
    _premises(pkg, "65 points", bf65, MAX_K)


@pytest.mark.parametrize("kind", ["shear", "far"])
def test_kinds_inputs(pkg, kind):
    mesh, inst, pts, bf = kinds_inputs(pkg, kind)
    _premises(pkg, kind, bf, MAX_K)
    assert (bf["counts"] == MAX_K).all()


def test_sponza_inputs(pkg):
    mesh, inst, pts, bf = sponza_inputs(pkg)
    _premises(pkg, "sponza, one identity instance", bf, MAX_K)
    flat = flat_entries_well(pkg, pts, mesh, bf["hits"])
    assert (bf["well"] & flat).mean() >= 0.99
    cut = scene_knn_truncate(pkg, bf, 8)
    assert (cut["counts"] == 8).sum() > 200 and (cut["counts"] == 0).sum() > 20


@pytest.mark.parametrize("seed", [0, 3])
def test_coincident_inputs(pkg, seed):
    mesh, stretched, inst, pts = coincident_inputs(pkg, seed)
    for blas_tris in ([mesh, stretched], [stretched, mesh]):
        bf = scene_knn_brute_force(pkg, pts, blas_tris, inst, MAX_K)
        _premises(pkg, "coincident", bf, MAX_K)
        assert bf["well"].all()                                       # (the GPU test compares every list)
        h = scene_knn_truncate(pkg, bf, 6)["hits"]
        assert (h["instance"] == np.array([0, 1, 0, 1, 0, 1])[None]).all() and np.array_equal(h["prim"][:, 0::2], h["prim"][:, 1::2])
        assert np.array_equal(h["dist2"][:, 0::2], h["dist2"][:, 1::2])


def test_builders_moved_and_deep_inputs(pkg):
    mesh, inst, pts, bf, kept = builders_inputs(pkg)
    assert kept >= 0.99 and bf["well"].all() and (bf["counts"] == 16).sum() > 500
    meshes, _, moved, pts, refit, bf_moved, bf_refit = moved_inputs(pkg)
    _premises(pkg, "after update", bf_moved, MAX_K)
    _premises(pkg, "after BLAS refit", bf_refit, MAX_K)
    _premises(pkg, "hygiene", small_inputs(pkg)[3], MAX_K)
    for H in (70, 250):
        tris, nodes, root, n, inst, pts, bf8 = deep_inputs(pkg, H)
        assert bf8["well"].all() and (bf8["counts"] == 8).sum() > 250, f"caterpillar {H}: {bf8['well'].sum()} of {len(pts)} well-conditioned at k = 8"
