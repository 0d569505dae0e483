"""CPU: bvh_scene_winding_prepare / bvh_scene_winding_number in the C ABI, the library and the Python binding, and the numpy restatements that the GPU tests
(tests/test_gpu_scene_winding.py) compare against, built on tests/test_winding.py's helpers: the f64 brute force over world triangles
(scene_winding_brute_force), the per-instance maps, instance moments and top-level moments operation for operation (scene_maps_host, scene_moments_host) and
the two-level walk with its opening decisions in f32 and its terms and sum in a chosen precision (scene_walk_host) — each checked here on the CPU oracle's
trees under hand-made top-level trees."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_point_query import E_INVALID, point_brute_force, tri_arrays
from test_scene import identity, instance_inverse, make_instances, mat34, rot, world_box, xf_points
from test_scene_point import flat_world_tris, shear_matrix, world_triangles
from test_winding import FOURPI32, THIRD32, _comps, _cross, _dot, leaf_sum, leaf_terms, moments_host, tree_arrays, walk_host, winding_brute_force

F32 = np.float32
F64 = np.float64
KEEP_BLAS = 1


# ---- the numpy restatements ---------------------------------------------------------------------------------------------------------------------------------

def scene_active(inst, n_blas):
    _, active = instance_inverse(inst["object_to_world"])
    return active & (inst["blas"] < n_blas)


def scene_winding_brute_force(pkg, blas_tris, inst, pts):
    """the exact value: per point, the f64 sum of the solid angles of the WORLD triangles (f32 vertices mapped in f32, in the header's order) of every active
    instance, over 4 pi"""
    pts = np.asarray(pts, dtype=F32)
    out = np.zeros(len(pts), dtype=F64)
    for k in np.nonzero(scene_active(inst, len(blas_tris)))[0]:
        V1, V2, V3 = world_triangles(inst["object_to_world"][k], blas_tris[int(inst["blas"][k])])
        out += leaf_sum(pts, V1, V2, V3, F64)
    out[np.isnan(pts).any(axis=1)] = np.nan
    return out


def scene_maps_host(pkg, inst, n_blas):
    """bvh_winding_map per instance: the cofactor matrix in f64 from the f32 entries, each rounded once; smax = (float)sqrt(lambda); all zero when inactive"""
    m = np.asarray(inst["object_to_world"], dtype=F32).reshape(-1, 12).astype(F64)
    a = {(i, j): m[:, 4 * i + j] for i in range(3) for j in range(3)}
    out = np.zeros(len(m), dtype=pkg.WINDING_MAP)
    with np.errstate(all="ignore"):
        c = [a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1], a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2], a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0],
             a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2], a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0], a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1],
             a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1], a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2], a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]]
        lam = np.zeros(len(m))
        for i in range(3):
            S = [np.abs((a[i, 0] * a[j, 0] + a[i, 1] * a[j, 1]) + a[i, 2] * a[j, 2]) for j in range(3)]
            lam = np.fmax(lam, (S[0] + S[1]) + S[2])
        out["c"] = np.stack(c, axis=1).astype(F32)
        out["smax"] = np.sqrt(lam).astype(F32)
    act = scene_active(inst, n_blas)
    out["c"][~act] = 0; out["smax"][~act] = 0
    return out, act


def map_area_vectors(cmat, A):
    """A_w.i = (C_i0 Ax + C_i1 Ay) + C_i2 Az in f32; cmat (9,), A (..., 3)"""
    cmat = np.asarray(cmat, dtype=F32); A = np.asarray(A, dtype=F32)
    with np.errstate(all="ignore"):
        return np.stack([(cmat[3 * i] * A[..., 0] + cmat[3 * i + 1] * A[..., 1]) + cmat[3 * i + 2] * A[..., 2] for i in range(3)], axis=-1)


def box_radius(lo, hi, p):
    """bvh_winding_prepare's r: the distance from p to the farthest corner of the box, a NaN side ignored; arrays (..., 3)"""
    lo, hi, p = (np.asarray(x, dtype=F32) for x in (lo, hi, p))
    with np.errstate(all="ignore"):
        e = np.fmax(np.abs(lo - p), np.abs(hi - p))
        return np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(F32)


def tree_moments(pkg, nodes, root, ni, leaf_sums):
    """moments_host's climb and finish on given leaf sums (n, 7) f32: internal sums left + right bottom-up, then p = M / area (the box centre when area is 0 or
    not finite) and r from the node's stored box"""
    total = 2 * ni + 1
    S = np.zeros((total, 7), dtype=F32)
    S[ni:] = leaf_sums
    left, right = nodes["left"][:ni].astype(np.int64), nodes["right"][:ni].astype(np.int64)
    order, stack = [], [int(root)]
    while stack:
        v = stack.pop()
        order.append(v)
        for ch in (int(left[v]), int(right[v])):
            if ch < ni:
                stack.append(ch)
    with np.errstate(all="ignore"):
        for v in reversed(order):
            S[v] = S[left[v]] + S[right[v]]
        lo, hi = nodes["min"][:ni].astype(F32), nodes["max"][:ni].astype(F32)
        area = S[:ni, 3]
        good = (area != 0) & np.isfinite(area)
        p = np.where(good[:, None], S[:ni, 4:7] / area[:, None], (lo + hi) * F32(0.5)).astype(F32)
    out = np.zeros(ni, dtype=pkg.WINDING_MOMENT)
    out["a"] = S[:ni, 0:3]; out["area"] = S[:ni, 3]; out["p"] = p; out["r"] = box_radius(lo, hi, p)
    return out


def scene_moments_host(pkg, blas, inst, top=None):
    """blas: [(nodes, leaves, layout, root, tris)] per BLAS; top: (nodes, leaves, layout, root) of the top-level tree (None with one instance).  Returns dict:
    blas (moments_host per BLAS), maps, active, wbox (n_inst, 6), inst (instance moments), top (top-level moments or an empty array)"""
    bm = [moments_host(pkg, nd, lv, lay, rt, tris) for nd, lv, lay, rt, tris in blas]
    maps, act = scene_maps_host(pkg, inst, len(blas))
    n_inst = len(inst)
    imom = np.zeros(n_inst, dtype=pkg.WINDING_MOMENT)
    wbox = np.zeros((n_inst, 6), dtype=F32); wbox[:, :3] = np.finfo(F32).max; wbox[:, 3:] = -np.finfo(F32).max
    with np.errstate(all="ignore"):
        for k in np.nonzero(act)[0]:
            b = int(inst["blas"][k]); nd, _, _, rt, _ = blas[b]
            R = bm[b][rt]
            M = inst["object_to_world"][k]
            wbox[k] = world_box(M, np.concatenate([nd["min"][rt], nd["max"][rt]]))
            imom["a"][k] = map_area_vectors(maps["c"][k], R["a"])
            imom["area"][k] = (maps["smax"][k] * maps["smax"][k]) * R["area"]
            imom["p"][k] = xf_points(M, R["p"])
            imom["r"][k] = box_radius(wbox[k, :3], wbox[k, 3:], imom["p"][k])
    tm = np.zeros(0, dtype=pkg.WINDING_MOMENT)
    if top is not None:
        tn, tl, tlay, troot = top
        n, ni, prims = tree_arrays(tn, tl, tlay)
        assert n == n_inst
        ok = prims < n_inst
        pr = np.where(ok, prims, 0)
        with np.errstate(all="ignore"):
            leaf = np.concatenate([imom["a"][pr], imom["area"][pr][:, None], imom["area"][pr][:, None] * imom["p"][pr]], axis=1).astype(F32)
        tm = tree_moments(pkg, tn, troot, ni, np.where(ok[:, None], leaf, F32(0.0)))
    return {"blas": bm, "maps": maps, "active": act, "wbox": wbox, "inst": imom, "top": tm}


def _far(A, P, R, q, beta, dtype):
    """the opening decision in f32 on records (A, P, R) seen from q (all row-aligned) and the dipole terms in ``dtype`` -> (far bool[m], term dtype[m])"""
    with np.errstate(all="ignore"):
        d = P - q
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        t = beta * R
        far = d2 > t * t
        fourpi = FOURPI32 if dtype == F32 else dtype(4.0 * np.pi)
        dd = _comps(P.astype(dtype) - q.astype(dtype), dtype)
        dd2 = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]
        term = (_dot(_comps(A, dtype), dd) / ((fourpi * dd2) * np.sqrt(dd2))).astype(dtype)
    return far, term


def _blas_walk(tree, mom, M, cmap, smax, pts, sel, beta, dtype, acc, visits):
    """instance walk for the points sel: the BLAS root opened, internal children by the world-mapped rule, leaf children the world-triangle term"""
    nodes, leaves, layout, root, tris = tree
    n, ni, prims = tree_arrays(nodes, leaves, layout)
    total = 2 * n - 1
    V1, V2, V3 = world_triangles(M, tris)
    left, right = nodes["left"][:ni].astype(np.int64), nodes["right"][:ni].astype(np.int64)
    with np.errstate(all="ignore"):
        Aw = map_area_vectors(cmap, mom["a"]); Pw = xf_points(M, mom["p"]); Rw = (F32(smax) * mom["r"]).astype(F32)
    pi = sel; nd = np.full(len(sel), int(root), dtype=np.int64)
    n_terms = 0
    while len(pi):
        if visits is not None:
            visits.append(nd.copy())
        nxt_p, nxt_n = [], []
        for side in (left, right):
            ch = side[nd]
            lf = (ch >= ni) & (ch < total)
            pr = prims[ch[lf] - ni]
            inr = pr < len(tris)
            if inr.any():
                s2 = pi[lf][inr]; pr = pr[inr]
                np.add.at(acc, s2, leaf_terms(pts[s2], V1[pr], V2[pr], V3[pr], dtype)); n_terms += len(s2)
            it = ch < ni
            c, qi = ch[it], pi[it]
            far, term = _far(Aw[c], Pw[c], Rw[c], pts[qi], beta, dtype)
            np.add.at(acc, qi[far], term[far]); n_terms += int(far.sum())
            nxt_p.append(qi[~far]); nxt_n.append(c[~far])
        pi, nd = np.concatenate(nxt_p), np.concatenate(nxt_n)
    return n_terms


def scene_walk_host(pkg, blas, inst, top, mom, pts, beta, dtype, stats=None):
    """bvh_scene_winding_number restated.  blas / top / mom as scene_moments_host takes and returns them.  The opening decisions are always in f32, the terms and
    the sum in ``dtype``.  With n_inst >= 2 the top-level root is opened; an internal top-level child follows the flat rule on its record; a leaf child is its
    instance's dipole iff approximated, otherwise the instance is entered.  beta = +inf opens everything: the plain sum over the world triangles, summed
    directly.  stats (a dict): 'terms' = the mean number of terms per live point, 'visits' = per entered instance the (instance, BLAS nodes opened) lists."""
    pts = np.ascontiguousarray(pts, dtype=F32)
    m = len(pts)
    live = ~np.isnan(pts).any(axis=1)
    acc = np.zeros(m, dtype=dtype)
    beta = F32(beta)
    act = mom["active"]
    n_inst = len(inst)
    if np.isinf(beta):
        n_terms = 0
        for k in np.nonzero(act)[0]:
            V1, V2, V3 = world_triangles(inst["object_to_world"][k], blas[int(inst["blas"][k])][4])
            acc += leaf_sum(pts, V1, V2, V3, dtype); n_terms += len(V1)
        if stats is not None:
            stats["terms"] = float(n_terms)
        acc[~live] = np.nan
        return acc
    n_terms = 0
    enter = [[] for _ in range(n_inst)]                              # per instance, the points that enter it
    if n_inst == 1:
        enter[0].append(np.nonzero(live)[0])
    else:
        tn, tl, tlay, troot = top
        _, tni, tprims = tree_arrays(tn, tl, tlay)
        ttotal = 2 * n_inst - 1
        left, right = tn["left"][:tni].astype(np.int64), tn["right"][:tni].astype(np.int64)
        T, I = mom["top"], mom["inst"]
        pi = np.nonzero(live)[0]; nd = np.full(len(pi), int(troot), dtype=np.int64)
        while len(pi):
            nxt_p, nxt_n = [], []
            for side in (left, right):
                ch = side[nd]
                lf = (ch >= tni) & (ch < ttotal)
                k = tprims[ch[lf] - tni]; qi = pi[lf]
                ok = k < n_inst
                k, qi = k[ok], qi[ok]
                ok = act[k]
                k, qi = k[ok], qi[ok]
                far, term = _far(I["a"][k].astype(F32), I["p"][k].astype(F32), I["r"][k].astype(F32), pts[qi], beta, dtype)
                np.add.at(acc, qi[far], term[far]); n_terms += int(far.sum())
                for kk in np.unique(k[~far]):
                    enter[int(kk)].append(qi[~far][k[~far] == kk])
                it = ch < tni
                c, qi = ch[it], pi[it]
                far, term = _far(T["a"][c].astype(F32), T["p"][c].astype(F32), T["r"][c].astype(F32), pts[qi], beta, dtype)
                np.add.at(acc, qi[far], term[far]); n_terms += int(far.sum())
                nxt_p.append(qi[~far]); nxt_n.append(c[~far])
            pi, nd = np.concatenate(nxt_p), np.concatenate(nxt_n)
    all_visits = []
    for k in range(n_inst):
        if not enter[k] or not act[k]:
            continue
        sel = np.concatenate(enter[k])
        if not len(sel):
            continue
        b = int(inst["blas"][k])
        visits = [] if stats is not None else None
        n_terms += _blas_walk(blas[b], mom["blas"][b], inst["object_to_world"][k], mom["maps"]["c"][k], mom["maps"]["smax"][k], pts, sel, beta, dtype, acc, visits)
        if visits is not None:
            all_visits.append((k, visits))
    if stats is not None:
        stats["terms"] = n_terms / max(int(live.sum()), 1)
        stats["visits"] = all_visits
    acc[~live] = np.nan
    return acc


def median_split_tlas(pkg, wbox):
    """a hand-made layout-0 top-level tree over the world boxes (median split of the box centres along the longest axis): what the CPU tests put where the GPU
    tests have a built one.  -> (nodes, None, 0, root)"""
    n = len(wbox); ni = n - 1
    nodes = np.zeros(2 * n - 1, dtype=pkg.BVH2_NODE)
    nodes["left"][ni:] = np.arange(n); nodes["right"][ni:] = pkg.INVALID
    nodes["min"][ni:] = wbox[:, :3]; nodes["max"][ni:] = wbox[:, 3:]
    cen = 0.5 * (wbox[:, :3].astype(F64) + wbox[:, 3:])
    nxt = [0]

    def build(idx):
        if len(idx) == 1:
            return ni + int(idx[0])
        v = nxt[0]; nxt[0] += 1
        c = cen[idx]
        ax = int(np.argmax(c.max(axis=0) - c.min(axis=0)))
        order = idx[np.argsort(c[:, ax], kind="stable")]
        l, r = build(order[: len(order) // 2]), build(order[len(order) // 2:])
        nodes["left"][v], nodes["right"][v] = l, r
        nodes["min"][v] = np.fmin(nodes["min"][l], nodes["min"][r]); nodes["max"][v] = np.fmax(nodes["max"][l], nodes["max"][r])
        return v
    root = build(np.arange(n))
    return nodes, None, 0, root


def scene_make_points(pkg, wtris, m, seed):
    """test_gpu_winding.make_points on the world triangles: points inside and outside the scene box, the first quarter near the surface (centroids jittered by
    1e-2 of the extent), the last 8 with a NaN coordinate"""
    rng = np.random.default_rng(seed)
    v1, v2, v3 = tri_arrays(wtris)
    v = np.concatenate([v1, v2, v3]).astype(F64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    p = lo - 0.5 * ext + rng.random((m, 3)) * 2.0 * ext
    k = m // 4
    t = rng.integers(0, len(wtris), size=k)
    p[:k] = ((v1[t].astype(F64) + v2[t]) + v3[t]) / 3.0 + rng.normal(0, 1e-2, (k, 3)) * ext
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    pts["point"] = p.astype(F32)
    pts["radius"] = np.inf
    for j, c in enumerate(range(m - 8, m)):
        pts["point"][c, j % 3] = np.nan
    return pts


def scene_conditioning(pkg, pts, wtris):
    """(distance to the world surface f64[m] (NaN for dead points), scene diagonal): the premise of every GPU input is that at least 0.95 of the points lie
    farther than 1e-4 x the diagonal from the surface"""
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(point_brute_force(pkg, pts, wtris)["closest"]["dist2"].astype(F64))
    dist[np.isnan(pts["point"]).any(axis=1)] = np.nan
    v = np.concatenate(tri_arrays(wtris)).astype(F64)
    return dist, float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


def transform_kinds(rng, t=(0.0, 0.0, 0.0)):
    """one of each kind the GPU tests mix: identity, rotation x uniform scale, non-uniform scale + shear, a reflection"""
    R = rot(int(rng.integers(3)), rng.uniform(0, 2 * np.pi)) @ rot(int(rng.integers(3)), rng.uniform(0, 2 * np.pi))
    return {"identity": mat34(np.eye(3), t), "similarity": mat34(rng.uniform(0.5, 2.0) * R, t), "shear": mat34(shear_matrix(rng), t),
            "mirror": mat34(R @ np.diag([-1.0, 1.0, 1.0]), t)}


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------------

FUNCS = ["bvh_scene_winding_prepare", "bvh_scene_winding_number", "bvh_scene_winding_moments", "bvh_scene_winding_instances"]


def test_header_declares_the_entry_points_and_the_flag(pkg):
    types = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh", "types.h")).read(), flags=re.S)
    assert re.search(r"typedef struct\s*\{\s*float c\[9\];\s*float smax;\s*uint32_t reserved\[6\];\s*\}\s*bvh_winding_map;", types)
    assert re.search(r"static_assert\(sizeof\(bvh_winding_map\) == 64", types)
    raw = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define\s+BVH_SCENE_WINDING_KEEP_BLAS\s+1u", text)
    assert re.search(r"\bint\s+bvh_scene_winding_prepare\s*\(\s*bvh_scene\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)", text)
    assert re.search(r"\bint\s+bvh_scene_winding_number\s*\(\s*bvh_scene\s*\*\s*\w+\s*,\s*const bvh_point_query\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*float\s+\w+\s*,\s*"
                     r"float\s*\*\s*\w+\s*\)", text)
    assert re.search(r"\bint\s+bvh_scene_winding_moments\s*\(\s*const bvh_scene\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*const bvh_winding_moment\s*\*\*\s*\w+\s*,\s*"
                     r"uint32_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"\bint\s+bvh_scene_winding_instances\s*\(\s*const bvh_scene\s*\*\s*\w+\s*,\s*const bvh_winding_moment\s*\*\*\s*\w+\s*,\s*"
                     r"const bvh_winding_map\s*\*\*\s*\w+\s*\)", text)
    assert "Flat trees only" not in raw
    assert "#define BVH_ABI_VERSION 4" in text                     # additive: no struct changed size, no signature changed


def test_library_exports_them_and_the_record_layout(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for name in FUNCS:
        assert hasattr(L, name) and name in pkg.EXPORTS, name
    dt = pkg.WINDING_MAP
    assert dt.itemsize == 64 and [dt.fields[k][1] for k in dt.names] == [0, 36, 40]
    assert pkg.SCENE_WINDING_KEEP_BLAS == KEEP_BLAS
    assert pkg.lib().bvh_abi_version() == 4


def test_errors_without_a_device(pkg):
    lib = pkg.lib()
    p, n = C.c_void_p(), C.c_uint32()
    assert lib.bvh_scene_winding_prepare(None, 0) == E_INVALID
    assert lib.bvh_scene_winding_prepare(None, KEEP_BLAS) == E_INVALID
    assert lib.bvh_scene_winding_number(None, 256, 4, 2.0, 8192) == E_INVALID
    assert lib.bvh_scene_winding_number(None, None, 0, 2.0, None) == E_INVALID
    assert lib.bvh_scene_winding_moments(None, 0, C.byref(p), C.byref(n)) == E_INVALID
    assert lib.bvh_scene_winding_instances(None, C.byref(p), C.byref(p)) == E_INVALID
    for name in ("winding_prepare", "winding_number", "signed_distance", "winding_moments", "winding_instances"):
        assert callable(getattr(pkg.Scene, name))


# ---- the maps -----------------------------------------------------------------------------------------------------------------------------------------------

def all_test_matrices():
    rng = np.random.default_rng(11)
    mats = []
    for _ in range(16):
        mats += list(transform_kinds(rng, rng.uniform(-3, 3, 3)).values())
    return np.array(mats, dtype=F32)


def test_cofactor_matrix_maps_area_vectors(pkg):
    mats = all_test_matrices()
    inst = make_instances(pkg, mats, [0] * len(mats))
    maps, act = scene_maps_host(pkg, inst, 1)
    assert act.all()
    rng = np.random.default_rng(2)
    for k in range(len(mats)):
        A = mats[k].astype(F64).reshape(3, 4)[:, :3]
        Cm = maps["c"][k].astype(F64).reshape(3, 3)
        assert np.abs(Cm - np.linalg.det(A) * np.linalg.inv(A).T).max() <= 1e-6 * np.abs(Cm).max()      # the cofactor matrix
        u, v = rng.normal(size=(50, 3)), rng.normal(size=(50, 3))
        lhs = np.cross(u @ A.T, v @ A.T); rhs = np.cross(u, v) @ Cm.T
        assert np.abs(lhs - rhs).max() <= 1e-5 * max(np.abs(lhs).max(), 1.0)
        got = map_area_vectors(maps["c"][k], np.cross(u, v).astype(F32))
        assert np.abs(got - rhs).max() <= 1e-5 * max(np.abs(rhs).max(), 1.0)


def test_smax_bounds_the_largest_singular_value(pkg):
    mats = all_test_matrices()
    inst = make_instances(pkg, mats, [0] * len(mats))
    maps, _ = scene_maps_host(pkg, inst, 1)
    for k in range(len(mats)):
        s = np.linalg.svd(mats[k].astype(F64).reshape(3, 4)[:, :3], compute_uv=False).max()
        assert maps["smax"][k] >= F32(s) or abs(float(maps["smax"][k]) - s) <= 1e-7 * s, (k, maps["smax"][k], s)
        assert float(maps["smax"][k]) <= np.sqrt(3.0) * s * (1 + 1e-6)                                    # Gershgorin: within sqrt(3)
    ident = make_instances(pkg, [identity()], [0])
    m1, _ = scene_maps_host(pkg, ident, 1)
    assert m1["smax"][0] == F32(1.0) and tuple(m1["c"][0]) == (1, 0, 0, 0, 1, 0, 0, 0, 1)
    dead = make_instances(pkg, [identity(), mat34(np.zeros((3, 3)), (1, 1, 1))], [5, 0])
    m2, act = scene_maps_host(pkg, dead, 1)
    assert not act.any() and not m2["c"].any() and not m2["smax"].any()


# ---- the brute force ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bunny(pkg):
    return pkg.meshgen.bunny_like(320)


def test_overlapping_closed_instances_count_and_a_reflection_subtracts(pkg, bunny):
    rng = np.random.default_rng(3)
    v = np.concatenate(tri_arrays(bunny)).astype(F64)
    cen, ext = v.mean(axis=0), v.max(axis=0) - v.min(axis=0)
    pts = (cen + rng.normal(size=(200, 3)) * 0.03 * ext).astype(F32)   # well inside every copy
    assert (np.abs(winding_brute_force(bunny, pts) - 1.0) <= 1e-6).all()

    def about_centre(A, t=(0.0, 0.0, 0.0)):                           # x -> A (x - cen) + cen + t
        A = np.asarray(A, dtype=F64)
        return mat34(A, cen - A @ cen + np.asarray(t))
    R = rot(2, 0.7) @ rot(0, 0.3)
    mats = [identity(), about_centre(1.1 * R), about_centre(np.diag([1.2, 0.9, 1.0]) @ R, 0.01 * ext)]
    for k in (1, 2, 3):
        w = scene_winding_brute_force(pkg, [bunny], make_instances(pkg, mats[:k], [0] * k), pts)
        assert np.abs(w - k).max() <= 1e-5, (k, np.abs(w - k).max())
    flip = about_centre(np.diag([-1.0, 1.0, 1.0]))
    mirror = make_instances(pkg, [flip], [0])
    assert np.abs(scene_winding_brute_force(pkg, [bunny], mirror, pts) + 1.0).max() <= 1e-5
    both = make_instances(pkg, [identity(), flip, identity(), mat34(np.zeros((3, 3)))], [0, 0, 9, 0])
    assert np.abs(scene_winding_brute_force(pkg, [bunny], both, pts)).max() <= 1e-5      # +1 - 1, the inactive two contribute nothing
    far = np.array([[30.0, 0, 0], [0, -40.0, 5]], dtype=F32)
    assert np.abs(scene_winding_brute_force(pkg, [bunny], both[:2], far)).max() <= 1e-6
    nanp = np.array([[np.nan, 0, 0]], dtype=F32)
    assert np.isnan(scene_winding_brute_force(pkg, [bunny], both, nanp)).all()


def test_open_mesh_under_shear_differs_between_world_and_object_evaluation(pkg, bunny):
    """why the scene form is stated on world triangles: the solid angle of a triangle is not invariant under a general 3x4 map, only the total over a closed
    surface is.  On an open mesh under a shear the world value and the object-space value (the flat function at W q) are different functions; on the closed
    mesh, and under a similarity on the open one, they agree."""
    half = bunny[:160]
    rng = np.random.default_rng(5)
    S = np.eye(3); S[0, 1] = 0.9; S[1, 2] = -0.6
    shear = make_instances(pkg, [mat34(np.diag([2.0, 0.5, 1.0]) @ S, (0.3, -0.2, 0.1))], [0])
    simil = make_instances(pkg, [mat34(1.7 * rot(1, 0.8) @ rot(2, -0.4), (0.3, -0.2, 0.1))], [0])
    obj_pts = (rng.normal(size=(300, 3)) * 0.5).astype(F32)
    for inst, open_differs in ((shear, True), (simil, False)):
        M = inst["object_to_world"][0]
        world_pts = xf_points(M, obj_pts)
        for mesh, closed in ((half, False), (bunny, True)):
            w_world = scene_winding_brute_force(pkg, [mesh], inst, world_pts)
            w_obj = winding_brute_force(mesh, obj_pts)
            diff = float(np.abs(w_world - w_obj).max())
            if closed or not open_differs:
                assert diff <= 2e-4, (closed, open_differs, diff)      # (up to the rounding of the mapped points)
            else:
                assert diff >= 0.05, diff


# ---- moments and walk on the CPU oracle's trees ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_scene(pkg, orc, bunny):
    """two BLASes (a layout-0 and a layout-1 tree of the oracle's) under 9 instances of every kind, one inactive, and a hand-made top-level tree"""
    meshes = [bunny, pkg.meshgen.uniform(65, 4)]
    blas = []
    for algo, tris in zip((1, 3), meshes):
        t = orc.build_tree(algo, tris)
        blas.append((t["nodes"], t["leaves"], t["layout"], t["root"], tris))
    rng = np.random.default_rng(8)
    mats, bl = [], []
    for k in range(8):
        t = np.array([k % 2, (k // 2) % 2, k // 4], dtype=F64) * 4.0 + rng.uniform(-0.3, 0.3, 3)
        mats.append(list(transform_kinds(rng, t).values())[k % 4]); bl.append(k % 2)
    mats.append(mat34(np.zeros((3, 3)), (1, 1, 1))); bl.append(0)
    inst = make_instances(pkg, mats, bl)
    pre = scene_moments_host(pkg, blas, inst)
    top = median_split_tlas(pkg, pre["wbox"])
    return meshes, blas, inst, top, scene_moments_host(pkg, blas, inst, top)


def test_tree_moments_is_moments_hosts_climb(pkg, small_scene):
    _, blas, _, _, mom = small_scene
    for (nodes, leaves, layout, root, tris), ref in zip(blas, mom["blas"]):
        n, ni, prims = tree_arrays(nodes, leaves, layout)
        v1, v2, v3 = (x[prims] for x in tri_arrays(tris))                 # the leaf sums, as moments_host makes them
        a, b, c = _comps(v1, F32), _comps(v2, F32), _comps(v3, F32)
        xx = _cross([b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)])
        A = [F32(0.5) * xx[k] for k in range(3)]
        area = np.sqrt((A[0] * A[0] + A[1] * A[1]) + A[2] * A[2])
        cen = [((a[k] + b[k]) + c[k]) * THIRD32 for k in range(3)]
        leaf = np.stack(A + [area] + [area * cen[k] for k in range(3)], axis=1).astype(F32)
        assert tree_moments(pkg, nodes, root, ni, leaf).tobytes() == ref.tobytes()


def test_instance_and_top_level_moments(pkg, small_scene):
    meshes, blas, inst, top, mom = small_scene
    act = mom["active"]
    assert list(act) == [True] * 8 + [False]
    assert not mom["inst"][8].tobytes().strip(b"\0") and not mom["maps"][8].tobytes().strip(b"\0")
    flat, ks, _ = flat_world_tris(pkg, meshes, inst)
    v1, v2, v3 = (x.astype(F64) for x in tri_arrays(flat))
    Aw = 0.5 * np.cross(v2 - v1, v3 - v1)
    for k in range(8):
        I = mom["inst"][k]
        # the mapped area vector is the sum of the world triangles' area vectors (closed or not), the centre lies in the world box, r reaches its corners
        assert np.abs(I["a"] - Aw[ks == k].sum(axis=0)).max() <= 1e-4 * max(np.abs(Aw[ks == k]).sum(), 1.0)
        wb = mom["wbox"][k]
        assert (I["p"] >= wb[:3] - 1e-5).all() and (I["p"] <= wb[3:] + 1e-5).all()
        corners = np.array([[wb[3 * ((c >> a) & 1) + a] for a in range(3)] for c in range(8)], dtype=F64)
        assert abs(np.linalg.norm(corners - I["p"], axis=1).max() - I["r"]) <= 1e-5 * I["r"]
        # the weight bounds the world area from above: smax^2 >= every singular-value product
        world_area = np.linalg.norm(Aw[ks == k], axis=1).sum()
        assert I["area"] >= world_area * (1 - 1e-5)
    tn, _, _, troot = top
    T = mom["top"]
    assert len(T) == 8
    assert np.abs(T["a"][troot] - mom["inst"]["a"].astype(F64).sum(axis=0)).max() <= 1e-4
    assert abs(T["area"][troot] - mom["inst"]["area"].astype(F64).sum()) <= 1e-4 * T["area"][troot]
    want = (mom["inst"]["area"].astype(F64)[:, None] * mom["inst"]["p"]).sum(axis=0) / mom["inst"]["area"].astype(F64).sum()
    assert np.abs(T["p"][troot] - want).max() <= 1e-4
    assert np.isfinite(T.view(F32)).all() and (T["r"] > 0).all()
    assert scene_moments_host(pkg, blas, inst, top)["top"].tobytes() == T.tobytes()        # the sums follow the tree


def test_scene_walk_host_against_the_brute_force(pkg, small_scene):
    meshes, blas, inst, top, mom = small_scene
    flat, _, _ = flat_world_tris(pkg, meshes, inst)
    pts = scene_make_points(pkg, flat, 400, 6)
    dist, diag = scene_conditioning(pkg, pts, flat)
    with np.errstate(invalid="ignore"):
        assert (dist > 1e-4 * diag).mean() >= 0.95
    xyz = pts["point"]
    bf = scene_winding_brute_force(pkg, meshes, inst, xyz)
    live = ~np.isnan(bf)
    assert live.sum() == len(pts) - 8
    assert np.abs(bf[live] - winding_brute_force(flat, xyz)[live]).max() <= 1e-12      # the flattened scene's flat brute force
    w_inf = scene_walk_host(pkg, blas, inst, top, mom, xyz, np.inf, F64)
    assert np.isnan(w_inf[~live]).all() and np.abs(w_inf[live] - bf[live]).max() <= 1e-12
    w_big = scene_walk_host(pkg, blas, inst, top, mom, xyz, 1e18, F64)
    assert np.abs(w_big[live] - bf[live]).max() <= 1e-12              # the level-by-level expansion with everything opened
    prev = None
    for beta in (2.0, 3.0, 4.0):
        st = {}
        w = scene_walk_host(pkg, blas, inst, top, mom, xyz, beta, F64, st)
        err = float(np.abs(w[live] - bf[live]).max())
        print(f"beta {beta}: max error {err:.4f}, mean terms {st['terms']:.1f} of {len(flat)}")
        assert st["terms"] < 0.5 * len(flat) and err <= 0.1
        assert prev is None or err <= prev * 1.05
        prev = err
    w32 = scene_walk_host(pkg, blas, inst, top, mom, xyz, 2.0, F32)
    w64 = scene_walk_host(pkg, blas, inst, top, mom, xyz, 2.0, F64)
    assert w32.dtype == F32 and np.abs(w32[live] - w64[live]).max() <= 1e-4


@pytest.mark.parametrize("b", [0, 1])
def test_one_identity_instance_is_the_flat_walk(pkg, small_scene, b):
    """one identity instance opens exactly the nodes bvh_winding_number opens on the BLAS and returns its values: C = I, smax = 1, M = I map every record onto
    itself"""
    meshes, blas, _, _, _ = small_scene
    nodes, leaves, layout, root, tris = blas[b]
    inst = make_instances(pkg, [identity()], [0])
    mom = scene_moments_host(pkg, [blas[b]], inst)
    pts = scene_make_points(pkg, tris, 300, 9)["point"]
    for beta in (2.0, 3.0):
        for dtype in (F32, F64):
            st, fl = {}, {}
            got = scene_walk_host(pkg, [blas[b]], inst, None, mom, pts, beta, dtype, st)
            ref = walk_host(nodes, leaves, layout, root, tris, mom["blas"][0], pts, beta, dtype, fl)
            live = ~np.isnan(ref)
            assert st["terms"] == fl["terms"]                          # the same opened set: the same number of terms
            assert np.abs(got[live].astype(F64) - ref[live]).max() <= (1e-14 if dtype == F64 else 0.0) and np.isnan(got[~live]).all()


def test_similarity_gives_the_flat_answer_at_the_mapped_point(pkg, small_scene):
    meshes, blas, _, _, _ = small_scene
    nodes, leaves, layout, root, tris = blas[0]
    rng = np.random.default_rng(12)
    M = transform_kinds(rng, (3.0, -2.0, 1.0))["similarity"]
    inst = make_instances(pkg, [M], [0])
    mom = scene_moments_host(pkg, [blas[0]], inst)
    obj = scene_make_points(pkg, tris, 300, 10)["point"][:-8]
    world = xf_points(M, obj)
    got = scene_walk_host(pkg, [blas[0]], inst, None, mom, world, 2.0, F64)
    ref = walk_host(nodes, leaves, layout, root, tris, mom["blas"][0], obj, 2.0, F64)
    # up to rounding: a point within rounding of an opening threshold may open another node, which moves the answer by that node's approximation error
    assert np.median(np.abs(got - ref)) <= 1e-5 and (np.abs(got - ref) <= 1e-4).mean() >= 0.98
