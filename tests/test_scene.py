"""CPU: instanced scenes (bvh_scene_*) and bvh_build_boxes in the C ABI, the library and the Python binding; the numpy restatement of the instance maths
(include/bvh_mi355x.h) and the two-level brute force the GPU scene tests (tests/test_gpu_scene.py) compare against."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_query import E_INVALID, QUERY_GROW, accepted, ray_ok, brute_force, tri_formula, tri_vertices

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def instance_inverse(m):
    """object_to_world (k, 12) float32 -> (world_to_object (k, 12) float32, active (k,) bool) in the header's operation order (k_instance_boxes)"""
    m = np.asarray(m, dtype=F32).reshape(-1, 12)
    a = m.astype(np.float64)
    a00, a01, a02, t0, a10, a11, a12, t1, a20, a21, a22, t2 = (a[:, j] for j in range(12))
    with np.errstate(all="ignore"):
        c00 = a11 * a22 - a12 * a21; c01 = a12 * a20 - a10 * a22; c02 = a10 * a21 - a11 * a20
        det = (a00 * c00 + a01 * c01) + a02 * c02
        i00, i01, i02 = c00 / det, (a02 * a21 - a01 * a22) / det, (a01 * a12 - a02 * a11) / det
        i10, i11, i12 = c01 / det, (a00 * a22 - a02 * a20) / det, (a02 * a10 - a00 * a12) / det
        i20, i21, i22 = c02 / det, (a01 * a20 - a00 * a21) / det, (a00 * a11 - a01 * a10) / det
        u0 = -((i00 * t0 + i01 * t1) + i02 * t2); u1 = -((i10 * t0 + i11 * t1) + i12 * t2); u2 = -((i20 * t0 + i21 * t1) + i22 * t2)
        w = np.stack([i00, i01, i02, u0, i10, i11, i12, u1, i20, i21, i22, u2], axis=1).astype(F32)
    active = np.isfinite(m).all(axis=1) & (det != 0) & np.isfinite(det) & np.isfinite(w).all(axis=1)
    return w, active


def xf_points(m, p):
    """f32 ((m0 x + m1 y) + m2 z) + m3 per row; m (12,), p (..., 3)"""
    m = np.asarray(m, dtype=F32); p = np.asarray(p, dtype=F32)
    with np.errstate(all="ignore"):
        return np.stack([((m[4 * i] * p[..., 0] + m[4 * i + 1] * p[..., 1]) + m[4 * i + 2] * p[..., 2]) + m[4 * i + 3] for i in range(3)], axis=-1)


def xf_dirs(m, d):
    m = np.asarray(m, dtype=F32); d = np.asarray(d, dtype=F32)
    with np.errstate(all="ignore"):
        return np.stack([(m[4 * i] * d[..., 0] + m[4 * i + 1] * d[..., 1]) + m[4 * i + 2] * d[..., 2] for i in range(3)], axis=-1)


def world_box(m, root_box):
    """fminf / fmaxf over the 8 mapped corners of root_box (min xyz, max xyz), corner 0 first"""
    lo, hi = np.asarray(root_box[:3], dtype=F32), np.asarray(root_box[3:], dtype=F32)
    corners = np.array([[hi[0] if c & 1 else lo[0], hi[1] if c & 2 else lo[1], hi[2] if c & 4 else lo[2]] for c in range(8)], dtype=F32)
    p = xf_points(m, corners)
    bmin, bmax = p[0].copy(), p[0].copy()
    for c in range(1, 8):
        bmin = np.fmin(bmin, p[c]); bmax = np.fmax(bmax, p[c])
    return np.concatenate([bmin, bmax])


def tris_root_box(tris):
    v0, v1, v2 = tri_vertices(tris)
    return np.concatenate([np.minimum(np.minimum(v0, v1), v2).min(axis=0), np.maximum(np.maximum(v0, v1), v2).max(axis=0)]).astype(F32)


def object_rays(rays, w):
    out = rays.copy()
    out["origin"] = xf_points(w, rays["origin"]); out["direction"] = xf_dirs(w, rays["direction"])
    return out


def make_instances(pkg, mats, blas):
    inst = np.zeros(len(mats), dtype=pkg.INSTANCE)
    inst["object_to_world"] = np.asarray(mats, dtype=F32).reshape(-1, 12); inst["blas"] = blas
    return inst


def identity():
    return np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=F32)


def scene_brute_force(pkg, rays, blas_tris, instances, root_boxes=None, chunk_elems=1 << 22):
    """every ray against every triangle of every active instance, in object space.  Returns dict: closest (INSTANCE_HIT: smallest (t, instance, prim)),
    hit, well (the object-space ray is well-conditioned for its BLAS and every accepted hit's world point lies in its instance's world box grown by g/2)."""
    n_blas = len(blas_tris)
    if root_boxes is None:
        root_boxes = [tris_root_box(t) for t in blas_tris]
    w, active = instance_inverse(instances["object_to_world"])
    active &= instances["blas"] < n_blas
    m = len(rays)
    out = np.zeros(m, dtype=pkg.INSTANCE_HIT)
    out["t"] = rays["tmax"]; out["prim"] = pkg.INVALID; out["instance"] = pkg.INVALID
    well = np.ones(m, dtype=bool)
    ok = ray_ok(rays)
    for k in np.nonzero(active)[0]:
        b = int(instances["blas"][k]); tris = blas_tris[b]
        wb = world_box(instances["object_to_world"][k], root_boxes[b]).astype(np.float64)
        g = 0.5 * QUERY_GROW * np.abs(wb).max()
        wlo, whi = wb[:3] - g, wb[3:] + g
        orays = object_rays(rays, w[k])
        v0, v1, v2 = tri_vertices(tris)
        lo = np.minimum(np.minimum(v0, v1), v2).astype(np.float64); hi = np.maximum(np.maximum(v0, v1), v2).astype(np.float64)
        gt = 0.5 * QUERY_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True)
        step = max(1, chunk_elems // max(len(tris), 1))
        for s in range(0, m, step):
            r = orays[s:s + step]; rw = rays[s:s + step]
            it, iu, iv, iw = tri_formula(r["origin"].astype(F32)[:, None, :], r["direction"].astype(F32)[:, None, :], v0[None], v1[None], v2[None])
            acc = accepted(it, iu, iv, iw, r["tmin"][:, None], r["tmax"][:, None]) & ok[s:s + step, None]
            tk = np.where(acc, it, np.inf)
            best = tk.argmin(axis=1); rows = np.arange(len(r))
            has = acc[rows, best]; bt = tk[rows, best]
            sl = out[s:s + step]
            better = has & (bt < sl["t"])                          # (instances in increasing order: an equal t keeps the lower instance)
            sl["t"][better] = bt[better]; sl["u"][better] = iu[rows, best][better]; sl["v"][better] = iv[rows, best][better]
            sl["prim"][better] = best[better]; sl["instance"][better] = k
            out[s:s + step] = sl
            ri, pi = np.nonzero(acc)
            if ri.size:
                po = r["origin"][ri].astype(np.float64) + it[ri, pi].astype(np.float64)[:, None] * r["direction"][ri].astype(np.float64)
                pw = rw["origin"][ri].astype(np.float64) + it[ri, pi].astype(np.float64)[:, None] * rw["direction"][ri].astype(np.float64)
                inside = ((po >= lo[pi] - gt[pi]) & (po <= hi[pi] + gt[pi])).all(axis=1) & ((pw >= wlo) & (pw <= whi)).all(axis=1)
                bad = np.zeros(len(r), dtype=bool); np.logical_or.at(bad, ri, ~inside)
                well[s:s + step] &= ~bad
    return {"closest": out, "hit": out["prim"] != pkg.INVALID, "well": well}


def scene_recompute(pkg, rays, blas_tris, instances, hits):
    """per reported hit: an accepted hit of (instance, prim) with bit-equal t / u / v; a miss must be the miss record"""
    w, active = instance_inverse(instances["object_to_world"])
    active &= instances["blas"] < len(blas_tris)
    good = np.zeros(len(rays), dtype=bool)
    miss = hits["prim"] == pkg.INVALID
    good[miss] = ((hits["t"].view(np.uint32) == rays["tmax"].view(np.uint32)) & (hits["u"] == 0) & (hits["v"] == 0) & (hits["instance"] == pkg.INVALID))[miss]
    for i in np.nonzero(~miss)[0]:
        k, p = int(hits["instance"][i]), int(hits["prim"][i])
        if k >= len(instances) or not active[k] or p >= len(blas_tris[instances["blas"][k]]):
            continue
        tris = blas_tris[instances["blas"][k]][p:p + 1]
        r = object_rays(rays[i:i + 1], w[k])
        v0, v1, v2 = tri_vertices(tris)
        it, iu, iv, iw = tri_formula(r["origin"].astype(F32), r["direction"].astype(F32), v0, v1, v2)
        acc = accepted(it, iu, iv, iw, r["tmin"], r["tmax"]) & ray_ok(rays[i:i + 1])
        same = (it.view(np.uint32) == hits["t"][i:i + 1].view(np.uint32)) & (iu.view(np.uint32) == hits["u"][i:i + 1].view(np.uint32)) & \
               (iv.view(np.uint32) == hits["v"][i:i + 1].view(np.uint32))
        good[i] = bool((acc & same)[0])
    return good


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)


SCENE_FUNCS = ["bvh_build_boxes", "bvh_scene_create", "bvh_scene_destroy", "bvh_scene_build", "bvh_scene_update", "bvh_scene_intersect", "bvh_scene_tlas"]


def test_header_declares_scene_types_and_entry_points(pkg):
    types = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh", "types.h")).read(), flags=re.S)
    assert re.search(r"typedef struct\s*\{\s*float object_to_world\[12\];\s*uint32_t blas;\s*uint32_t reserved\[3\];\s*\}\s*bvh_instance;", types)
    assert re.search(r"typedef struct\s*\{\s*float t, u, v;\s*uint32_t prim_idx, instance_idx;\s*uint32_t reserved\[3\];\s*\}\s*bvh_instance_hit;", types)
    text = header_text()
    assert re.search(r"typedef struct\s*\{\s*bvh_result tree;\s*bvh_build_input tris;\s*\}\s*bvh_blas;", text)
    assert re.search(r"typedef struct bvh_scene bvh_scene;", text)
    assert re.search(r"\bint\s+bvh_build_boxes\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*bvh_algo\s+\w+\s*,\s*const void\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*int\s+\w+\s*,\s*"
                     r"bvh_result\s*\*\s*\w+\s*,\s*bvh_timings\s*\*\s*\w+\s*\)", text)
    assert re.search(r"\bint\s+bvh_scene_build\s*\(\s*bvh_scene\s*\*\s*\w+\s*,\s*bvh_algo\s+\w+\s*,\s*const bvh_blas\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*"
                     r"const bvh_instance\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*int\s+\w+\s*,\s*bvh_timings\s*\*\s*\w+\s*\)", text)
    assert re.search(r"\bint\s+bvh_scene_intersect\s*\(\s*bvh_scene\s*\*\s*\w+\s*,\s*const bvh_ray\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*bvh_instance_hit\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text
    L = C.CDLL(pkg.LIB_PATH)
    for name in SCENE_FUNCS:
        assert hasattr(L, name) and name in pkg.EXPORTS
    assert pkg.lib().bvh_abi_version() == 4 and b"0.4" in pkg.lib().bvh_version()


def test_struct_sizes(pkg, tmp_path):
    assert pkg.INSTANCE.itemsize == 64 and pkg.INSTANCE_HIT.itemsize == 32 and C.sizeof(pkg.Blas) == 128
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "bvh_mi355x.h"\nint main(void) { printf("%zu %zu %zu", sizeof(bvh_instance), sizeof(bvh_instance_hit), sizeof(bvh_blas)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-std=c++17", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout == "64 32 128"


def test_errors_without_a_device(pkg):
    """NULL arguments are refused before any device call"""
    L = pkg.lib()
    r = pkg.Result(); t = pkg.Timings(); h = C.c_void_p()
    box = np.zeros(4, dtype=pkg.AABB)
    assert L.bvh_build_boxes(None, 3, box.ctypes.data, 4, 30, C.byref(r), C.byref(t)) == E_INVALID
    assert L.bvh_scene_create(None, C.byref(h)) == E_INVALID
    blas = (pkg.Blas * 1)(); inst = np.zeros(1, dtype=pkg.INSTANCE)
    assert L.bvh_scene_build(None, 3, blas, 1, inst.ctypes.data, 1, 0, None) == E_INVALID
    assert L.bvh_scene_update(None, inst.ctypes.data, 0, None) == E_INVALID
    assert L.bvh_scene_intersect(None, 16, 1, 64, 0) == E_INVALID
    assert L.bvh_scene_tlas(None, C.byref(r)) == E_INVALID
    L.bvh_scene_destroy(None)


def rot(axis, ang):
    c, s = np.cos(ang), np.sin(ang)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3); R[i, i] = c; R[j, j] = c; R[i, j] = -s; R[j, i] = s
    return R


def mat34(A, t=(0.0, 0.0, 0.0)):
    return np.concatenate([np.asarray(A, dtype=np.float64), np.asarray(t, dtype=np.float64)[:, None]], axis=1).astype(F32).reshape(12)


def test_inverse_restatement_exact_on_hand_cases():
    cases = []
    for sx in (0.25, 1.0, 2.0, 4.0):                          # power-of-two scales, translations
        for t in ((0, 0, 0), (3.5, -2.0, 1024.0)):
            cases.append((np.diag([sx, 2.0 / sx if sx != 1 else 1.0, 0.5]), t))
    for perm in ((1, 2, 0), (2, 0, 1), (0, 2, 1)):            # axis permutations, mirrors
        cases.append((np.eye(3)[list(perm)], (1.0, 2.0, 3.0)))
        cases.append((-np.eye(3)[list(perm)] * 2.0, (-8.0, 0.25, 16.0)))
    cases.append((np.diag([-1.0, 1.0, 1.0]), (5.0, 0.0, 0.0)))
    for A, t in cases:
        M = mat34(A, t)
        w, active = instance_inverse(M)
        assert active[0]
        Ainv = np.linalg.inv(np.asarray(A, dtype=np.float64))
        exact = mat34(Ainv, -Ainv @ np.asarray(t, dtype=np.float64))
        assert np.array_equal(w[0], exact), (A, t, w[0], exact)       # (by value: a zero translation may come out as -0)
        # and a point maps back exactly
        p = np.array([[1.5, -3.0, 0.75]], dtype=F32)
        assert np.array_equal(xf_points(w[0], xf_points(M, p)), p)
    bad = [mat34(np.zeros((3, 3))), mat34(np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1.0]])), mat34(np.eye(3), (np.nan, 0, 0)),
           mat34(np.eye(3), (np.inf, 0, 0)), mat34(np.diag([1e-39, 1.0, 1.0])), mat34(np.diag([1e-30, 1e-30, 1e-30]))]
    _, active = instance_inverse(np.array(bad))
    assert not active[:5].any()                               # singular, NaN / inf entries, an inverse entry 1e39 that is not finite in f32
    assert active[5]                                          # (det 1e-90 is finite and non-zero in f64; the inverse 1e30 fits f32)



def small_mesh(pkg, n, seed):
    return pkg.meshgen.uniform(n, seed)


def random_rays(pkg, lo, hi, m, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(m, dtype=pkg.RAY)
    o = lo - 0.5 * (hi - lo) + rng.random((m, 3)) * 2.0 * (hi - lo)
    d = lo + rng.random((m, 3)) * (hi - lo) - o
    r["origin"] = o.astype(F32); r["direction"] = d.astype(F32); r["tmin"] = 0.0; r["tmax"] = 3e38
    return r


def test_two_level_brute_force_matches_flattened_with_identities(pkg):
    meshes = [small_mesh(pkg, 40, 1), small_mesh(pkg, 25, 2)]
    blas_of = [0, 1, 0]
    inst = make_instances(pkg, [identity()] * 3, blas_of)
    rays = random_rays(pkg, np.zeros(3), np.ones(3), 400, 3)
    got = scene_brute_force(pkg, rays, meshes, inst)
    flat = np.concatenate([meshes[b] for b in blas_of])
    offs = np.cumsum([0] + [len(meshes[b]) for b in blas_of])
    ref = brute_force(rays, flat)["closest"]
    hit = ref["prim"] != pkg.INVALID
    assert hit.sum() > 50
    k = np.searchsorted(offs, ref["prim"][hit], side="right") - 1
    g = got["closest"]
    assert np.array_equal(g["prim"] != pkg.INVALID, hit)
    for f in ("t", "u", "v"):
        assert np.array_equal(g[f].view(np.uint32), ref[f].view(np.uint32))
    assert np.array_equal(g["instance"][hit], k) and np.array_equal(g["prim"][hit], ref["prim"][hit] - offs[k])
    assert (g["instance"][~hit] == pkg.INVALID).all()
    assert scene_recompute(pkg, rays, meshes, inst, g).all()


def test_two_level_brute_force_tie_goes_to_the_lower_instance(pkg):
    mesh = small_mesh(pkg, 30, 4)
    inst = make_instances(pkg, [identity(), mat34(np.eye(3), (40.0, 0, 0)), identity()], [0, 0, 0])
    rays = random_rays(pkg, np.zeros(3), np.ones(3), 300, 5)
    g = scene_brute_force(pkg, rays, [mesh], inst)["closest"]
    hit = g["prim"] != pkg.INVALID
    assert hit.sum() > 30
    assert (g["instance"][hit] == 0).all()                    # instance 2 ties with 0 on every hit; instance 1 is far away
    inst2 = inst.copy(); inst2["blas"][0] = 7                 # instance 0 inactive (blas out of range): 2 wins
    g2 = scene_brute_force(pkg, rays, [mesh], inst2)["closest"]
    assert (g2["instance"][hit] == 2).all() and np.array_equal(g2["t"], g["t"])
