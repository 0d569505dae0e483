#!/usr/bin/env python3
"""time of instanced scenes (bvh_scene_*), one process, one device.  Writes <out>/scene.json.

  overhead    one identity instance over the Sponza-like 262 144 mesh (single-pass LBVH and HPLOC BLAS) against bvh_intersect on the same tree: 1024 x 1024
              primary rays (bvh_generate_rays, the view of tools/time_query.py), closest hit
  instancing  64 instances of that mesh on an 8 x 8 grid (16.8 M triangles in view) against one flattened HPLOC build of the same 16.8 M triangles: build
              time (bvh_scene_build, host wall clock, blocking, against bvh_build's events), closest-hit query time of 1024 x 1024 rays of a camera above the
              grid, and the device bytes each holds (triangles + tree arrays + scene memory; the contexts' arenas are scratch and not counted)
  update      bvh_scene_update of 10^5 instances (device records) of a small mesh, HIP events around the loop
A second pass with per-kernel events splits k_scene_intersect / k_scene_intersect_deep / k_instance_boxes / k_refit_climb.

    python tools/time_scene.py
    python tools/time_scene.py --reps 20 --skip-flat
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(ROOT)); sys.path.insert(0, ROOT)
import bvh_pkg  # noqa: E402
from time_query import W, timed, view  # noqa: E402


def stream_of(L, ctx):
    return torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))


def grid_instances(pkg, n_side, step, blas=0):
    k = np.arange(n_side * n_side)
    inst = np.zeros(len(k), dtype=pkg.INSTANCE)
    m = np.zeros((len(k), 12), dtype=np.float32); m[:, 0] = m[:, 5] = m[:, 10] = 1.0
    m[:, 3] = (k % n_side) * step[0]; m[:, 11] = (k // n_side) * step[2]
    inst["object_to_world"] = m; inst["blas"] = blas
    return inst


def pinhole_rays(pkg, eye, target, fov_deg=60.0):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = target - eye; f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 1.0, 0.0]); r /= np.linalg.norm(r); u = np.cross(r, f)
    s = np.tan(np.radians(fov_deg) / 2)
    x, y = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(W) + 0.5) / W * 2 - 1, indexing="ij")
    d = f[None] + s * x.reshape(-1, 1) * r[None] + s * y.reshape(-1, 1) * u[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(W * W, dtype=pkg.RAY)
    rays["origin"] = eye.astype(np.float32); rays["direction"] = d.astype(np.float32); rays["tmax"] = 3.0e38
    return rays


def kernel_split(ctx, fn, reps=10):
    ctx.set_profiling(2)
    for i in range(reps):
        assert fn(i) == 0
    out = {k: (ms / cnt, cnt) for k, (ms, cnt) in ctx.kernel_times().items()}
    ctx.set_profiling(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--n", type=int, default=262_144)
    ap.add_argument("--update-instances", type=int, default=100_000)
    ap.add_argument("--skip-flat", action="store_true", help="no flattened 64-copy build (host memory / time)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(ROOT), "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    n = a.n
    tris = pkg.meshgen.sponza_like(n, 3)
    scene_ctx = pkg.Context(0); s_scene = stream_of(L, scene_ctx)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "camera": W * W, "n": n}
    # ---- overhead of the second level: one identity instance against bvh_intersect on the same tree
    cam, _ = view(pkg, "sponza")
    d_cam = scene_ctx.alloc(W * W * 32)
    scene_ctx.reserve(2)
    assert L.bvh_generate_rays(scene_ctx.handle, np.ascontiguousarray(cam).ctypes.data, d_cam.ptr, W, W) == 0
    d_ihits = scene_ctx.alloc(W * W * 32)
    out["overhead"] = []
    blas_ctx = {}
    for algo in (pkg.ALGO_SINGLEPASS, pkg.ALGO_HPLOC):
        c = pkg.Context(0); blas_ctx[algo] = c; s_blas = stream_of(L, c)
        d_tris = c.upload(tris); c._keep = d_tris
        b = pkg.BUILDERS[algo]().build(c, d_tris, on_device=True, n=n)
        d_rays = c.alloc(W * W * 32); d_hits = c.alloc(W * W * 16)
        assert L.bvh_dev_copy(c.handle, d_rays.ptr, d_cam.ptr, W * W * 32) == 0
        q = lambda i: L.bvh_intersect(c.handle, C.byref(b.result), None, d_rays.ptr, W * W, d_hits.ptr, 0)
        assert q(0) == 0
        t_one = timed(s_blas, q, a.reps)
        sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [b], grid_instances(pkg, 1, (0, 0, 0)))
        qs = lambda i: L.bvh_scene_intersect(sc.handle, d_cam.ptr, W * W, d_ihits.ptr, 0)
        assert qs(0) == 0
        t_sc = timed(s_scene, qs, a.reps)
        row = {"blas": pkg.ALGO_NAMES[algo], "intersect_ms": t_one, "scene_one_instance_ms": t_sc, "ratio": t_sc / t_one,
               "kernels": kernel_split(scene_ctx, qs)}
        out["overhead"].append(row); print(json.dumps(row), flush=True)
        sc.close(); d_rays.free(); d_hits.free()
        b_keep = b
    # ---- instancing against flattening: 64 instances on an 8 x 8 grid, HPLOC BLAS (the last one built above)
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    step = (hi - lo) * 1.1
    inst = grid_instances(pkg, 8, step)
    centre = np.array([lo[0] + 4 * step[0], hi[1], lo[2] + 4 * step[2]])
    rays = pinhole_rays(pkg, centre + np.array([0.0, 4 * step[0], -6 * step[2]]), centre - np.array([0.0, hi[1] - lo[1], 0.0]), 70.0)
    d_grid = scene_ctx.upload(rays)
    sc = pkg.Scene(scene_ctx)
    walls = []
    for i in range(max(3, a.reps // 10)):
        t0 = time.perf_counter(); sc.build(pkg.ALGO_HPLOC, [b_keep], inst); walls.append((time.perf_counter() - t0) * 1e3)
    qg = lambda i: L.bvh_scene_intersect(sc.handle, d_grid.ptr, W * W, d_ihits.ptr, 0)
    assert qg(0) == 0
    hits = d_ihits.download(pkg.INSTANCE_HIT, W * W)
    bytes_blas = n * 64 + (n - 1) * 32 + n * 28
    bytes_scene = 64 + 64 * 64 * 3 + 24 * 64 + 63 * 32 + 64 * 28 + 4 * 127 + 4 * 64 + 4 * (2 * n - 1)
    inst_row = {"instances": 64, "triangles_in_view": 64 * n, "scene_build_ms_wall": float(np.median(walls)), "scene_query_ms": timed(s_scene, qg, a.reps),
                "hit_fraction": float((hits["prim"] != pkg.INVALID).mean()), "instances_hit": int(len(np.unique(hits["instance"][hits["prim"] != pkg.INVALID]))),
                "bytes_blas_plus_scene": bytes_blas + bytes_scene, "kernels": kernel_split(scene_ctx, qg)}
    if not a.skip_flat:
        flat = np.concatenate([tris.copy() for _ in range(64)])
        for k in range(64):
            off = np.array([inst["object_to_world"][k][3], 0.0, inst["object_to_world"][k][11]], dtype=np.float32)
            for f in ("v1", "v2", "v3"):
                flat[f][k * n:(k + 1) * n] += off
        fctx = pkg.Context(0); s_flat = stream_of(L, fctx)
        fctx.reserve(64 * n)
        d_flat = fctx.upload(flat); del flat
        fb = pkg.HPLOC()
        build = lambda i: L.bvh_build(fctx.handle, pkg.ALGO_HPLOC, d_flat.ptr, 64 * n, 1, C.byref(fb.result), None)
        assert build(0) == 0
        inst_row["flat_build_ms"] = timed(s_flat, build, max(3, a.reps // 5))
        fb.result = pkg.Result.from_buffer_copy(fb.result)
        d_fr = fctx.upload(rays); d_fh = fctx.alloc(W * W * 16)
        qf = lambda i: L.bvh_intersect(fctx.handle, C.byref(fb.result), None, d_fr.ptr, W * W, d_fh.ptr, 0)
        assert qf(0) == 0
        inst_row["flat_query_ms"] = timed(s_flat, qf, a.reps)
        fh = d_fh.download(pkg.HIT, W * W)
        inst_row["flat_hit_fraction"] = float((fh["prim"] != pkg.INVALID).mean())
        inst_row["same_t_fraction"] = float((fh["t"] == hits["t"]).mean())
        inst_row["bytes_flat"] = 64 * n * 64 + (64 * n - 1) * 32 + 64 * n * 28
        for buf in (d_flat, d_fr, d_fh):
            buf.free()
        fctx.close()
    out["instancing"] = inst_row; print(json.dumps({k: v for k, v in inst_row.items() if k != "kernels"}), flush=True)
    sc.close(); d_grid.free()
    # ---- update of 10^5 instances of a small mesh
    m = a.update_instances
    small = pkg.meshgen.uniform(64, 5)
    c = pkg.Context(0); sb = pkg.HPLOC().build(c, small)
    side = int(np.ceil(np.sqrt(m)))
    inst = grid_instances(pkg, side, (1.5, 0, 1.5))[:m]
    sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [sb], inst)
    moved = inst.copy(); moved["object_to_world"][:, 7] += 0.25
    d_moved = scene_ctx.upload(moved)
    up = lambda i: L.bvh_scene_update(sc.handle, d_moved.ptr, 1, None)
    assert up(0) == 0
    t0 = time.perf_counter(); sc.build(pkg.ALGO_HPLOC, [sb], inst); rebuild_wall = (time.perf_counter() - t0) * 1e3
    upd = {"instances": m, "update_ms": timed(s_scene, up, a.reps), "scene_build_ms_wall": rebuild_wall, "kernels": kernel_split(scene_ctx, up)}
    out["update"] = upd; print(json.dumps(upd), flush=True)
    sc.close(); d_moved.free(); c.close()
    for cc in blas_ctx.values():
        cc._keep.free(); cc.close()
    d_cam.free(); d_ihits.free(); scene_ctx.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "scene.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
