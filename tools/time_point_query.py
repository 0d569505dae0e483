#!/usr/bin/env python3
"""time of bvh_closest_point, with bvh_intersect camera rays on the same tree for scale; one process, one device.

For each mesh and builder (all four): one build, then --reps queries of each workload timed with HIP events around the loop on the context's stream:
  band      near-surface points: --points vertices jittered by 1e-3 of the scene extent (normal, per axis), radius 2e-3 of the extent (a narrow band);
            closest and any
  uniform   --points uniform points in the scene box, infinite radius; closest and any
  camera    1024 x 1024 primary rays of bvh_generate_rays through bvh_intersect, closest hit (the eye of tools/time_query.py)
A second pass with per-kernel events (bvh_ctx_kernel_times) splits k_closest_point / k_closest_point_deep per workload: the share of the deep pass in the
launch.  The tree's height is taken from a read-back: a tree no taller than 65 cannot send a query to the stackless pass.  Writes <out>/point_query.json.

    python tools/time_point_query.py                  # Sponza-like 262 144 and uniform 10 M
    python tools/time_point_query.py --n 2000000      # one uniform mesh
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bvh_pkg  # noqa: E402
from time_query import W, timed, tree_height, view  # noqa: E402


def band_points(pkg, tris, lo, hi, m, seed):
    rng = np.random.default_rng(seed)
    ext = float((hi - lo).max())
    f = ("v1", "v2", "v3")[seed % 3]
    base = tris[f][rng.integers(0, len(tris), size=m)].astype(np.float64)
    p = np.zeros(m, dtype=pkg.POINT_QUERY)
    p["point"] = (base + rng.normal(0.0, 1e-3 * ext, (m, 3))).astype(np.float32)
    p["radius"] = np.float32(2e-3 * ext)
    return p


def uniform_points(pkg, lo, hi, m, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros(m, dtype=pkg.POINT_QUERY)
    p["point"] = (lo + rng.random((m, 3)) * (hi - lo)).astype(np.float32)
    p["radius"] = np.inf
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one uniform mesh of this size instead of the default two")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    meshes = [("uniform", a.n)] if a.n else [("sponza", 262_144), ("uniform", 10_000_000)]
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    rows = []
    for kind, n in meshes:
        tris = pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 1)
        v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        ctx.reserve(n)
        d_tris = ctx.upload(tris)
        cam, _ = view(pkg, kind)
        d_cam = ctx.alloc(W * W * 32)
        assert L.bvh_generate_rays(ctx.handle, np.ascontiguousarray(cam).ctypes.data, d_cam.ptr, W, W) == 0
        d_band = ctx.upload(band_points(pkg, tris, lo, hi, a.points, 1))
        d_unif = ctx.upload(uniform_points(pkg, lo, hi, a.points, 2))
        d_hits = ctx.alloc(max(W * W * 16, a.points * 32))
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
            res = b.result
            row = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(res.layout), "height": tree_height(pkg, b)}
            row["stackless_pass_possible"] = row["height"] - 1 > 64

            def q(d_pts, kind_):
                return lambda i: L.bvh_closest_point(ctx.handle, C.byref(res), None, d_pts.ptr, a.points, d_hits.ptr, kind_)
            work = (("band_closest", q(d_band, 0)), ("band_any", q(d_band, 1)), ("uniform_closest", q(d_unif, 0)), ("uniform_any", q(d_unif, 1)))
            for name, fn in work:
                assert fn(0) == 0
                ms = timed(stream, fn, a.reps)
                row[name + "_ms"] = ms; row[name + "_mq_s"] = a.points / ms / 1e3
            # answers: hit fraction and mean distance of the closest queries (a read-back of the last launch of each)
            for name, d_pts in (("band", d_band), ("uniform", d_unif)):
                assert L.bvh_closest_point(ctx.handle, C.byref(res), None, d_pts.ptr, a.points, d_hits.ptr, 0) == 0
                h = d_hits.download(pkg.POINT_HIT, a.points)
                hit = h["prim"] != pkg.INVALID
                row[name + "_hit_fraction"] = float(hit.mean())
                row[name + "_mean_dist"] = float(np.sqrt(h["dist2"][hit].astype(np.float64)).mean()) if hit.any() else None
            cam_q = lambda i: L.bvh_intersect(ctx.handle, C.byref(res), None, d_cam.ptr, W * W, d_hits.ptr, 0)
            assert cam_q(0) == 0
            row["camera_closest_ms"] = timed(stream, cam_q, a.reps)
            row["camera_closest_mrays_s"] = W * W / row["camera_closest_ms"] / 1e3
            # per-kernel split (deep pass share) of each point workload
            for name, fn in work:
                ctx.set_profiling(2)
                for i in range(5):
                    assert fn(i) == 0
                kt = ctx.kernel_times()
                ctx.set_profiling(0)
                row["kernels_" + name] = {k: (ms / cnt, cnt) for k, (ms, cnt) in kt.items()}
                main_ms = kt.get("k_closest_point", (0.0, 1))[0]; deep_ms = kt.get("k_closest_point_deep", (0.0, 1))[0]
                row[name + "_deep_share"] = deep_ms / (main_ms + deep_ms) if main_ms + deep_ms > 0 else None
            rows.append(row)
            print(json.dumps(row), flush=True)
        for buf in (d_tris, d_cam, d_band, d_unif, d_hits):
            buf.free()
    ctx.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "point_query.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "points": a.points, "camera": W * W, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
