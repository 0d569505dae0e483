#!/usr/bin/env python3
"""time of bvh_refit against a full rebuild, one process, one device.

For each mesh and builder: one build, then --refits refits timed with HIP events on the context's stream, alternating two device-resident meshes (the
build's and a jittered copy); the parent plan is made by the first (untimed) refit and excluded.  A second run with per-kernel events refits a
caller-owned copy of the tree (which makes the plan on every call) for the per-kernel split and the plan's own cost.  In the same process: the full
E+M+S+B build time of the same mesh for single-pass LBVH and HPLOC.  Writes <out>/refit.json and <out>/refit.md.

    python tools/time_refit.py                 # uniform 10 M, uniform 2 M, Sponza-like 262 144
    python tools/time_refit.py --n 10000000    # one uniform mesh
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
import bvh_pkg  # noqa: E402

BYTES_PER_PRIM = 200          # nominal bytes a refit moves per primitive (DESIGN.md "Refit"); bvh_timings.bytes_algorithmic
HBM_BPS = 8e12


def jitter(tris, seed, scale=1e-3):
    rng = np.random.default_rng(seed)
    t = tris.copy()
    for f in ("v1", "v2", "v3"):
        t[f] = (t[f] + rng.normal(0.0, scale, t[f].shape)).astype(np.float32)
    return t


def timed(stream, fn, reps):
    """mean ms per call of fn() over reps calls, HIP events around the whole loop"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    for i in range(reps):
        fn(i)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one uniform mesh of this size instead of the default three")
    ap.add_argument("--refits", type=int, default=200)
    ap.add_argument("--builds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    meshes = [("uniform", a.n)] if a.n else [("uniform", 10_000_000), ("uniform", 2_000_000), ("sponza", 262_144)]
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    rows = []
    for kind, n in meshes:
        tris = pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 1)
        ctx.reserve(n)
        d_a, d_b = ctx.upload(tris), ctx.upload(jitter(tris, 7))
        builds = {}
        for algo in (pkg.ALGO_SINGLEPASS, pkg.ALGO_HPLOC):
            res = pkg.Result()
            def build(i, algo=algo, res=res):
                assert L.bvh_build(ctx.handle, algo, d_a.ptr, n, 1, C.byref(res), None) == 0
            build(0); build(0)
            builds[pkg.ALGO_NAMES[algo]] = timed(stream, build, a.builds)
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, d_a, on_device=True, n=n)
            res = b.result
            def refit(i, res=res):
                assert L.bvh_refit(ctx.handle, C.byref(res), (d_b if i % 2 == 0 else d_a).ptr, 1, None) == 0
            for i in range(4):
                refit(i)                                  # (the first one makes the plan)
            ms = timed(stream, refit, a.refits)
            # per-kernel split and the plan: a caller-owned copy of the tree (a new plan on every call)
            n_nodes = 2 * n - 1 if res.layout == 0 else n - 1
            own = {"d_nodes": ctx.alloc(n_nodes * 32), "d_prim_aabbs": ctx.alloc(n * 24), "d_scene_extent": ctx.alloc(24)}
            if res.layout == 1:
                own["d_leaves"] = ctx.alloc(n * 28)
            sizes = {"d_nodes": n_nodes * 32, "d_prim_aabbs": n * 24, "d_scene_extent": 24, "d_leaves": n * 28}
            mine = pkg.Result.from_buffer_copy(res)
            for f, buf in own.items():
                assert L.bvh_dev_copy(ctx.handle, buf.ptr, getattr(res, f), sizes[f]) == 0
                setattr(mine, f, buf.ptr)
            reps = 20
            ctx.synchronize()
            ctx.set_profiling(2)
            for i in range(reps):
                assert L.bvh_refit(ctx.handle, C.byref(mine), (d_b if i % 2 == 0 else d_a).ptr, 1, None) == 0
            kt = {k: v[0] / v[1] for k, v in ctx.kernel_times().items()}
            ctx.set_profiling(0)
            for buf in own.values():
                buf.free()
            row = {"mesh": kind, "n": n, "builder": pkg.ALGO_NAMES[algo], "refit_ms": round(ms, 4), "plan_ms": round(kt.get("k_refit_plan", 0.0), 4),
                   "kernels_ms": {k: round(v, 4) for k, v in kt.items()},
                   "bytes_per_refit": BYTES_PER_PRIM * n, "fraction_of_8TBps": round(BYTES_PER_PRIM * n / (ms * 1e-3) / HBM_BPS, 3),
                   "build_ms": {k: round(v, 4) for k, v in builds.items()},
                   "refit_over_lbvh_single_build": round(ms / builds["SinglePassLbvh"], 3)}
            row["bar_0.6_met"] = row["refit_over_lbvh_single_build"] <= 0.6
            rows.append(row)
            print(json.dumps(row), flush=True)
        d_a.free(); d_b.free()
    ctx.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "refit.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "refits": a.refits, "builds": a.builds, "rows": rows}, f, indent=1)
    with open(os.path.join(a.out, "refit.md"), "w") as f:
        f.write("# bvh_refit vs a full build (tools/time_refit.py)\n\n")
        f.write(f"{a.refits} refits per row, alternating two device-resident meshes, HIP events; plan excluded (cached). Per-kernel split: per-launch means of a\n"
                "caller-owned tree (new plan every call). Bytes: nominal 200 B / primitive.\n\n")
        f.write("| mesh | n | builder | refit ms | plan ms | k_extents | k_refit_climb | of 8 TB/s | LBVH-1 build ms | HPLOC build ms | refit / LBVH-1 |\n")
        f.write("|---|---:|---|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            k = r["kernels_ms"]
            f.write(f"| {r['mesh']} | {r['n']} | {r['builder']} | {r['refit_ms']:.4f} | {r['plan_ms']:.4f} | {k.get('k_extents', 0):.4f} | {k.get('k_refit_climb', 0):.4f} | "
                    f"{r['fraction_of_8TBps']:.2f} | {r['build_ms']['SinglePassLbvh']:.4f} | {r['build_ms']['HPLOC']:.4f} | {r['refit_over_lbvh_single_build']:.3f} |\n")


if __name__ == "__main__":
    main()
