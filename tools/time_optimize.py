#!/usr/bin/env python3
"""time and payoff of bvh_optimize (treelet restructuring), one process, one device.

For each mesh and builder (single-pass LBVH, PLOC++, HPLOC) and each round count: one build, then
  optimise ms   --reps optimisations timed one by one with HIP events on the context's stream, alternating two device-resident copies of the built tree
                (caller-owned node arrays; each copy is restored from the pristine tree between its runs, outside the events).  A caller-owned tree gets a
                new parent plan on every call, so the time includes k_refit_plan — what the first optimise after a build pays on the ctx's own tree.
  tree quality  BVH2 SAH (bvh_sah_cost) and the collapsed BVH4 cost (bvh_collapse4 + bvh_bvh4_cost) before and after
  ray payoff    bvh_intersect closest hit, camera (1024 x 1024 primary rays) and incoherent (1 M random rays), tools/time_query.py's workloads, before and after;
                break-even camera frames = optimise ms / camera ms saved per frame
A last pass with per-kernel events gives the k_refit_plan / k_optimize split.  Writes <out>/optimize.json and <out>/optimize.md.

    python tools/time_optimize.py                 # Sponza-like 262 144, uniform 2 M, uniform 10 M
    python tools/time_optimize.py --n 2000000     # one uniform mesh
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
from time_query import W, random_rays, timed, view  # noqa: E402


def per_call(stream, before, fn, reps):
    """mean ms of fn(i) over reps calls, each between its own pair of HIP events; before(i) runs outside them"""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for i, (e0, e1) in enumerate(evs):
        before(i)
        e0.record(stream)
        fn(i)
        e1.record(stream)
    evs[-1][1].synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in evs) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one uniform mesh of this size instead of the default three")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ray-reps", type=int, default=20)
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    meshes = [("uniform", a.n)] if a.n else [("sponza", 262_144), ("uniform", 2_000_000), ("uniform", 10_000_000)]
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
        d_inc = ctx.upload(random_rays(pkg, lo, hi, a.rays, 1, False))
        d_hits = ctx.alloc(max(W * W, a.rays) * 16)
        d_wide = ctx.alloc(n * 128); d_prims = ctx.alloc(n * 8)
        cost = C.c_double()
        for algo in (pkg.ALGO_SINGLEPASS, pkg.ALGO_PLOCPP, pkg.ALGO_HPLOC):
            for rounds in (1, 3):
                b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
                res = b.result
                node_bytes = (2 * n - 1 if res.layout == 0 else n - 1) * 32
                row = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(res.layout), "rounds": rounds}

                def quality(r):
                    assert L.bvh_sah_cost(ctx.handle, C.byref(r), C.byref(cost)) == 0
                    sah = cost.value
                    nw = C.c_uint32()
                    assert L.bvh_collapse4(ctx.handle, C.byref(r), d_wide.ptr, d_prims.ptr, C.byref(nw)) == 0
                    assert L.bvh_bvh4_cost(ctx.handle, d_wide.ptr, nw.value, d_prims.ptr, r.d_prim_aabbs, n, C.byref(cost)) == 0
                    return sah, cost.value

                def rays(r):
                    out = {}
                    for name, d_rays, m in (("camera", d_cam, W * W), ("incoherent", d_inc, a.rays)):
                        fn = lambda i: L.bvh_intersect(ctx.handle, C.byref(r), None, d_rays.ptr, m, d_hits.ptr, 0)
                        assert fn(0) == 0
                        out[name] = timed(stream, fn, a.ray_reps)
                    return out

                row["sah_before"], row["bvh4_cost_before"] = quality(res)
                rb = rays(res)
                # the pristine tree and two working copies of its nodes (leaves are read only)
                bufs = [ctx.alloc(node_bytes) for _ in range(3)]
                assert L.bvh_dev_copy(ctx.handle, bufs[0].ptr, res.d_nodes, node_bytes) == 0
                copies = []
                for k in (1, 2):
                    r = pkg.Result.from_buffer_copy(res); r.d_nodes = bufs[k].ptr
                    copies.append(r)
                restore = lambda i: L.bvh_dev_copy(ctx.handle, copies[i % 2].d_nodes, bufs[0].ptr, node_bytes)
                opt = lambda i: L.bvh_optimize(ctx.handle, C.byref(copies[i % 2]), rounds, None)
                restore(0); assert opt(0) == 0                                   # (warm)
                row["optimize_ms"] = per_call(stream, restore, opt, a.reps)
                # per-kernel split (events per launch)
                ctx.set_profiling(2)
                for i in range(10):
                    restore(i); assert opt(i) == 0
                row["kernels"] = {k: (ms / 10, cnt // 10) for k, (ms, cnt) in ctx.kernel_times().items() if k in ("k_refit_plan", "k_optimize")}
                ctx.set_profiling(0)
                for buf in bufs:
                    buf.free()
                # the builder's own tree, optimised: quality and rays after
                b.optimize(rounds)
                row["sah_after"], row["bvh4_cost_after"] = quality(res)
                ra = rays(res)
                for name in ("camera", "incoherent"):
                    row[f"{name}_ms_before"], row[f"{name}_ms_after"] = rb[name], ra[name]
                    m = W * W if name == "camera" else a.rays
                    row[f"{name}_mrays_s_before"], row[f"{name}_mrays_s_after"] = m / rb[name] / 1e3, m / ra[name] / 1e3
                saved = rb["camera"] - ra["camera"]
                row["break_even_camera_frames"] = row["optimize_ms"] / saved if saved > 0 else None
                rows.append(row)
                print(json.dumps(row), flush=True)
        for buf in (d_tris, d_cam, d_inc, d_hits, d_wide, d_prims):
            buf.free()
    ctx.close()
    os.makedirs(a.out, exist_ok=True)
    dev = torch.cuda.get_device_name(0)
    with open(os.path.join(a.out, "optimize.json"), "w") as f:
        json.dump({"device": dev, "reps": a.reps, "ray_reps": a.ray_reps, "rays": a.rays, "camera": W * W, "rows": rows}, f, indent=1)
    lines = [f"# bvh_optimize: time and payoff ({dev}, tools/time_optimize.py)", "",
             f"Optimise: mean of {a.reps} calls, HIP events per call, two alternating device-resident copies of the built tree, parent plan included.  "
             f"Rays: bvh_intersect closest hit, mean of {a.ray_reps} queries; camera = {W}x{W} primary rays, incoherent = {a.rays} random rays.  "
             "Break-even: optimise ms / camera ms saved per frame.", "",
             "| mesh | builder | rounds | optimise ms | plan / k_optimize ms | BVH2 SAH before -> after | BVH4 cost before -> after | camera ms before -> after | "
             "incoherent ms before -> after | break-even frames |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        k = r["kernels"]
        split = f"{k.get('k_refit_plan', (0.0, 0))[0]:.3f} / {k.get('k_optimize', (0.0, 0))[0]:.3f}"
        be = "never" if r["break_even_camera_frames"] is None else f"{r['break_even_camera_frames']:.1f}"
        lines.append(f"| {r['mesh']} | {r['builder']} | {r['rounds']} | {r['optimize_ms']:.3f} | {split} | {r['sah_before']:.2f} -> {r['sah_after']:.2f} | "
                     f"{r['bvh4_cost_before']:.2f} -> {r['bvh4_cost_after']:.2f} | {r['camera_ms_before']:.3f} -> {r['camera_ms_after']:.3f} | "
                     f"{r['incoherent_ms_before']:.3f} -> {r['incoherent_ms_after']:.3f} | {be} |")
    with open(os.path.join(a.out, "optimize.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
