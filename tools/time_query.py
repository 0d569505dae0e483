#!/usr/bin/env python3
"""time of bvh_intersect against the image traversal (bvh_trace, BVH_TRACE_WHILE_WHILE, identity transform), one process, one device.

For each mesh and builder (single-pass LBVH, HPLOC): one build, then --reps queries of each workload timed with HIP events around the loop on the context's
stream:
  camera      1024 x 1024 primary rays of bvh_generate_rays, closest hit; the same rays through k_trace_while on the same tree in the LBVH layout (HPLOC:
              bvh_to_lbvh_layout first, timed on its own, since that copy is what a caller pays today)
  incoherent  1 M rays, random origin in the scene box, random direction, closest hit and any hit
  segments    1 M any-hit segments of random length between two random points of the scene box
A second pass with per-kernel events splits k_intersect / k_intersect_deep.  The tree's height (and the deepest possible short stack, <= height - 1) is taken
from a read-back: a tree no taller than 65 cannot send a ray to the stackless pass.  Writes <out>/query.json.

    python tools/time_query.py                 # Sponza-like 262 144 and uniform 10 M
    python tools/time_query.py --n 2000000     # one uniform mesh
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

W = 1024


def timed(stream, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    for i in range(reps):
        fn(i)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def tree_height(pkg, b):
    t = b.download()
    n = b.result.n_leaves; ni = n - 1
    left = t["nodes"]["left"][:ni].astype(np.int64); right = t["nodes"]["right"][:ni].astype(np.int64)
    frontier, h = np.array([t["root"]]), 0
    while frontier.size:
        h += 1
        ch = np.concatenate([left[frontier], right[frontier]])
        frontier = ch[ch < ni]
    return h + 1                                          # (+ the leaf level)


def view(pkg, kind):
    cam, _ = pkg.cornell_view()
    cam = cam.copy()
    if kind == "sponza":
        cam["eye"][0] = (15.0, 6.0, 17.0, 0.0)
    else:
        cam["eye"][0] = (0.5, 0.5, 2.2, 0.0)
    cam["quat"][0] = pkg.qt_rotation((0.0, 1.0, 0.0, 0.0))
    xf = np.zeros(1, dtype=pkg.TRANSFORMATION); xf["scale"][0] = (1.0, 1.0, 1.0); xf["quat"][0] = (0.0, 0.0, 0.0, 1.0)
    return cam, xf


def random_rays(pkg, lo, hi, m, seed, segments):
    rng = np.random.default_rng(seed)
    r = np.zeros(m, dtype=pkg.RAY)
    o = lo + rng.random((m, 3)) * (hi - lo)
    if segments:
        p = lo + rng.random((m, 3)) * (hi - lo)
        d = p - o
        r["tmax"] = rng.random(m).astype(np.float32)       # t in units of d: a random fraction of the segment o -> p
    else:
        d = rng.normal(size=(m, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        r["tmax"] = 3.0e38
    r["origin"] = o.astype(np.float32); r["direction"] = d.astype(np.float32)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one uniform mesh of this size instead of the default two")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rays", type=int, default=1_000_000)
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
        cam, xf = view(pkg, kind)
        d_cam = ctx.alloc(W * W * 32)
        assert L.bvh_generate_rays(ctx.handle, np.ascontiguousarray(cam).ctypes.data, d_cam.ptr, W, W) == 0
        d_inc = ctx.upload(random_rays(pkg, lo, hi, a.rays, 1, False))
        d_seg = ctx.upload(random_rays(pkg, lo, hi, a.rays, 2, True))
        d_hits = ctx.alloc(max(W * W, a.rays) * 16)
        d_rgba = ctx.alloc(W * W * 4)
        d_lbvh = ctx.alloc((2 * n - 1) * 32)
        for algo in (pkg.ALGO_SINGLEPASS, pkg.ALGO_HPLOC):
            b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
            res = b.result
            row = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(res.layout), "height": tree_height(pkg, b)}
            row["stackless_pass_possible"] = row["height"] - 1 > 64

            def q(d_rays, m, kind_):
                return lambda i: L.bvh_intersect(ctx.handle, C.byref(res), None, d_rays.ptr, m, d_hits.ptr, kind_)
            for name, fn, m in (("camera_closest", q(d_cam, W * W, 0), W * W), ("camera_any", q(d_cam, W * W, 1), W * W),
                                ("incoherent_closest", q(d_inc, a.rays, 0), a.rays), ("incoherent_any", q(d_inc, a.rays, 1), a.rays),
                                ("segments_any", q(d_seg, a.rays, 1), a.rays)):
                assert fn(0) == 0
                ms = timed(stream, fn, a.reps)
                row[name + "_ms"] = ms; row[name + "_mrays_s"] = m / ms / 1e3
            # the image traversal on the same camera rays and the same tree in the LBVH layout
            nodes = res.d_nodes
            if res.layout == 1:
                conv = lambda i: L.bvh_to_lbvh_layout(ctx.handle, C.byref(res), d_lbvh.ptr)
                assert conv(0) == 0
                row["to_lbvh_layout_ms"] = timed(stream, conv, a.reps)
                nodes = d_lbvh.ptr
            trace = lambda i: L.bvh_trace(ctx.handle, 0, d_cam.ptr, d_tris.ptr, nodes, res.root, n - 1, np.ascontiguousarray(xf).ctypes.data, d_rgba.ptr, None, W, W)
            assert trace(0) == 0
            row["trace_while_ms"] = timed(stream, trace, a.reps)
            row["trace_while_mrays_s"] = W * W / row["trace_while_ms"] / 1e3
            row["trace_while_plus_layout_ms"] = row["trace_while_ms"] + row.get("to_lbvh_layout_ms", 0.0)
            # per-kernel split of the camera closest-hit query
            ctx.set_profiling(2)
            for _ in range(10):
                assert L.bvh_intersect(ctx.handle, C.byref(res), None, d_cam.ptr, W * W, d_hits.ptr, 0) == 0
            row["kernels_camera_closest"] = {k: (ms / cnt, cnt) for k, (ms, cnt) in ctx.kernel_times().items()}
            ctx.set_profiling(0)
            rows.append(row)
            print(json.dumps(row), flush=True)
        for buf in (d_tris, d_cam, d_inc, d_seg, d_hits, d_rgba, d_lbvh):
            buf.free()
    ctx.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "query.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rays": a.rays, "camera": W * W, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
