#!/usr/bin/env python3
"""time of k-nearest queries on instanced scenes (bvh_scene_knn), one process, one device.  Writes <out>/scene_knn.json and <out>/scene_knn.md.

  one instance   one identity instance over the Sponza-like 262 144 mesh (HPLOC BLAS) against bvh_knn on the same tree, k = 1, 8, 32
  64 instances   the 64-instance scene of tools/time_scene_point.py (an 8 x 8 grid of that mesh, 16.8 M triangles), k = 1, 8, 32, with
                 bvh_scene_closest_point (BVH_QUERY_CLOSEST) on the same scene and points as the yardstick of k = 1
on 2^20 near-surface points (tools/time_scene_point.py's: a point of a random triangle moved by up to 0.05, radius 0.1).  HIP events on the context's stream:
one warm-up call of every shape, then --windows windows of --reps calls each, the calls of a case timed in alternation inside every window round so that a
drift of the machine falls on all of them; the median window is the figure, the smallest and largest are kept as the spread (tools/time_knn.py's method).  A
separate pass with per-kernel events splits k_scene_knn / k_scene_knn_deep.  The kernels' registers, scratch and LDS are read from the compiler
(-Rpass-analysis=kernel-resource-usage on csrc/scene_knn.hip) when hipcc is there.

    python tools/time_scene_knn.py
    python tools/time_scene_knn.py --reps 3 --windows 3
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(ROOT)); sys.path.insert(0, ROOT)
import bvh_pkg  # noqa: E402
from time_query import timed  # noqa: E402
from time_scene import grid_instances, kernel_split, stream_of  # noqa: E402
from time_scene_point import point_sets  # noqa: E402

M = 1 << 20
KS = (1, 8, 32)


def resource_usage():
    """{kernel: {vgprs, sgprs, scratch, lds, occupancy}} of csrc/scene_knn.hip as the Makefile compiles it, or {} without hipcc"""
    csrc = os.path.join(os.path.dirname(ROOT), "hip-bvh-construction_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return {}
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(os.path.dirname(ROOT), "include"), "-I" + csrc,
           "-mllvm", "-amdgpu-kernarg-preload-count=16", "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "scene_knn.hip"),
           "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void bvh::", "") or m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z\[\]/ ]+?): (\d+)", line)
        if m and name and m.group(1).strip() in keys:
            out[name][keys[m.group(1).strip()]] = int(m.group(2))
    return out


def windows(work, n_windows, reps):
    """{name: {median, min, max, windows}} of the (name, stream, fn) calls, timed in alternation"""
    for _, _, fn in work:
        assert fn(0) == 0                                                   # warm-up: every shape the windows use
    times = {name: [] for name, _, _ in work}
    for _ in range(n_windows):
        for name, s, fn in work:
            times[name].append(timed(s, fn, reps))
    return {name: {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "windows": t} for name, t in times.items()}


def write_md(out, path):
    cell = lambda t: f"{t['median']:.2f} ms [{t['min']:.2f} .. {t['max']:.2f}]"
    L = [f"# k-nearest queries on instanced scenes on one MI355X (`tools/time_scene_knn.py --reps {out['reps']} --windows {out['windows']}`, "
         "`profiles/scene_knn.json`)", "",
         f"{out['device']}.  Sponza-like mesh of {out['n']:,} triangles (HPLOC BLAS), {out['points']:,} near-surface points (a point of a random triangle moved "
         f"by up to 0.05, radius 0.1).  HIP events on the context's stream, one warm-up call, then {out['windows']} windows of {out['reps']} calls timed in "
         "alternation; median window per call, [smallest .. largest window].", "",
         "## One identity instance against `bvh_knn` on the same tree", "",
         "| k | `bvh_knn` | `bvh_scene_knn`, 1 instance | ratio | mean list length | same (dist2, prim) lists |", "|---|---|---|---|---|---|"]
    for r in out["one_instance"]:
        L.append(f"| {r['k']} | {cell(r['knn_ms'])} | {cell(r['scene_ms'])} | {r['ratio']:.2f}x | {r['mean_len']:.2f} | {r['same_lists_fraction']:.4f} |")
    L += ["", "## 64 instances (an 8 x 8 grid of the mesh, 16.8 M triangles, one BLAS)", "",
          f"`bvh_scene_closest_point` (`BVH_QUERY_CLOSEST`) on the same scene and points: {cell(out['instancing']['closest_ms'])}.", "",
          "| k | `bvh_scene_knn` | against `bvh_scene_closest_point` | mean list length | `k_scene_knn` (ms) | `k_scene_knn_deep` (ms) |", "|---|---|---|---|---|---|"]
    for r in out["instancing"]["rows"]:
        kt = r["kernels"]
        L.append(f"| {r['k']} | {cell(r['scene_ms'])} | {r['ratio_to_closest']:.2f}x | {r['mean_len']:.2f} | {kt['k_scene_knn'][0]:.3f} | "
                 f"{kt['k_scene_knn_deep'][0]:.4f} |")
    L += ["", f"k = 1 records equal `bvh_scene_closest_point`'s (dist2, prim, instance) on every query: {out['instancing']['k1_equals_closest']}.", "",
          "## Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", ""]
    if out["resources"]:
        L += ["| kernel | VGPRs | SGPRs | scratch (bytes / lane) | LDS (bytes / block) | occupancy (waves / SIMD) |", "|---|---|---|---|---|---|"]
        for name, r in out["resources"].items():
            L.append(f"| `{name}` | {r.get('vgprs')} | {r.get('sgprs')} | {r.get('scratch')} | {r.get('lds')} | {r.get('occupancy')} |")
    else:
        L.append("not measured (no hipcc where the tool ran)")
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--n", type=int, default=262_144)
    ap.add_argument("--points", type=int, default=M)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(ROOT), "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    n, m = a.n, a.points
    tris = pkg.meshgen.sponza_like(n, 3)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "points": m, "n": n, "resources": resource_usage()}
    scene_ctx = pkg.Context(0); s_scene = stream_of(L, scene_ctx)
    bctx = pkg.Context(0); s_blas = stream_of(L, bctx)
    d_tris = bctx.upload(tris)
    b = pkg.HPLOC().build(bctx, d_tris, on_device=True, n=n)
    kmax = max(KS)
    d_shits = scene_ctx.alloc(m * kmax * 16); d_scounts = scene_ctx.alloc(m * 4); d_cp = scene_ctx.alloc(m * 32)
    d_bhits = bctx.alloc(m * kmax * 8); d_bcounts = bctx.alloc(m * 4)
    scene_knn = lambda sc, pts, k: (lambda i: L.bvh_scene_knn(sc.handle, pts.ptr, m, k, d_shits.ptr, d_scounts.ptr))
    # ---- one identity instance against bvh_knn on the same tree
    one = grid_instances(pkg, 1, (0, 0, 0))
    sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [b], one)
    pts = point_sets(pkg, tris, one, m, 1)["near-surface"]
    d_sp, d_bp = scene_ctx.upload(pts), bctx.upload(pts)
    flat_knn = lambda k: (lambda i: L.bvh_knn(bctx.handle, C.byref(b.result), None, d_bp.ptr, m, k, d_bhits.ptr, d_bcounts.ptr))
    work = [(f"knn{k}", s_blas, flat_knn(k)) for k in KS] + [(f"scene{k}", s_scene, scene_knn(sc, d_sp, k)) for k in KS]
    t = windows(work, a.windows, a.reps)
    out["one_instance"] = []
    for k in KS:
        assert flat_knn(k)(0) == 0 and scene_knn(sc, d_sp, k)(0) == 0
        bctx.synchronize(); scene_ctx.synchronize()
        ref = d_bhits.download(pkg.KNN_HIT, m * k).reshape(m, k)
        got = d_shits.download(pkg.INSTANCE_KNN_HIT, m * k).reshape(m, k)
        same = ((ref["dist2"].view(np.uint32) == got["dist2"].view(np.uint32)) & (ref["prim"] == got["prim"])).all(axis=1)
        row = {"k": k, "knn_ms": t[f"knn{k}"], "scene_ms": t[f"scene{k}"], "ratio": t[f"scene{k}"]["median"] / t[f"knn{k}"]["median"],
               "mean_len": float(d_scounts.download(np.uint32, m).mean()), "same_lists_fraction": float(same.mean())}
        out["one_instance"].append(row)
        print(json.dumps({"k": k, "knn": row["knn_ms"]["median"], "scene": row["scene_ms"]["median"], "ratio": row["ratio"], "same": row["same_lists_fraction"]}), flush=True)
    d_sp.free(); d_bp.free(); sc.close()
    # ---- the 64 instances of tools/time_scene_point.py, k = 1 against bvh_scene_closest_point
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    inst = grid_instances(pkg, 8, (v.max(axis=0) - v.min(axis=0)) * 1.1)
    sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [b], inst)
    pts = point_sets(pkg, tris, inst, m, 2)["near-surface"]
    d_sp = scene_ctx.upload(pts)
    closest = lambda i: L.bvh_scene_closest_point(sc.handle, d_sp.ptr, m, d_cp.ptr, 0)
    t = windows([("closest", s_scene, closest)] + [(f"scene{k}", s_scene, scene_knn(sc, d_sp, k)) for k in KS], a.windows, a.reps)
    assert closest(0) == 0
    scene_ctx.synchronize()
    cp = d_cp.download(pkg.INSTANCE_POINT_HIT, m)
    out["instancing"] = {"instances": 64, "closest_ms": t["closest"], "rows": []}
    for k in KS:
        fn = scene_knn(sc, d_sp, k)
        assert fn(0) == 0
        scene_ctx.synchronize()
        got = d_shits.download(pkg.INSTANCE_KNN_HIT, m * k).reshape(m, k)
        if k == 1:
            g = got[:, 0]
            out["instancing"]["k1_equals_closest"] = bool(g["dist2"].tobytes() == cp["dist2"].tobytes() and np.array_equal(g["prim"], cp["prim"]) and
                                                          np.array_equal(g["instance"], cp["instance"]))
        row = {"k": k, "scene_ms": t[f"scene{k}"], "ratio_to_closest": t[f"scene{k}"]["median"] / t["closest"]["median"],
               "mean_len": float(d_scounts.download(np.uint32, m).mean()), "kernels": kernel_split(scene_ctx, fn, reps=3)}
        out["instancing"]["rows"].append(row)
        print(json.dumps({"k": k, "scene": row["scene_ms"]["median"], "closest": t["closest"]["median"], "ratio": row["ratio_to_closest"]}), flush=True)
    d_sp.free(); sc.close()
    for buf in (d_shits, d_scounts, d_cp, d_bhits, d_bcounts, d_tris):
        buf.free()
    scene_ctx.close(); bctx.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "scene_knn.json"), "w") as f:
        json.dump(out, f, indent=1)
    write_md(out, os.path.join(a.out, "scene_knn.md"))


if __name__ == "__main__":
    main()
