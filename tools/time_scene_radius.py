#!/usr/bin/env python3
"""time of fixed-radius searches on instanced scenes (bvh_scene_radius_search), one process, one device.  Writes <out>/scene_radius.json and
<out>/scene_radius.md.

  one instance   one identity instance over the Sponza-like 262 144 mesh (HPLOC BLAS) against bvh_radius_search on the same tree
  64 instances   the 64-instance scene of tools/time_scene_point.py (an 8 x 8 grid of that mesh, 16.8 M triangles) against bvh_radius_search on a flat HPLOC
                 build of the 16.8 M world triangles (--skip-flat: without it)
on 2^20 near-surface points (tools/time_scene_point.py's: a point of a random triangle moved by up to 0.05) with each of --radii, chosen so that the median
slice holds a handful of triangles; the slice-length distribution is recorded beside every figure.  Calls timed: count only / count + unsorted fill / count +
sorted fill (the capacity is the total, no read-back), and bvh_scene_knn k = 32 on the same scene and points as a second yardstick.  HIP events on the context's
stream: one warm-up call of every shape, then --windows windows of --reps calls each, the calls of a case timed in alternation inside every window round so that
a drift of the machine falls on all of them; the median window is the figure, the smallest and largest are kept as the spread (tools/time_scene_knn.py's
method).  A separate pass with per-kernel events splits k_scene_radius_count / k_scene_radius_fill / k_scene_radius_deep / k_overlap_scan.  The kernels'
registers, scratch and LDS are read from the compiler (-Rpass-analysis=kernel-resource-usage on csrc/scene_radius.hip) when hipcc is there.

    python tools/time_scene_radius.py
    python tools/time_scene_radius.py --reps 3 --windows 3 --skip-flat
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
from time_scene import grid_instances, kernel_split, stream_of  # noqa: E402
from time_scene_knn import windows  # noqa: E402
from time_scene_point import point_sets  # noqa: E402

M = 1 << 20
SORTED = 1
PASSES = (("count", None), ("unsorted", 0), ("sorted", SORTED))


def resource_usage():
    """{kernel: {vgprs, sgprs, scratch, lds, occupancy}} of csrc/scene_radius.hip as the Makefile compiles it, or {} without hipcc"""
    csrc = os.path.join(os.path.dirname(ROOT), "hip-bvh-construction_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return {}
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(os.path.dirname(ROOT), "include"), "-I" + csrc,
           "-mllvm", "-amdgpu-kernarg-preload-count=16", "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(csrc, "scene_radius.hip"), "-o", os.devnull]
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


def distribution(offsets):
    n = np.diff(offsets.astype(np.int64))
    return {"total": int(n.sum()), "empty": float((n == 0).mean()), "mean": float(n.mean()), "median": float(np.median(n)), "p90": float(np.percentile(n, 90)),
            "p99": float(np.percentile(n, 99)), "max": int(n.max()), "over_32": float((n > 32).mean())}


def world_copies(pkg, tris, inst):
    """the world triangles of translated instances of one mesh, instance after instance (the scene's (instance, prim) is prim = instance * n + prim here)"""
    t = inst["object_to_world"].reshape(-1, 3, 4)[:, :, 3]
    out = np.zeros(len(inst) * len(tris), dtype=pkg.meshgen.TRIANGLE)
    for k in range(len(inst)):
        part = out[k * len(tris): (k + 1) * len(tris)]
        for f in ("v1", "v2", "v3"):
            part[f] = tris[f] + t[k]
    return out


class Searcher:
    """the three timed calls of one entry point on one set of device points, the capacity taken from a first counting call"""

    def __init__(self, ctx, m, search):
        self.ctx, self.m, self.search = ctx, m, search                     # search(flags, d_offsets, d_hits, capacity, total_out) -> rc
        self.d_off = ctx.alloc((m + 1) * 4)
        total = C.c_uint64()
        assert search(0, self.d_off.ptr, None, 0, C.byref(total)) == 0
        self.total = total.value
        self.d_hits = ctx.alloc(max(self.total, 1) * 16)

    def fn(self, flags):
        if flags is None:
            return lambda i: self.search(0, self.d_off.ptr, None, 0, None)
        return lambda i: self.search(flags, self.d_off.ptr, self.d_hits.ptr, self.total, None)

    def offsets(self):
        self.ctx.synchronize()
        return self.d_off.download(np.uint32, self.m + 1)

    def free(self):
        self.d_off.free(); self.d_hits.free()


def write_md(out, path):
    cell = lambda t: f"{t['median']:.2f} ms [{t['min']:.2f} .. {t['max']:.2f}]"
    dist = lambda d: (f"{d['total']:,} records; empty {d['empty']:.3f}, median {d['median']:.0f}, mean {d['mean']:.2f}, p90 {d['p90']:.0f}, p99 {d['p99']:.0f}, "
                      f"longest {d['max']}, over 32: {d['over_32']:.3f}")
    L = [f"# Fixed-radius searches on instanced scenes on one MI355X (`tools/time_scene_radius.py --reps {out['reps']} --windows {out['windows']}`, "
         "`profiles/scene_radius.json`)", "",
         f"{out['device']}.  Sponza-like mesh of {out['n']:,} triangles (HPLOC BLAS), {out['points']:,} near-surface points (a point of a random triangle moved "
         f"by up to 0.05).  HIP events on the context's stream, one warm-up call, then {out['windows']} windows of {out['reps']} calls timed in alternation; median "
         "window per call, [smallest .. largest window].  count: a count-only call; unsorted / sorted: a call that counts and fills (capacity = the total, no "
         "read-back).", ""]
    for case, title, flat in (("one_instance", "One identity instance against `bvh_radius_search` on the same tree", "`bvh_radius_search`"),
                              ("instancing", "64 instances (an 8 x 8 grid of the mesh, 16.8 M triangles, one BLAS)", "`bvh_radius_search`, flat HPLOC build")):
        L += [f"## {title}", ""]
        for r in out[case]:
            L += [f"### radius {r['radius']}", "", f"Slices: {dist(r['slices'])}.", ""]
            L += [f"| call | {flat} | `bvh_scene_radius_search` | ratio |", "|---|---|---|---|"]
            for name, _ in PASSES:
                if r.get("flat_ms"):
                    L.append(f"| {name} | {cell(r['flat_ms'][name])} | {cell(r['scene_ms'][name])} | {r['ratio'][name]:.2f}x |")
                else:
                    L.append(f"| {name} | not built | {cell(r['scene_ms'][name])} | |")
            L += ["", f"`bvh_scene_knn` k = 32 on the same scene and points: {cell(r['knn32_ms'])} (mean list length {r['knn32_mean_len']:.2f}).", ""]
            if r.get("flat_ms"):
                L += [f"Same offsets as the flat search: {r['same_offsets']}; same sorted (dist2, prim) records: {r['same_records']}.", ""]
            kt = r["kernels"]
            L += ["Per kernel, sorted call (ms per launch, launches): " + ", ".join(f"`{k}` {v[0]:.4f} ({v[1]})" for k, v in sorted(kt.items())) + ".", ""]
    L += ["## Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", ""]
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
    ap.add_argument("--radii", type=float, nargs="+", default=[0.025, 0.05, 0.1])
    ap.add_argument("--skip-flat", action="store_true", help="no flat HPLOC build of the 64 copies (host memory / time)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(ROOT), "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    n, m = a.n, a.points
    tris = pkg.meshgen.sponza_like(n, 3)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "points": m, "n": n, "radii": a.radii, "resources": resource_usage()}
    scene_ctx = pkg.Context(0); s_scene = stream_of(L, scene_ctx)
    bctx = pkg.Context(0); s_blas = stream_of(L, bctx)
    d_tris = bctx.upload(tris)
    b = pkg.HPLOC().build(bctx, d_tris, on_device=True, n=n)
    d_khits = scene_ctx.alloc(m * 32 * 16); d_kcounts = scene_ctx.alloc(m * 4)

    def case(sc, inst, seed, flat_ctx, flat_stream, flat_tree, n_per_instance):
        rows = []
        base = point_sets(pkg, tris, inst, m, seed)["near-surface"]
        for radius in a.radii:
            pts = base.copy(); pts["radius"] = radius
            d_sp = scene_ctx.upload(pts)
            scene = Searcher(scene_ctx, m, lambda fl, o, h, cap, tot: L.bvh_scene_radius_search(sc.handle, d_sp.ptr, m, fl, o, h, cap, tot))
            knn = lambda i: L.bvh_scene_knn(sc.handle, d_sp.ptr, m, 32, d_khits.ptr, d_kcounts.ptr)
            work = [(f"scene {name}", s_scene, scene.fn(fl)) for name, fl in PASSES] + [("knn32", s_scene, knn)]
            flat = None
            if flat_tree is not None:
                d_fp = flat_ctx.upload(pts)
                flat = Searcher(flat_ctx, m, lambda fl, o, h, cap, tot: L.bvh_radius_search(flat_ctx.handle, C.byref(flat_tree.result), None, d_fp.ptr, m, fl, o, h,
                                                                                              cap, tot))
                work += [(f"flat {name}", flat_stream, flat.fn(fl)) for name, fl in PASSES]
            t = windows(work, a.windows, a.reps)
            assert scene.fn(SORTED)(0) == 0
            off = scene.offsets()
            row = {"radius": radius, "slices": distribution(off), "scene_ms": {name: t[f"scene {name}"] for name, _ in PASSES}, "knn32_ms": t["knn32"],
                   "knn32_mean_len": float(d_kcounts.download(np.uint32, m).mean())}
            if flat is not None:
                assert flat.fn(SORTED)(0) == 0
                foff = flat.offsets()
                row["flat_ms"] = {name: t[f"flat {name}"] for name, _ in PASSES}
                row["ratio"] = {name: t[f"scene {name}"]["median"] / t[f"flat {name}"]["median"] for name, _ in PASSES}
                row["same_offsets"] = bool(off.tobytes() == foff.tobytes())
                got = scene.d_hits.download(pkg.INSTANCE_KNN_HIT, scene.total)
                ref = flat.d_hits.download(pkg.KNN_HIT, flat.total)
                row["same_records"] = bool(row["same_offsets"] and got["dist2"].tobytes() == ref["dist2"].tobytes() and
                                           np.array_equal(got["instance"].astype(np.uint64) * n_per_instance + got["prim"], ref["prim"]))
                flat.free(); d_fp.free()
            row["kernels"] = kernel_split(scene_ctx, scene.fn(SORTED), reps=3)
            rows.append(row)
            print(json.dumps({"radius": radius, "slices": row["slices"], "scene": {k: v["median"] for k, v in row["scene_ms"].items()},
                              "flat": {k: v["median"] for k, v in row.get("flat_ms", {}).items()}, "knn32": t["knn32"]["median"]}), flush=True)
            scene.free(); d_sp.free()
        return rows

    # ---- one identity instance against bvh_radius_search on the same tree
    one = grid_instances(pkg, 1, (0, 0, 0))
    sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [b], one)
    out["one_instance"] = case(sc, one, 1, bctx, s_blas, b, n)
    sc.close()
    # ---- the 64 instances of tools/time_scene_point.py against a flat HPLOC build of the world triangles
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    inst = grid_instances(pkg, 8, (v.max(axis=0) - v.min(axis=0)) * 1.1)
    sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [b], inst)
    flat_ctx = flat_tree = s_flat = d_world = None
    if not a.skip_flat:
        flat_ctx = pkg.Context(0); s_flat = stream_of(L, flat_ctx)
        d_world = flat_ctx.upload(world_copies(pkg, tris, inst))
        flat_tree = pkg.HPLOC().build(flat_ctx, d_world, on_device=True, n=n * len(inst))
    out["instancing"] = case(sc, inst, 2, flat_ctx, s_flat, flat_tree, n)
    sc.close()
    for buf in (d_khits, d_kcounts, d_tris) + ((d_world,) if d_world is not None else ()):
        buf.free()
    if flat_ctx is not None:
        flat_ctx.close()
    scene_ctx.close(); bctx.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "scene_radius.json"), "w") as f:
        json.dump(out, f, indent=1)
    write_md(out, os.path.join(a.out, "scene_radius.md"))


if __name__ == "__main__":
    main()
