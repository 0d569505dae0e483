#!/usr/bin/env python3
"""time of box queries on instanced scenes (bvh_scene_overlap), one process, one device.  Writes <out>/scene_overlap.json and <out>/scene_overlap.md,
stamped with the library's machine-code hash.

  one instance   one identity instance over the Sponza-like 262 144 mesh (HPLOC BLAS) against bvh_overlap on the same tree: same offsets, same prims
  64 instances   the 64-instance scene of tools/time_scene.py (an 8 x 8 grid of that mesh, 16.8 M triangles) against bvh_overlap on a flat HPLOC build of
                 the 16.8 M world triangles (--skip-flat: without it).  A time comparison only: the flat tree's leaf boxes are the world triangles' own
                 boxes, never larger than the mapped object boxes (equal under these translations up to the rounding of the sum), so both totals are
                 reported
on 2^20 query boxes centred on tools/time_scene_point.py's near-surface points (a point of a random triangle moved by up to 0.05) with each of --halves as
the half-width on every axis; the slice-length distribution is recorded beside every figure.  Calls timed: count only / count + unsorted fill / count +
sorted fill (the capacity is the total, no read-back).  HIP events on the context's stream: one warm-up call of every shape, then --windows windows of
--reps calls each, the calls of a case timed in alternation inside every window round so that a drift of the machine falls on all of them; the median
window is the figure, the smallest and largest are kept as the spread (tools/time_scene_knn.py's method).  A separate pass with per-kernel events splits
k_scene_overlap_count / k_scene_overlap_fill / k_scene_overlap_deep / k_overlap_scan.  The kernels' registers, scratch and LDS are read from the compiler
(-Rpass-analysis=kernel-resource-usage on csrc/scene_overlap.hip) when hipcc is there.

    python tools/time_scene_overlap.py
    python tools/time_scene_overlap.py --reps 3 --windows 3 --skip-flat
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
from bench import kernel_source_hash  # noqa: E402
from time_scene import grid_instances, kernel_split, stream_of  # noqa: E402
from time_scene_knn import windows  # noqa: E402
from time_scene_point import point_sets  # noqa: E402
from time_scene_radius import distribution, world_copies  # noqa: E402

M = 1 << 20
SORTED = 1
PASSES = (("count", None), ("unsorted", 0), ("sorted", SORTED))


def resource_usage():
    """{kernel: {vgprs, sgprs, scratch, lds, occupancy}} of csrc/scene_overlap.hip as the Makefile compiles it, or {} without hipcc"""
    csrc = os.path.join(os.path.dirname(ROOT), "hip-bvh-construction_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return {}
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(os.path.dirname(ROOT), "include"), "-I" + csrc,
           "-mllvm", "-amdgpu-kernarg-preload-count=16", "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(csrc, "scene_overlap.hip"), "-o", os.devnull]
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


class Searcher:
    """the three timed calls of one entry point on one set of device boxes, the capacity taken from a first counting call"""

    def __init__(self, ctx, m, record_bytes, search):
        self.ctx, self.m, self.search = ctx, m, search                     # search(flags, d_offsets, d_prims, capacity, total_out) -> rc
        self.d_off = ctx.alloc((m + 1) * 4)
        total = C.c_uint64()
        assert search(0, self.d_off.ptr, None, 0, C.byref(total)) == 0
        self.total = total.value
        self.d_prims = ctx.alloc(max(self.total, 1) * record_bytes)

    def fn(self, flags):
        if flags is None:
            return lambda i: self.search(0, self.d_off.ptr, None, 0, None)
        return lambda i: self.search(flags, self.d_off.ptr, self.d_prims.ptr, self.total, None)

    def offsets(self):
        self.ctx.synchronize()
        return self.d_off.download(np.uint32, self.m + 1)

    def free(self):
        self.d_off.free(); self.d_prims.free()


def sorted_slices(off, prims):
    q = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    return prims[np.lexsort((prims, q))]


def write_md(out, path):
    cell = lambda t: f"{t['median']:.2f} ms [{t['min']:.2f} .. {t['max']:.2f}]"
    dist = lambda d: (f"{d['total']:,} records; empty {d['empty']:.3f}, median {d['median']:.0f}, mean {d['mean']:.2f}, p90 {d['p90']:.0f}, p99 {d['p99']:.0f}, "
                      f"longest {d['max']}, over 32: {d['over_32']:.3f}")
    L = [f"# Box queries on instanced scenes on one MI355X (`tools/time_scene_overlap.py --reps {out['reps']} --windows {out['windows']}`, "
         f"`profiles/scene_overlap.json`; machine code `{out['_kernel_source_hash']}`, the `kernel_source_hash` of `bench.py`)", "",
         f"{out['device']}.  Sponza-like mesh of {out['n']:,} triangles (HPLOC BLAS), {out['boxes']:,} query boxes centred on near-surface points (a point of a "
         f"random triangle moved by up to 0.05).  HIP events on the context's stream, one warm-up call, then {out['windows']} windows of {out['reps']} calls timed "
         "in alternation; median window per call, [smallest .. largest window].  count: a count-only call; unsorted / sorted: a call that counts and fills "
         "(capacity = the total, no read-back).  `bvh_overlap` has no sorted mode: its one fill stands beside both of the scene's, with a ratio for the unsorted "
         "one only.", ""]
    for case, title, flat in (("one_instance", "One identity instance against `bvh_overlap` on the same tree", "`bvh_overlap`"),
                              ("instancing", "64 instances (an 8 x 8 grid of the mesh, 16.8 M triangles, one BLAS)", "`bvh_overlap`, flat HPLOC build")):
        L += [f"## {title}", ""]
        for r in out[case]:
            L += [f"### half-width {r['half']}", "", f"Slices: {dist(r['slices'])}.", ""]
            if r.get("flat_ms"):
                L += [f"`bvh_overlap`'s slices: {dist(r['flat_slices'])}.", ""]
            L += [f"| call | {flat} | `bvh_scene_overlap` | ratio |", "|---|---|---|---|"]
            for name, _ in PASSES:
                if r.get("flat_ms") and name == "sorted":
                    L.append(f"| {name} | no sorted mode (its fill: {cell(r['flat_ms'][name])}) | {cell(r['scene_ms'][name])} | |")
                elif r.get("flat_ms"):
                    L.append(f"| {name} | {cell(r['flat_ms'][name])} | {cell(r['scene_ms'][name])} | {r['ratio'][name]:.2f}x |")
                else:
                    L.append(f"| {name} | not built | {cell(r['scene_ms'][name])} | |")
            L.append("")
            if r.get("flat_ms"):
                same = "not compared (the flat build numbers its primitives instance * n + prim)" if r["same_prims"] is None else r["same_prims"]
                L += [f"Same offsets as `bvh_overlap`: {r['same_offsets']}; same prims per slice: {same}.", ""]
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
    ap.add_argument("--boxes", type=int, default=M)
    ap.add_argument("--halves", type=float, nargs="+", default=[0.0125, 0.025, 0.05])
    ap.add_argument("--skip-flat", action="store_true", help="no flat HPLOC build of the 64 copies (host memory / time)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(ROOT), "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    n, m = a.n, a.boxes
    tris = pkg.meshgen.sponza_like(n, 3)
    out = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "boxes": m, "n": n,
           "halves": a.halves, "resources": resource_usage()}
    scene_ctx = pkg.Context(0); s_scene = stream_of(L, scene_ctx)
    bctx = pkg.Context(0); s_blas = stream_of(L, bctx)
    d_tris = bctx.upload(tris)
    b = pkg.HPLOC().build(bctx, d_tris, on_device=True, n=n)

    def case(sc, inst, seed, flat_ctx, flat_stream, flat_tree, compare):
        rows = []
        centres = np.ascontiguousarray(point_sets(pkg, tris, inst, m, seed)["near-surface"]["point"], dtype=np.float32)
        for half in a.halves:
            boxes = np.zeros(m, dtype=pkg.AABB); boxes["min"] = centres - np.float32(half); boxes["max"] = centres + np.float32(half)
            d_sb = scene_ctx.upload(boxes)
            scene = Searcher(scene_ctx, m, 8, lambda fl, o, h, cap, tot: L.bvh_scene_overlap(sc.handle, d_sb.ptr, m, fl, o, h, cap, tot))
            work = [(f"scene {name}", s_scene, scene.fn(fl)) for name, fl in PASSES]
            flat = None
            if flat_tree is not None:
                d_fb = flat_ctx.upload(boxes)
                flat = Searcher(flat_ctx, m, 4, lambda fl, o, h, cap, tot: L.bvh_overlap(flat_ctx.handle, C.byref(flat_tree.result), d_fb.ptr, m, 0, o, h, cap, tot))
                work += [("flat count", flat_stream, flat.fn(None)), ("flat fill", flat_stream, flat.fn(0))]
            t = windows(work, a.windows, a.reps)
            assert scene.fn(SORTED)(0) == 0
            off = scene.offsets()
            row = {"half": half, "slices": distribution(off), "scene_ms": {name: t[f"scene {name}"] for name, _ in PASSES}}
            if flat is not None:
                assert flat.fn(0)(0) == 0
                foff = flat.offsets()
                row["flat_slices"] = distribution(foff)
                row["flat_ms"] = {"count": t["flat count"], "unsorted": t["flat fill"], "sorted": t["flat fill"]}
                row["ratio"] = {name: t[f"scene {name}"]["median"] / row["flat_ms"][name]["median"] for name in ("count", "unsorted")}
                row["same_offsets"] = bool(off.tobytes() == foff.tobytes())
                row["same_prims"] = False if compare else None
                if compare and row["same_offsets"]:
                    got = scene.d_prims.download(pkg.INSTANCE_PRIM, scene.total)
                    ref = flat.d_prims.download(np.uint32, flat.total)
                    row["same_prims"] = bool((got["instance"] == 0).all() and got["prim"].tobytes() == sorted_slices(foff, ref).tobytes())
                flat.free(); d_fb.free()
            row["kernels"] = kernel_split(scene_ctx, scene.fn(SORTED), reps=3)
            rows.append(row)
            print(json.dumps({"half": half, "slices": row["slices"], "scene": {k: v["median"] for k, v in row["scene_ms"].items()},
                              "flat": {k: v["median"] for k, v in row.get("flat_ms", {}).items()}, "flat_total": row.get("flat_slices", {}).get("total")}), flush=True)
            scene.free(); d_sb.free()
        return rows

    # ---- one identity instance against bvh_overlap on the same tree
    one = grid_instances(pkg, 1, (0, 0, 0))
    sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [b], one)
    out["one_instance"] = case(sc, one, 1, bctx, s_blas, b, True)
    sc.close()
    # ---- the 64 instances of tools/time_scene.py against a flat HPLOC build of the world triangles
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    inst = grid_instances(pkg, 8, (v.max(axis=0) - v.min(axis=0)) * 1.1)
    sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [b], inst)
    flat_ctx = flat_tree = s_flat = d_world = None
    if not a.skip_flat:
        flat_ctx = pkg.Context(0); s_flat = stream_of(L, flat_ctx)
        d_world = flat_ctx.upload(world_copies(pkg, tris, inst))
        flat_tree = pkg.HPLOC().build(flat_ctx, d_world, on_device=True, n=n * len(inst))
    out["instancing"] = case(sc, inst, 2, flat_ctx, s_flat, flat_tree, False)
    sc.close()
    for buf in (d_tris,) + ((d_world,) if d_world is not None else ()):
        buf.free()
    if flat_ctx is not None:
        flat_ctx.close()
    scene_ctx.close(); bctx.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "scene_overlap.json"), "w") as f:
        json.dump(out, f, indent=1)
    write_md(out, os.path.join(a.out, "scene_overlap.md"))


if __name__ == "__main__":
    main()
