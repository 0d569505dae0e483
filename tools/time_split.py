#!/usr/bin/env python3
"""what early split clipping (bvh_split_refs) costs and buys; one process, one device.

For each mesh (Sponza-like 262 144, uniform 2 M) and sa_max = 1/4, 1/16 and 1/64 of the mesh's largest root-box area: the references per triangle, the count
and fill kernel times (per-kernel events of bvh_ctx_kernel_times over --reps calls: k_split_count, k_overlap_scan, k_split_fill, k_split_heavy), and for the
HPLOC and single-pass LBVH builders bvh_sah_cost of the tree over the references and of the unsplit tree, their build times (bvh_build_boxes over the
reference boxes against bvh_build on the triangles) and the time of 1024 x 1024 closest-hit camera rays (bvh_generate_rays, the view of tools/time_query.py) on
both trees with HIP events on the context's stream: one warm-up call, then --windows windows of --reps calls per tree — the two trees share one arena, so half
of the unsplit tree's windows run before the split tree's and half after, on a rebuilt tree; median window and spread.  The split tree is relabelled
(bvh_remap_leaves) and queried with the original triangles.  Nothing here is a pass criterion: where splitting does not pay the table says so.  Writes <out>/split.json and <out>/split.md, stamped with the library's machine-code hash.

    python tools/time_split.py                     # both meshes
    python tools/time_split.py --n 2000000         # one uniform mesh
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
from _srchash import kernel_source_hash  # noqa: E402
from time_query import timed, view  # noqa: E402

SPLIT_KERNELS = ("k_split_count", "k_overlap_scan", "k_split_fill", "k_split_heavy")


def render(doc):
    out = ["# bvh_split_refs — measured cost and effect (MI355X, one device)\n",
           f"`python tools/time_split.py` (raw rows: `profiles/split.json`; machine code `{doc['_kernel_source_hash']}`, the `kernel_source_hash` of `bench.py`; "
           f"device {doc['device']}).  sa_max = the mesh's largest root-box area / k, max_depth 16.  Kernel times: per-kernel events, mean of {doc['reps']} calls "
           f"(count = k_split_count + k_overlap_scan, fill = k_split_fill + k_split_heavy), ms.  Rays: {doc['width']} x {doc['width']} closest-hit camera rays, "
           f"HIP events on the context's stream, one warm-up call, then {doc['windows']} windows of {doc['reps']} calls per tree (half of the unsplit tree's windows "
           "before the split tree's, half after: one arena); ms per call, median window (smallest – largest).  SAH: `bvh_sah_cost`.  None of these numbers is a pass criterion.\n",
           "| mesh | k | refs / triangle | heavy triangles | count | fill | builder | SAH unsplit | SAH split | build unsplit | build split | rays unsplit | rays split |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        def cell(t):
            return f"{t['median']:.3f} ({t['min']:.3f} – {t['max']:.3f})"
        out.append(f"| {r['mesh']} | {r['k']} | {r['refs_per_triangle']:.3f} | {r['heavy']} | {r['count_ms']:.4f} | {r['fill_ms']:.4f} | {r['builder']} | "
                   f"{r['sah_unsplit']:.2f} | {r['sah_split']:.2f} | {r['build_unsplit_ms']:.3f} | {r['build_split_ms']:.3f} | {cell(r['rays_unsplit_ms'])} | "
                   f"{cell(r['rays_split_ms'])} |")
    return "\n".join(out) + "\n"


def root_area_max(tris):
    v = np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1)
    ext = (v.max(axis=1) - v.min(axis=1)).astype(np.float32)
    return np.float32((np.float32(2) * ((ext[:, 0] * ext[:, 1] + ext[:, 0] * ext[:, 2]) + ext[:, 1] * ext[:, 2])).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one uniform mesh of this size instead of the default two")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--ks", type=int, nargs="+", default=[4, 16, 64], help="sa_max = the largest root-box area / k")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    meshes = [("uniform", a.n)] if a.n else [("sponza", 262_144), ("uniform", 2_000_000)]
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    rows = []
    doc = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "width": a.width,
           "rows": rows}

    def dump():
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "split.json"), "w") as f:
            json.dump(doc, f, indent=1)
        with open(os.path.join(a.out, "split.md"), "w") as f:
            f.write(render(doc))

    W = a.width
    for kind, n in meshes:
        tris = pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 1)
        amax = root_area_max(tris)
        d_tris = ctx.upload(tris)
        inp = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_tris.ptr, None, None, 0, 0)
        cam, _ = view(pkg, kind)
        ctx.reserve(n)
        d_rays, d_hits = ctx.alloc(W * W * 32), ctx.alloc(W * W * 16)
        assert L.bvh_generate_rays(ctx.handle, np.ascontiguousarray(cam).ctypes.data, d_rays.ptr, W, W) == 0
        d_off = ctx.alloc((n + 1) * 4)
        for k in a.ks:
            sa = float(np.float32(amax * np.float32(1.0 / k)))
            total = C.c_uint64()
            assert L.bvh_split_refs(ctx.handle, C.byref(inp), n, sa, 16, d_off.ptr, None, None, 0, C.byref(total)) == 0
            total = int(total.value)
            counts = np.diff(d_off.download(np.uint32, n + 1).astype(np.int64))
            d_boxes, d_prims = ctx.alloc(total * 24), ctx.alloc(total * 4)
            assert L.bvh_split_refs(ctx.handle, C.byref(inp), n, sa, 16, d_off.ptr, d_boxes.ptr, d_prims.ptr, total, None) == 0      # warm-up
            ctx.set_profiling(2)
            for _ in range(a.reps):
                assert L.bvh_split_refs(ctx.handle, C.byref(inp), n, sa, 16, d_off.ptr, d_boxes.ptr, d_prims.ptr, total, None) == 0
            kt = ctx.kernel_times()
            ctx.set_profiling(0)
            per = {name: (kt[name][0] / max(kt[name][1], 1) if name in kt else 0.0) for name in SPLIT_KERNELS}
            # k_overlap_scan's mark covers both of its launches; every call makes one
            calls = {name: (kt[name][1] if name in kt else 0) for name in SPLIT_KERNELS}
            for algo in (pkg.ALGO_HPLOC, pkg.ALGO_SINGLEPASS):
                ctx.set_profiling(1)
                u = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
                u = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)              # (the second build: warm)
                build_unsplit = float(u.timings.ms_total)
                ctx.set_profiling(0)
                sah_unsplit = u.sah_cost()

                def shoot(b):
                    res = b.result
                    return lambda i: L.bvh_intersect(ctx.handle, C.byref(res), C.byref(inp), d_rays.ptr, W * W, d_hits.ptr, pkg.QUERY_CLOSEST)
                # the two trees cannot live in one arena at once: time the unsplit tree's windows, then the split tree's, then the unsplit tree's again
                times = {"unsplit": [], "split": []}
                fn = shoot(u)
                assert fn(0) == 0
                for _ in range((a.windows + 1) // 2):
                    times["unsplit"].append(timed(stream, fn, a.reps))
                ctx.set_profiling(1)
                s = pkg.BUILDERS[algo]().build_boxes(ctx, d_boxes, n=total)
                s = pkg.BUILDERS[algo]().build_boxes(ctx, d_boxes, n=total)
                build_split = float(s.timings.ms_total)
                ctx.set_profiling(0)
                sah_split = s.sah_cost()
                s.remap_leaves(d_prims, n_map=total)
                fn = shoot(s)
                assert fn(0) == 0
                for _ in range(a.windows):
                    times["split"].append(timed(stream, fn, a.reps))
                u = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
                fn = shoot(u)
                assert fn(0) == 0
                for _ in range(a.windows // 2):
                    times["unsplit"].append(timed(stream, fn, a.reps))
                row = {"mesh": f"{kind}_{n}", "n": n, "k": k, "sa_max": sa, "total": total, "refs_per_triangle": total / n, "max_refs": int(counts.max()),
                       "heavy": int((counts > 64).sum()), "kernel_ms": per, "kernel_calls": calls, "count_ms": per["k_split_count"] + per["k_overlap_scan"],
                       "fill_ms": per["k_split_fill"] + per["k_split_heavy"], "builder": pkg.ALGO_NAMES[algo], "sah_unsplit": sah_unsplit, "sah_split": sah_split,
                       "build_unsplit_ms": build_unsplit, "build_split_ms": build_split}
                for w in ("unsplit", "split"):
                    t = times[w]
                    row[f"rays_{w}_ms"] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "windows": t}
                rows.append(row)
                print(json.dumps(row), flush=True)
                dump()
            d_boxes.free(); d_prims.free()
        for buf in (d_tris, d_rays, d_hits, d_off):
            buf.free()
    ctx.close()
    dump()


if __name__ == "__main__":
    main()
