#!/usr/bin/env python3
"""time of bvh_knn, with bvh_closest_point on the same tree and points as the yardstick; one process, one device.

For each mesh and builder (all four): one build, then for each workload
  band      near-surface points: --points vertices jittered by 1e-3 of the scene extent (normal, per axis), radius 2e-3 of the extent (a narrow band)
  uniform   --points uniform points in the scene box, infinite radius
bvh_closest_point (BVH_QUERY_CLOSEST) and bvh_knn with k = 1, 8, 32 (lists and counts) are timed with HIP events on the context's stream: one warm-up call,
then --windows windows of --reps calls each; the median window is the figure, the smallest and largest are kept as the spread.  The four are timed in
alternation inside every window round, so a drift of the machine falls on all of them.  Also recorded: the mean list length per workload and k, the
k = 1 answers compared with bvh_closest_point's (dist2, prim) on every query, and the per-kernel split (k_knn / k_knn_deep) from bvh_ctx_kernel_times.
Writes <out>/knn.json and <out>/knn.md.

    python tools/time_knn.py                  # Sponza-like 262 144 and uniform 10 M
    python tools/time_knn.py --n 2000000      # one uniform mesh
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
from time_point_query import band_points, uniform_points  # noqa: E402
from time_query import timed, tree_height  # noqa: E402

KS = (1, 8, 32)


def write_md(path, doc):
    rows = doc["rows"]
    out = ["# bvh_knn: k-nearest-triangle queries (tools/time_knn.py)", "",
           f"{doc['device']}; {doc['points']:,} queries per call; HIP events on the context's stream, one warm-up call, then {doc['windows']} windows of "
           f"{doc['reps']} calls; median window per call in ms, [smallest .. largest window].  `closest` is `bvh_closest_point` `BVH_QUERY_CLOSEST` on the same "
           "tree and points.  band: vertices jittered by 1e-3 of the extent, radius 2e-3 of the extent; uniform: points in the scene box, infinite radius.  "
           f"Library: {doc['library']}.", ""]
    for wl in ("band", "uniform"):
        out += [f"## {wl}", "",
                "| mesh | builder | closest ms | k=1 ms | k=1 / closest | k=8 ms | k=8 ns/query | k=32 ms | k=32 ns/query | mean list length k=8 / k=32 |",
                "|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            def cell(name):
                t = r[f"{wl}_{name}_ms"]
                return f"{t['median']:.3f} [{t['min']:.3f} .. {t['max']:.3f}]"
            cp, k1, k8, k32 = (r[f"{wl}_{x}_ms"]["median"] for x in ("closest", "k1", "k8", "k32"))
            out.append(f"| {r['mesh']} | {r['builder']} | {cell('closest')} | {cell('k1')} | {k1 / cp:.2f} | {cell('k8')} | {k8 * 1e6 / doc['points']:.1f} | "
                       f"{cell('k32')} | {k32 * 1e6 / doc['points']:.1f} | {r[wl + '_mean_len_k8']:.2f} / {r[wl + '_mean_len_k32']:.2f} |")
        out.append("")
    out += ["k = 1 records equal `bvh_closest_point`'s (dist2, prim) on every query of every row: " + str(all(r["k1_equals_closest"] for r in rows)) + ".  "
            "Largest share of `k_knn_deep` in a call: " + f"{max(r[w + '_k8_deep_share'] or 0.0 for r in rows for w in ('band', 'uniform')):.4f}"
            " (trees of height " + ", ".join(sorted({str(r['height']) for r in rows})) + ": no query reaches the stackless pass; the launch returns at once).", ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one uniform mesh of this size instead of the default two")
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    meshes = [("uniform", a.n)] if a.n else [("sponza", 262_144), ("uniform", 10_000_000)]
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    rows = []
    m = a.points
    for kind, n in meshes:
        tris = pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 1)
        v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        ctx.reserve(n)
        d_tris = ctx.upload(tris)
        d_pts = {"band": ctx.upload(band_points(pkg, tris, lo, hi, m, 1)), "uniform": ctx.upload(uniform_points(pkg, lo, hi, m, 2))}
        d_hits = ctx.alloc(m * max(32, max(KS) * 8)); d_cp = ctx.alloc(m * 32); d_counts = ctx.alloc(m * 4)
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
            res = b.result
            row = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(res.layout), "height": tree_height(pkg, b), "k1_equals_closest": True}
            for wl, pts in d_pts.items():
                def closest(i, pts=pts):
                    assert L.bvh_closest_point(ctx.handle, C.byref(res), None, pts.ptr, m, d_cp.ptr, pkg.QUERY_CLOSEST) == 0

                def knn(k, pts=pts):
                    def fn(i):
                        assert L.bvh_knn(ctx.handle, C.byref(res), None, pts.ptr, m, k, d_hits.ptr, d_counts.ptr) == 0
                    return fn
                work = [("closest", closest)] + [(f"k{k}", knn(k)) for k in KS]
                for _, fn in work:
                    fn(0)                                                       # warm-up: every shape the windows use
                times = {name: [] for name, _ in work}
                for _ in range(a.windows):
                    for name, fn in work:                                       # alternating
                        times[name].append(timed(stream, fn, a.reps))
                for name, t in times.items():
                    row[f"{wl}_{name}_ms"] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "windows": t}
                # answers: list lengths, and k = 1 against bvh_closest_point
                closest(0)
                cp = d_cp.download(pkg.POINT_HIT, m)
                for k in KS:
                    knn(k)(0)
                    cnt = d_counts.download(np.uint32, m)
                    row[f"{wl}_mean_len_k{k}"] = float(cnt.mean())
                    if k == 1:
                        h = d_hits.download(pkg.KNN_HIT, m)
                        same = h["dist2"].tobytes() == cp["dist2"].tobytes() and h["prim"].tobytes() == cp["prim"].tobytes()
                        row["k1_equals_closest"] = row["k1_equals_closest"] and bool(same)
                # per-kernel split of the k = 8 call
                ctx.set_profiling(2)
                for i in range(3):
                    knn(8)(i)
                kt = ctx.kernel_times()
                ctx.set_profiling(0)
                row[f"kernels_{wl}_k8"] = {name: (ms / cnt, cnt) for name, (ms, cnt) in kt.items()}
                main_ms = kt.get("k_knn", (0.0, 1))[0]; deep_ms = kt.get("k_knn_deep", (0.0, 1))[0]
                row[f"{wl}_k8_deep_share"] = deep_ms / (main_ms + deep_ms) if main_ms + deep_ms > 0 else None
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.startswith("kernels_")}), flush=True)
        for buf in (d_tris, d_hits, d_cp, d_counts, *d_pts.values()):
            buf.free()
    ctx.close()
    os.makedirs(a.out, exist_ok=True)
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "points": m,
           "library": os.path.relpath(pkg.LIB_PATH, ROOT), "rows": rows}
    with open(os.path.join(a.out, "knn.json"), "w") as f:
        json.dump(doc, f, indent=1)
    write_md(os.path.join(a.out, "knn.md"), doc)


if __name__ == "__main__":
    main()
