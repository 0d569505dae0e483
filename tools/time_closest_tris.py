#!/usr/bin/env python3
"""time of bvh_closest_tris, with bvh_intersect_tris (count only) on the same pair of meshes and bvh_closest_point on the query mesh's 3 n vertices as the
context for the cost of its leaf routine; one process, one device.

For each mesh — bunny-like 327 680 and Sponza-like 262 144, each against a copy of itself moved by (0.37, 0.11, -0.23) of its extent, the pair
tools/time_intersect_tris.py and tests/test_intersect_tris.py use — and each builder (single-pass LBVH: layout 0; HPLOC: layout 1): one build of the tree over
the mesh, the moved copy as the queries, then
  closest / any, unbounded          radius +inf
  closest / any, band               radius 2e-3 of the extent's diagonal
  tris                              bvh_intersect_tris, count only, on the same pair
  points                            bvh_closest_point BVH_QUERY_CLOSEST, unbounded, on the moved copy's 3 n vertices
are timed with HIP events on the context's stream: one warm-up call each, then --windows windows of --reps calls; the median window is the figure, the
smallest and largest are kept as the spread.  The workloads alternate inside every window round, so a drift of the machine falls on all of them.  Also
recorded: hits, crossings (feature 15) and the smallest distance per workload, the vertex-only distance from bvh_closest_point (an upper bound of the true
one: it sees no edge-edge and no face-vertex minimum of the tree's side), and the per-kernel split from bvh_ctx_kernel_times.
Writes <out>/closest_tris.json and <out>/closest_tris.md.  These are reported numbers, not gates: there is no earlier figure to compare with.

    python tools/time_closest_tris.py
    python tools/time_closest_tris.py --n 20000      # both meshes at this size
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
from time_query import timed, tree_height  # noqa: E402

SHIFT = (0.37, 0.11, -0.23)
WORKLOADS = ("closest_inf", "any_inf", "closest_band", "any_band", "tris", "points")


def write_md(path, doc):
    out = ["# bvh_closest_tris: nearest triangle and distance, mesh to mesh (tools/time_closest_tris.py)", "",
           f"{doc['device']}; the queries are the tree's own mesh moved by {SHIFT} of its extent, one query per triangle; HIP events on the context's stream, one "
           f"warm-up call, then {doc['windows']} windows of {doc['reps']} calls; median window per call in ms, [smallest .. largest window].  band: radius 2e-3 "
           "of the extent's diagonal.  `tris` is `bvh_intersect_tris` count-only on the same pair; `points` is `bvh_closest_point` `BVH_QUERY_CLOSEST`, unbounded, "
           f"on the query mesh's 3 n vertices.  Reported numbers, not gates.  Library: {doc['library']}.", "",
           "| mesh | builder | closest inf ms | any inf ms | closest band ms | any band ms | tris (count) ms | points (3 n) ms | closest inf ns/query | closest inf / points |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        def cell(name):
            t = r[f"{name}_ms"]
            return f"{t['median']:.3f} [{t['min']:.3f} .. {t['max']:.3f}]"
        ci, pt = r["closest_inf_ms"]["median"], r["points_ms"]["median"]
        out.append(f"| {r['mesh']} | {r['builder']} | " + " | ".join(cell(w) for w in WORKLOADS) + f" | {ci * 1e6 / r['n']:.1f} | {ci / pt:.2f} |")
    out += ["", "| mesh | builder | hits inf / band | crossings (feature 15) | crossing rows of `tris` | distance | vertex-only distance (`points`) | share of `k_closest_tris_deep` |",
            "|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        out.append(f"| {r['mesh']} | {r['builder']} | {r['hits_inf']:,} / {r['hits_band']:,} | {r['crossings']:,} | {r['tris_rows']:,} | {r['distance']:.6g} | "
                   f"{r['vertex_distance']:.6g} | {r['deep_share']:.4f} |")
    out.append("")
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="both meshes at this size instead of 327 680 / 262 144")
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    rows = []
    for kind, n in (("bunny", a.n or 327_680), ("sponza", a.n or 262_144)):
        tris = pkg.meshgen.bunny_like(n, 2) if kind == "bunny" else pkg.meshgen.sponza_like(n, 3)
        n = len(tris)
        v = np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1).astype(np.float32)
        flat = v.reshape(-1, 3).astype(np.float64)
        ext = flat.max(axis=0) - flat.min(axis=0)
        moved = (v + (np.array(SHIFT) * ext).astype(np.float32)[None, None, :]).astype(np.float32)
        other = np.zeros(n, dtype=pkg.meshgen.TRIANGLE)
        other["v1"], other["v2"], other["v3"] = moved[:, 0], moved[:, 1], moved[:, 2]
        band = float(2e-3 * np.linalg.norm(ext))
        pts = np.zeros(3 * n, dtype=pkg.POINT_QUERY)
        pts["point"] = moved.reshape(-1, 3); pts["radius"] = np.inf
        ctx.reserve(n)
        d_tris, d_other, d_pts = ctx.upload(tris), ctx.upload(other), ctx.upload(pts)
        d_hits, d_off, d_ph = ctx.alloc(n * 16), ctx.alloc((n + 1) * 4), ctx.alloc(3 * n * 32)
        qin = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_other.ptr, None, None, 0, 0)
        for algo in (1, 3):
            b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
            res = b.result
            row = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(res.layout), "height": tree_height(pkg, b), "band": band}

            def closest(radius, q):
                def fn(i):
                    assert L.bvh_closest_tris(ctx.handle, C.byref(res), None, C.byref(qin), n, radius, d_hits.ptr, q) == 0
                return fn

            def tris_count(i):
                assert L.bvh_intersect_tris(ctx.handle, C.byref(res), None, C.byref(qin), n, pkg.TRIS_QUERY, d_off.ptr, None, 0, None) == 0

            def points(i):
                assert L.bvh_closest_point(ctx.handle, C.byref(res), None, d_pts.ptr, 3 * n, d_ph.ptr, pkg.QUERY_CLOSEST) == 0
            work = [("closest_inf", closest(float("inf"), pkg.QUERY_CLOSEST)), ("any_inf", closest(float("inf"), pkg.QUERY_ANY)),
                    ("closest_band", closest(band, pkg.QUERY_CLOSEST)), ("any_band", closest(band, pkg.QUERY_ANY)), ("tris", tris_count), ("points", points)]
            for _, fn in work:
                fn(0)                                                           # warm-up: every shape the windows use
            times = {name: [] for name, _ in work}
            for _ in range(a.windows):
                for name, fn in work:                                           # alternating
                    times[name].append(timed(stream, fn, a.reps))
            for name, t in times.items():
                row[f"{name}_ms"] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "windows": t}
            # answers
            work[0][1](0)
            h = d_hits.download(pkg.TRI_HIT, n)
            hit = h["prim"] != pkg.INVALID
            row["hits_inf"] = int(hit.sum()); row["crossings"] = int((hit & (h["feature"] == 15)).sum())
            row["distance"] = float(np.sqrt(np.float64(h["dist2"][hit].min()))) if hit.any() else float("inf")
            work[2][1](0)
            row["hits_band"] = int((d_hits.download(pkg.TRI_HIT, n)["prim"] != pkg.INVALID).sum())
            tris_count(0)
            row["tris_rows"] = int((np.diff(d_off.download(np.uint32, n + 1).astype(np.int64)) > 0).sum())
            points(0)
            row["vertex_distance"] = float(np.sqrt(np.float64(d_ph.download(pkg.POINT_HIT, 3 * n)["dist2"].min())))
            # per-kernel split of the unbounded closest call
            ctx.set_profiling(2)
            for i in range(3):
                work[0][1](i)
            kt = ctx.kernel_times()
            ctx.set_profiling(0)
            row["kernels_closest_inf"] = {name: (ms / cnt, cnt) for name, (ms, cnt) in kt.items()}
            main_ms = kt.get("k_closest_tris", (0.0, 1))[0]; deep_ms = kt.get("k_closest_tris_deep", (0.0, 1))[0]
            row["deep_share"] = deep_ms / (main_ms + deep_ms) if main_ms + deep_ms > 0 else 0.0
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.startswith("kernels_")}), flush=True)
        for buf in (d_tris, d_other, d_pts, d_hits, d_off, d_ph):
            buf.free()
    ctx.close()
    os.makedirs(a.out, exist_ok=True)
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "library": os.path.relpath(pkg.LIB_PATH, ROOT), "rows": rows}
    with open(os.path.join(a.out, "closest_tris.json"), "w") as f:
        json.dump(doc, f, indent=1)
    write_md(os.path.join(a.out, "closest_tris.md"), doc)


if __name__ == "__main__":
    main()
