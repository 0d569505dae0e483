#!/usr/bin/env python3
"""time of bvh_radius_search, with bvh_knn(k = 32) and bvh_closest_point BVH_QUERY_ANY on the same tree and points beside every row; one process, one device.

For each mesh (Sponza-like 262 144, uniform 10 M) and builder (all four): one build, then --points near-surface points (vertices jittered by 1e-3 of the
scene extent) at four radii, one per target in --targets: the radius whose mean neighbour count over the first 16 384 points is nearest to 1, 8, 32 and 256,
found by bisection with count-only calls on the first builder's tree and then used for every builder.  Each radius is timed five ways with HIP events on the
context's stream: bvh_closest_point BVH_QUERY_ANY, bvh_knn k = 32, bvh_radius_search count-only (d_hits NULL), count + unsorted fill and count +
BVH_RADIUS_SORTED fill (capacity = the total).  One warm-up call of each, then --windows windows of --reps calls each; the five alternate inside every window
round, so a drift of the machine falls on all of them.  The median window is the figure, the smallest and largest are kept as the spread.  Also recorded:
mean and maximum neighbours per query.  Nothing here is a pass criterion.  Writes <out>/radius.json and <out>/radius.md, stamped with the library's
machine-code hash.

    python tools/time_radius.py                     # both meshes
    python tools/time_radius.py --n 2000000         # one uniform mesh
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
from time_point_query import band_points  # noqa: E402
from time_query import timed  # noqa: E402

WAYS = ("any", "knn32", "count", "fill", "fill_sorted")
CALIBRATE = 16_384


def render(doc):
    out = ["# bvh_radius_search — measured times (MI355X, one device)\n",
           f"`python tools/time_radius.py` (raw rows: `profiles/radius.json`; machine code `{doc['_kernel_source_hash']}`, the `kernel_source_hash` of "
           f"`bench.py`; device {doc['device']}).  {doc['points']:,} near-surface queries per call (vertices jittered by 1e-3 of the extent), one radius per "
           f"target mean neighbour count.  HIP events on the context's stream, one warm-up call, then {doc['windows']} windows of {doc['reps']} calls, the "
           "five calls alternating; ms per call, median window (smallest – largest).  any = `bvh_closest_point` `BVH_QUERY_ANY`, knn32 = `bvh_knn` k = 32, on "
           "the same tree and points; count = `d_hits` NULL; fill / sorted fill = count + fill with capacity = the total.  None of these times is a pass "
           "criterion.\n",
           "| mesh | builder (layout) | target | radius | neighbours mean | max | any | knn k=32 | count only | count + fill | count + sorted fill |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        def cell(w):
            t = r[w + "_ms"]
            return f"{t['median']:.3f} ({t['min']:.3f} – {t['max']:.3f})"
        out.append(f"| {r['mesh']} | {r['builder']} ({r['layout']}) | {r['target']} | {r['radius']:.5g} | {r['mean_count']:.2f} | {r['max_count']} | {cell('any')} | "
                   f"{cell('knn32')} | {cell('count')} | {cell('fill')} | {cell('fill_sorted')} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one uniform mesh of this size instead of the default two")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--targets", type=float, nargs="+", default=[1, 8, 32, 256], help="mean neighbour counts to aim the radii at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    meshes = [("uniform", a.n)] if a.n else [("sponza", 262_144), ("uniform", 10_000_000)]
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    rows = []
    doc = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "points": a.points,
           "targets": a.targets, "rows": rows}

    def dump():
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "radius.json"), "w") as f:
            json.dump(doc, f, indent=1)
        with open(os.path.join(a.out, "radius.md"), "w") as f:
            f.write(render(doc))

    m = a.points
    for kind, n in meshes:
        tris = pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 1)
        v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        ext = float((hi - lo).max())
        ctx.reserve(n)
        d_tris = ctx.upload(tris)
        pts = band_points(pkg, tris, lo, hi, m, 1)
        d_pts, d_off = ctx.alloc(m * 16), ctx.alloc((m + 1) * 4)
        d_any, d_knn, d_cnt = ctx.alloc(m * 32), ctx.alloc(m * 32 * 8), ctx.alloc(m * 4)
        radii = {}
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
            res = b.result

            def mean_count(radius, k=min(CALIBRATE, m)):
                pts["radius"] = np.float32(radius); d_pts.upload(pts)
                total = C.c_uint64()
                assert L.bvh_radius_search(ctx.handle, C.byref(res), None, d_pts.ptr, k, 0, d_off.ptr, None, 0, C.byref(total)) == 0
                return total.value / k
            for target in a.targets:
                if target not in radii:                                     # bisection on log(radius): the mean count grows with the radius
                    r_lo, r_hi = 1e-6 * ext, 2.0 * ext
                    for _ in range(40):
                        mid = float(np.sqrt(r_lo * r_hi))
                        if mean_count(mid) < target:
                            r_lo = mid
                        else:
                            r_hi = mid
                    radii[target] = r_hi
                pts["radius"] = np.float32(radii[target]); d_pts.upload(pts)
                total = C.c_uint64()
                assert L.bvh_radius_search(ctx.handle, C.byref(res), None, d_pts.ptr, m, 0, d_off.ptr, None, 0, C.byref(total)) == 0
                total = int(total.value)
                counts = np.diff(d_off.download(np.uint32, m + 1).astype(np.int64))
                d_hits = ctx.alloc(max(total, 1) * 8)
                work = {
                    "any": lambda i: L.bvh_closest_point(ctx.handle, C.byref(res), None, d_pts.ptr, m, d_any.ptr, pkg.QUERY_ANY),
                    "knn32": lambda i: L.bvh_knn(ctx.handle, C.byref(res), None, d_pts.ptr, m, 32, d_knn.ptr, d_cnt.ptr),
                    "count": lambda i: L.bvh_radius_search(ctx.handle, C.byref(res), None, d_pts.ptr, m, 0, d_off.ptr, None, 0, None),
                    "fill": lambda i: L.bvh_radius_search(ctx.handle, C.byref(res), None, d_pts.ptr, m, 0, d_off.ptr, d_hits.ptr, total, None),
                    "fill_sorted": lambda i: L.bvh_radius_search(ctx.handle, C.byref(res), None, d_pts.ptr, m, pkg.RADIUS_SORTED, d_off.ptr, d_hits.ptr, total, None),
                }
                for w in WAYS:
                    assert work[w](0) == 0                                  # warm-up: every shape the windows use
                times = {w: [] for w in WAYS}
                for _ in range(a.windows):
                    for w in WAYS:                                          # alternating
                        times[w].append(timed(stream, work[w], a.reps))
                row = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(res.layout), "target": target, "radius": radii[target],
                       "n_points": m, "total": total, "mean_count": float(counts.mean()), "max_count": int(counts.max())}
                for w in WAYS:
                    t = times[w]
                    row[w + "_ms"] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "windows": t}
                rows.append(row)
                print(json.dumps(row), flush=True)
                dump()
                d_hits.free()
        for buf in (d_tris, d_pts, d_off, d_any, d_knn, d_cnt):
            buf.free()
    ctx.close()
    dump()


if __name__ == "__main__":
    main()
