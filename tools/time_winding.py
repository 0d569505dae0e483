#!/usr/bin/env python3
"""time of bvh_winding_prepare and bvh_winding_number, with bvh_closest_point and a count-only bvh_intersect_all parity test on the same tree and points as
the yardsticks; one process, one device.

For each mesh and builder (all four): one build, one bvh_winding_prepare (timed on its own), then --points uniform points in the scene box grown by a quarter
of its extent on every side.  Timed with HIP events on the context's stream, one warm-up call, then --windows windows of --reps calls each, in alternation
inside every window round so that a drift of the machine falls on all of them; the median window is the figure, the smallest and largest are the spread:
  winding b   bvh_winding_number at beta = 2, 3, 4
  closest     bvh_closest_point BVH_QUERY_CLOSEST, infinite radius (the distance a signed distance needs anyway)
  parity      bvh_intersect_all, count only (d_hits NULL), one ray per point along +x: the crossing-number inside / outside test
Also recorded: the share of points on which w > 0.5 at beta 2 and 3 agrees with beta 4, the share on which the crossing parity agrees with beta 4, and the
per-kernel split (k_winding / k_winding_deep, k_winding_climb / k_winding_finish) from bvh_ctx_kernel_times.
Writes <out>/winding.json and <out>/winding.md.

    python tools/time_winding.py                  # bunny-like 5 120 and 327 680, uniform 10 M
    python tools/time_winding.py --n 2000000      # one uniform mesh
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

BETAS = (2.0, 3.0, 4.0)


def write_md(path, doc):
    rows = doc["rows"]
    out = ["# bvh_winding_number: generalized winding numbers (tools/time_winding.py)", "",
           f"{doc['device']}; {doc['points']:,} points per call, uniform in the scene box grown by a quarter of its extent; HIP events on the context's stream, one "
           f"warm-up call, then {doc['windows']} windows of {doc['reps']} calls in alternation; median window per call in ms, [smallest .. largest window].  "
           "`closest` is `bvh_closest_point` `BVH_QUERY_CLOSEST` with an infinite radius, `parity` a count-only `bvh_intersect_all` of one +x ray per point.  "
           f"Library: {doc['library']}.", "",
           "| mesh | builder | prepare ms | beta 2 ms | beta 3 ms | beta 4 ms | closest ms | parity ms | beta 2 / closest | beta 2 ns/point |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        def cell(name):
            t = r[f"{name}_ms"]
            return f"{t['median']:.3f} [{t['min']:.3f} .. {t['max']:.3f}]"
        b2, cp = r["beta2_ms"]["median"], r["closest_ms"]["median"]
        out.append(f"| {r['mesh']} | {r['builder']} | {cell('prepare')} | {cell('beta2')} | {cell('beta3')} | {cell('beta4')} | {cell('closest')} | {cell('parity')} | "
                   f"{b2 / cp:.2f} | {b2 * 1e6 / doc['points']:.1f} |")
    out += ["", "## agreement of the inside / outside answer with beta 4 (share of the points)", "",
            "| mesh | builder | beta 2 | beta 3 | crossing parity | inside share at beta 4 | k_winding_deep share of a beta 2 call |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        deep = r["beta2_deep_share"]
        out.append(f"| {r['mesh']} | {r['builder']} | {r['agree_beta2']:.6f} | {r['agree_beta3']:.6f} | {r['agree_parity']:.6f} | {r['inside_share']:.4f} | "
                   f"{'n/a' if deep is None else f'{deep:.4f}'} |")
    out += ["", "(The uniform mesh is a triangle soup: it has no inside, the winding number there is a smooth field and the parity of a soup means nothing; its rows "
            "are for the time only.  Trees of height " + ", ".join(sorted({str(r['height']) for r in rows})) + ": no query reaches the stackless pass, and the "
            "`k_winding_deep` share is the launch that returns at once.)", ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one uniform mesh of this size instead of the default three")
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    meshes = [("uniform", a.n)] if a.n else [("bunny", 5_120), ("bunny", 327_680), ("uniform", 10_000_000)]
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    rows = []
    m = a.points
    for kind, n in meshes:
        tris = pkg.meshgen.bunny_like(n) if kind == "bunny" else pkg.meshgen.uniform(n, 1)
        v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        ext = hi - lo
        rng = np.random.default_rng(4)
        pts = np.zeros(m, dtype=pkg.POINT_QUERY)
        pts["point"] = (lo - 0.25 * ext + rng.random((m, 3)) * 1.5 * ext).astype(np.float32)
        pts["radius"] = np.inf
        rays = np.zeros(m, dtype=pkg.RAY)
        rays["origin"] = pts["point"]; rays["direction"] = (1.0, 0.0, 0.0); rays["tmin"] = 0.0; rays["tmax"] = np.inf
        ctx.reserve(n)
        d_tris, d_pts, d_rays = ctx.upload(tris), ctx.upload(pts), ctx.upload(rays)
        d_w, d_cp, d_off, d_mom = ctx.alloc(m * 4), ctx.alloc(m * 32), ctx.alloc((m + 1) * 4), ctx.alloc((n - 1) * 32)
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
            res = b.result
            row = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(res.layout), "height": tree_height(pkg, b)}

            def prep(i):
                assert L.bvh_winding_prepare(ctx.handle, C.byref(res), None, d_mom.ptr) == 0

            def wind(beta):
                def fn(i):
                    assert L.bvh_winding_number(ctx.handle, C.byref(res), None, d_mom.ptr, d_pts.ptr, m, beta, d_w.ptr) == 0
                return fn

            def closest(i):
                assert L.bvh_closest_point(ctx.handle, C.byref(res), None, d_pts.ptr, m, d_cp.ptr, pkg.QUERY_CLOSEST) == 0

            def parity(i):
                assert L.bvh_intersect_all(ctx.handle, C.byref(res), None, d_rays.ptr, m, 0, d_off.ptr, None, 0, None) == 0
            work = [("prepare", prep)] + [(f"beta{int(bt)}", wind(bt)) for bt in BETAS] + [("closest", closest), ("parity", parity)]
            for _, fn in work:
                fn(0)                                                           # warm-up: every shape the windows use
            times = {name: [] for name, _ in work}
            for _ in range(a.windows):
                for name, fn in work:                                           # alternating
                    times[name].append(timed(stream, fn, a.reps))
            for name, t in times.items():
                row[f"{name}_ms"] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "windows": t}
            # answers: inside / outside at each beta and by crossing parity
            inside = {}
            for bt in BETAS:
                wind(bt)(0)
                inside[bt] = d_w.download(np.float32, m) > np.float32(0.5)
            parity(0)
            off = d_off.download(np.uint32, m + 1).astype(np.int64)
            odd = (np.diff(off) & 1) == 1
            row["agree_beta2"] = float((inside[2.0] == inside[4.0]).mean()); row["agree_beta3"] = float((inside[3.0] == inside[4.0]).mean())
            row["agree_parity"] = float((odd == inside[4.0]).mean()); row["inside_share"] = float(inside[4.0].mean())
            # per-kernel split of the prepare and of the beta 2 call
            ctx.set_profiling(2)
            prep(0)
            for i in range(3):
                wind(2.0)(i)
            kt = ctx.kernel_times()
            ctx.set_profiling(0)
            row["kernels"] = {name: (ms / cnt, cnt) for name, (ms, cnt) in kt.items()}
            main_ms = kt.get("k_winding", (0.0, 1))[0]; deep_ms = kt.get("k_winding_deep", (0.0, 1))[0]
            row["beta2_deep_share"] = deep_ms / (main_ms + deep_ms) if main_ms + deep_ms > 0 else None
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "kernels"}), flush=True)
        for buf in (d_tris, d_pts, d_rays, d_w, d_cp, d_off, d_mom):
            buf.free()
    ctx.close()
    os.makedirs(a.out, exist_ok=True)
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "points": m,
           "library": os.path.relpath(pkg.LIB_PATH, ROOT), "rows": rows}
    with open(os.path.join(a.out, "winding.json"), "w") as f:
        json.dump(doc, f, indent=1)
    write_md(os.path.join(a.out, "winding.md"), doc)


if __name__ == "__main__":
    main()
