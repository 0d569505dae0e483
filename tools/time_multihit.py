#!/usr/bin/env python3
"""time of bvh_intersect_all, with bvh_intersect closest-hit on the same tree and rays beside every row; one process, one device.

For each mesh (Sponza-like 262 144, uniform 10 M) and builder (all four): one build, then two ray sets — 1024^2 camera rays (cornell_view) and 1 M random
through-rays (from a sphere around the scene through a random point of its box, no tmax) — each timed four ways with HIP events on the context's stream:
bvh_intersect BVH_QUERY_CLOSEST, bvh_intersect_all count-only (d_hits NULL), count + unsorted fill and count + BVH_HITS_SORTED fill (capacity = the total).
One warm-up call of each, then --windows windows of --reps calls each; the four alternate inside every window round, so a drift of the machine falls on all
of them.  The median window is the figure, the smallest and largest are kept as the spread.  Also recorded: mean and maximum hits per ray.  The number to
read is count-only / closest per row.  Writes <out>/multihit.json and <out>/multihit.md, stamped with the library's machine-code hash.

    python tools/time_multihit.py                     # both meshes
    python tools/time_multihit.py --n 2000000         # one uniform mesh
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
from time_query import timed  # noqa: E402

WAYS = ("closest", "count", "fill", "fill_sorted")


def through_rays(pkg, lo, hi, m, seed):
    rng = np.random.default_rng(seed)
    ext = hi - lo
    centre, radius = 0.5 * (lo + hi), float(np.linalg.norm(ext))
    u = rng.normal(size=(m, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = centre + radius * u
    d = (lo + rng.random((m, 3)) * ext) - o
    r = np.zeros(m, dtype=pkg.RAY)
    r["origin"] = o.astype(np.float32); r["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    r["tmax"] = np.float32(3.0e38)
    return r


def render(doc):
    out = ["# bvh_intersect_all — measured times (MI355X, one device)\n",
           f"`python tools/time_multihit.py` (raw rows: `profiles/multihit.json`; machine code `{doc['_kernel_source_hash']}`, the `kernel_source_hash` of "
           f"`bench.py`; device {doc['device']}).  camera = {doc['width']}² rays of the Cornell view, through = {doc['through']:,} rays from a sphere around "
           f"the scene through a random point of its box, no tmax.  HIP events on the context's stream, one warm-up call, then {doc['windows']} windows of "
           f"{doc['reps']} calls, the four calls alternating; ms per call, median window (smallest – largest).  closest = `bvh_intersect` `BVH_QUERY_CLOSEST` "
           "on the same tree and rays; count = `d_hits` NULL; fill / sorted fill = count + fill with capacity = the total.  None of these times is a pass "
           "criterion.\n",
           "| mesh | builder (layout) | rays | hits / ray mean | max | closest | count only | count / closest | count + fill | count + sorted fill |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        def cell(w):
            t = r[w + "_ms"]
            return f"{t['median']:.3f} ({t['min']:.3f} – {t['max']:.3f})"
        out.append(f"| {r['mesh']} | {r['builder']} ({r['layout']}) | {r['rays']} | {r['mean_hits']:.2f} | {r['max_hits']} | {cell('closest')} | {cell('count')} | "
                   f"{r['count_over_closest']:.2f} | {cell('fill')} | {cell('fill_sorted')} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one uniform mesh of this size instead of the default two")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--through", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    meshes = [("uniform", a.n)] if a.n else [("sponza", 262_144), ("uniform", 10_000_000)]
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    rows = []
    doc = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "width": a.width,
           "through": a.through, "rows": rows}

    def dump():
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "multihit.json"), "w") as f:
            json.dump(doc, f, indent=1)
        with open(os.path.join(a.out, "multihit.md"), "w") as f:
            f.write(render(doc))

    cam, _ = pkg.cornell_view()
    for kind, n in meshes:
        tris = pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 1)
        v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        ctx.reserve(n)
        d_tris = ctx.upload(tris)
        d_cam = ctx.alloc(a.width * a.width * 32)
        assert L.bvh_generate_rays(ctx.handle, np.ascontiguousarray(cam).ctypes.data, d_cam.ptr, a.width, a.width) == 0
        sets = {"camera": (d_cam, a.width * a.width), "through": (ctx.upload(through_rays(pkg, lo, hi, a.through, 3)), a.through)}
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
            res = b.result
            for name, (d_rays, m) in sets.items():
                d_off, d_one = ctx.alloc((m + 1) * 4), ctx.alloc(m * 16)
                total = C.c_uint64()
                assert L.bvh_intersect_all(ctx.handle, C.byref(res), None, d_rays.ptr, m, 0, d_off.ptr, None, 0, C.byref(total)) == 0
                total = int(total.value)
                counts = np.diff(d_off.download(np.uint32, m + 1).astype(np.int64))
                d_hits = ctx.alloc(max(total, 1) * 16)
                work = {
                    "closest": lambda i: L.bvh_intersect(ctx.handle, C.byref(res), None, d_rays.ptr, m, d_one.ptr, pkg.QUERY_CLOSEST),
                    "count": lambda i: L.bvh_intersect_all(ctx.handle, C.byref(res), None, d_rays.ptr, m, 0, d_off.ptr, None, 0, None),
                    "fill": lambda i: L.bvh_intersect_all(ctx.handle, C.byref(res), None, d_rays.ptr, m, 0, d_off.ptr, d_hits.ptr, total, None),
                    "fill_sorted": lambda i: L.bvh_intersect_all(ctx.handle, C.byref(res), None, d_rays.ptr, m, pkg.HITS_SORTED, d_off.ptr, d_hits.ptr, total, None),
                }
                for w in WAYS:
                    assert work[w](0) == 0                                  # warm-up: every shape the windows use
                times = {w: [] for w in WAYS}
                for _ in range(a.windows):
                    for w in WAYS:                                          # alternating
                        times[w].append(timed(stream, work[w], a.reps))
                row = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(res.layout), "rays": name, "n_rays": m, "total": total,
                       "mean_hits": float(counts.mean()), "max_hits": int(counts.max())}
                for w in WAYS:
                    t = times[w]
                    row[w + "_ms"] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "windows": t}
                row["count_over_closest"] = row["count_ms"]["median"] / row["closest_ms"]["median"]
                rows.append(row)
                print(json.dumps(row), flush=True)
                dump()
                for buf in (d_off, d_one, d_hits):
                    buf.free()
        for buf in [d_tris] + [s[0] for s in sets.values()]:
            buf.free()
    ctx.close()
    dump()


if __name__ == "__main__":
    main()
