#!/usr/bin/env python3
"""time of bvh_radius_tris, with bvh_closest_tris (closest and any, in the band) and bvh_intersect_tris (count only) on the same pair of meshes as the context;
one process, one device.

For each mesh — bunny-like 327 680 and Sponza-like 262 144, each against a copy of itself moved by (0.37, 0.11, -0.23) of its extent, the pair
tools/time_closest_tris.py uses — and each builder (single-pass LBVH: layout 0; HPLOC: layout 1): one build of the tree over the mesh, the moved copy as the
queries, then at the radii band = 2e-3 of the extent's diagonal and 10 x band
  count                             d_hits NULL
  unsorted                          count + fill, flags 0, the exact capacity
  sorted                            count + fill, BVH_RADIUS_TRIS_SORTED, the exact capacity (quadratic in a slice's length: left out, and said so, where the
                                    longest slice exceeds --max-sorted-slice)
and at band only
  self                              BVH_RADIUS_TRIS_SELF | BVH_RADIUS_TRIS_SKIP_SHARED, count + unsorted fill, the tree's own mesh
  closest_band / any_band           bvh_closest_tris at the same radius
  tris                              bvh_intersect_tris, count only
are timed with HIP events on the context's stream: one warm-up call each, then --windows windows of --reps calls; the median window is the figure, the
smallest and largest are kept as the spread.  The workloads alternate inside every window round, so a drift of the machine falls on all of them.  Also
recorded: records, longest slice and crossings (feature 15) per radius, and the number of box pairs that reach the leaf routine — counted on the host for a
strided sample of --sample queries (bvh_overlap with the query boxes inflated by the radius gives the candidates, query.hpp's box_box_dist_pass restated in
f32 decides) and scaled to all queries: that, not the record count, is what the time of the walk should track.
Writes <out>/radius_tris.json and <out>/radius_tris.md.  These are reported numbers, not gates: there is no earlier figure to compare with.

    python tools/time_radius_tris.py
    python tools/time_radius_tris.py --n 20000      # both meshes at this size
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
F32 = np.float32
GROW = F32(2.0 ** -16)


def leaf_pairs(b, v, moved, radius, sample):
    """how many (query, tree triangle) pairs of the sampled queries pass box_box_dist_pass on their two stage-E boxes against radius^2 — the pairs that reach
    the leaf routine (the test is monotone under containment, so every box above such a leaf passes too)"""
    q = moved[sample]
    qlo, qhi = q.min(axis=1), q.max(axis=1)
    g = GROW * np.maximum(np.abs(qlo), np.abs(qhi)).max(axis=1, keepdims=True)
    qlo, qhi = (qlo - g).astype(F32), (qhi + g).astype(F32)
    tlo_all, thi_all = v.min(axis=1), v.max(axis=1)
    pad = np.float64(radius) * (1.0 + 1e-5) + 2.0 ** -15 * float(np.abs(v).max())                # the radius and the tree boxes' own growth, with room
    boxes = np.concatenate([qlo.astype(np.float64) - pad, qhi.astype(np.float64) + pad], axis=1).astype(F32)
    total = 0
    r2 = F32(radius) * F32(radius)
    for s in range(0, len(sample), 512):                                                         # (in pieces: a wall-sized query has many candidates)
        off, prims = b.overlap(boxes[s:s + 512])
        r = s + np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
        tlo, thi = tlo_all[prims], thi_all[prims]
        gt = GROW * np.maximum(np.abs(tlo), np.abs(thi)).max(axis=1, keepdims=True)
        d = np.maximum(np.maximum((tlo - gt) - qhi[r], qlo[r] - (thi + gt)), F32(0.0)).astype(F32)
        lb = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        total += int((lb * (F32(1.0) - F32(2.0 ** -20)) <= r2).sum())
    return total


def write_md(path, doc):
    def cell(t):
        return "not measured" if t is None else f"{t['median']:.3f} [{t['min']:.3f} .. {t['max']:.3f}]"

    def ratio(a, b):
        return "-" if a is None or b is None else f"{a['median'] / b['median']:.2f}"
    out = ["# bvh_radius_tris: every triangle within a radius, mesh to mesh (tools/time_radius_tris.py)", "",
           f"{doc['device']}; the queries are the tree's own mesh moved by {SHIFT} of its extent, one query per triangle; HIP events on the context's stream, one "
           f"warm-up call, then {doc['windows']} windows of {doc['reps']} calls; median window per call in ms, [smallest .. largest window].  band: radius 2e-3 "
           "of the extent's diagonal.  `count`: d_hits NULL; `unsorted` / `sorted`: count + fill with the exact capacity (the sorted fill is quadratic in a "
           f"slice's length and is left out where the longest slice exceeds {doc['max_sorted_slice']:,}).  Leaf pairs: the box pairs that reach the leaf routine, "
           f"counted on the host for a strided sample of {doc['sample']:,} queries and scaled.  Reported numbers, not gates.  Library: {doc['library']}.", "",
           "| mesh | builder | radius | count ms | unsorted ms | sorted ms | records | longest slice | crossings | leaf pairs (est.) | count ns / leaf pair | "
           "unsorted / count | sorted / unsorted |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        for label in ("band", "band10"):
            w = r[label]
            per = w["count_ms"]["median"] * 1e6 / w["leaf_pairs"] if w["leaf_pairs"] else float("nan")
            out.append(f"| {r['mesh']} | {r['builder']} | {label} ({w['radius']:.4g}) | {cell(w['count_ms'])} | {cell(w['unsorted_ms'])} | {cell(w['sorted_ms'])} | "
                       f"{w['records']:,} | {w['longest']:,} | {w['crossings']:,} | {w['leaf_pairs']:,} | {per:.2f} | {ratio(w['unsorted_ms'], w['count_ms'])} | "
                       f"{ratio(w['sorted_ms'], w['unsorted_ms'])} |")
    out += ["", "At band, on the same inputs in the same windows: the self mode (`BVH_RADIUS_TRIS_SELF | BVH_RADIUS_TRIS_SKIP_SHARED`, count + unsorted fill, the "
            "tree's own mesh), `bvh_closest_tris` closest and any, `bvh_intersect_tris` count only.", "",
            "| mesh | builder | self ms | self records | closest band ms | any band ms | tris (count) ms | count / closest band | count / any band | count / tris |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        c = r["band"]["count_ms"]
        out.append(f"| {r['mesh']} | {r['builder']} | {cell(r['self_ms'])} | {r['self_records']:,} | {cell(r['closest_band_ms'])} | {cell(r['any_band_ms'])} | "
                   f"{cell(r['tris_ms'])} | {ratio(c, r['closest_band_ms'])} | {ratio(c, r['any_band_ms'])} | {ratio(c, r['tris_ms'])} |")
    out.append("")
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="both meshes at this size instead of 327 680 / 262 144")
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sample", type=int, default=8192, help="queries of the host-side leaf-pair count")
    ap.add_argument("--max-sorted-slice", type=int, default=4096, help="the sorted fill is not run where the longest slice is longer")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    S, SELF = pkg.RADIUS_TRIS_SORTED, pkg.RADIUS_TRIS_SELF | pkg.RADIUS_TRIS_SKIP_SHARED
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
        sample = np.arange(0, n, max(1, n // a.sample))[: a.sample]
        ctx.reserve(n)
        d_tris, d_other = ctx.upload(tris), ctx.upload(other)
        d_one, d_off = ctx.alloc(n * 16), ctx.alloc((n + 1) * 4)
        qin = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_other.ptr, None, None, 0, 0)
        for algo in (1, 3):
            b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
            res = b.result
            row = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(res.layout), "height": tree_height(pkg, b)}

            def radius_tris(radius, flags, queries, d_hits, cap):
                def fn(i):
                    assert L.bvh_radius_tris(ctx.handle, C.byref(res), None, C.byref(queries) if queries is not None else None, n, radius, flags, d_off.ptr,
                                             d_hits.ptr if d_hits is not None else None, cap, None) == 0
                return fn

            def counted(radius, flags, queries):
                total = C.c_uint64()
                assert L.bvh_radius_tris(ctx.handle, C.byref(res), None, C.byref(queries) if queries is not None else None, n, radius, flags, d_off.ptr, None, 0,
                                         C.byref(total)) == 0
                return int(total.value), int(np.diff(d_off.download(np.uint32, n + 1).astype(np.int64)).max())

            def closest(radius, q):
                def fn(i):
                    assert L.bvh_closest_tris(ctx.handle, C.byref(res), None, C.byref(qin), n, radius, d_one.ptr, q) == 0
                return fn

            def tris_count(i):
                assert L.bvh_intersect_tris(ctx.handle, C.byref(res), None, C.byref(qin), n, pkg.TRIS_QUERY, d_off.ptr, None, 0, None) == 0
            work, bufs = [], []
            for label, radius in (("band", band), ("band10", 10.0 * band)):
                total, longest = counted(radius, 0, qin)
                d_hits = ctx.alloc(max(total, 1) * 16); bufs.append(d_hits)
                w = row[label] = {"radius": radius, "records": total, "longest": longest, "leaf_pairs": int(round(leaf_pairs(b, v, moved, radius, sample) * n / len(sample)))}
                work += [(label, "count_ms", radius_tris(radius, 0, qin, None, 0)), (label, "unsorted_ms", radius_tris(radius, 0, qin, d_hits, total))]
                if longest <= a.max_sorted_slice:
                    work.append((label, "sorted_ms", radius_tris(radius, S, qin, d_hits, total)))
                else:
                    w["sorted_ms"] = None
                radius_tris(radius, 0, qin, d_hits, total)(0)
                w["crossings"] = int((d_hits.download(pkg.TRI_HIT, total)["feature"] == 15).sum()) if total else 0
            self_total, self_longest = counted(band, SELF, None)
            d_self = ctx.alloc(max(self_total, 1) * 16); bufs.append(d_self)
            row["self_records"], row["self_longest"] = self_total, self_longest
            work += [(None, "self_ms", radius_tris(band, SELF, None, d_self, self_total)), (None, "closest_band_ms", closest(band, pkg.QUERY_CLOSEST)),
                     (None, "any_band_ms", closest(band, pkg.QUERY_ANY)), (None, "tris_ms", tris_count)]
            for _, _, fn in work:
                fn(0)                                                           # warm-up: every shape the windows use
            times = {(label, name): [] for label, name, _ in work}
            for _ in range(a.windows):
                for label, name, fn in work:                                    # alternating
                    times[(label, name)].append(timed(stream, fn, a.reps))
            for (label, name), t in times.items():
                (row[label] if label else row)[name] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "windows": t}
            # per-kernel split of the count + unsorted fill at band
            ctx.set_profiling(2)
            for i in range(3):
                work[1][2](i)
            kt = ctx.kernel_times()
            ctx.set_profiling(0)
            row["kernels_unsorted_band"] = {name: (ms / cnt, cnt) for name, (ms, cnt) in kt.items()}
            rows.append(row)
            print(json.dumps({k: val for k, val in row.items() if not k.startswith("kernels_")}), flush=True)
            for buf in bufs:
                buf.free()
        for buf in (d_tris, d_other, d_one, d_off):
            buf.free()
    ctx.close()
    os.makedirs(a.out, exist_ok=True)
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "sample": a.sample, "max_sorted_slice": a.max_sorted_slice,
           "library": os.path.relpath(pkg.LIB_PATH, ROOT), "rows": rows}
    with open(os.path.join(a.out, "radius_tris.json"), "w") as f:
        json.dump(doc, f, indent=1)
    write_md(os.path.join(a.out, "radius_tris.md"), doc)


if __name__ == "__main__":
    main()
