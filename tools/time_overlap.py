#!/usr/bin/env python3
"""time of bvh_overlap, with bvh_closest_point any-hit queries of the same footprint on the same tree for orientation; one process, one device.

For each mesh and builder (all four): one build, then up to --boxes query boxes per workload — centres uniform in the scene box, half-widths a random fraction of
2 % / 10 % / 50 % of the scene extent per axis (small / medium / large), and a mixed set with a third of each in random order (and the same mixed set sorted by
size on the host) — timed with HIP events around --reps calls on the context's stream, count-only (d_prims NULL) and count + fill (capacity = the total), the two
alternating.  A scene-sized box touches a large share of the mesh (a "large" box about an eighth of it: 1 M of them on 10 M triangles would be 10^12 results per
call), so each workload is first counted with a pilot of 4096 boxes and then uses min(--boxes, --target-results / mean results per query) boxes, at least 4096: the
row records the number, and times are also given per query.  Beside each count-only time: bvh_closest_point BVH_QUERY_ANY for the same number of queries at the boxes' centres, radius = the box's half-diagonal.
BVH_OVERLAP_SELF on each mesh (d_boxes = the tree's own primitive boxes), and on the Sponza-like mesh the same queries after a bvh_refit of a jittered mesh and
after bvh_optimize(3).  A workload whose total exceeds --max-total results is timed count-only.  Writes <out>/overlap.json and <out>/overlap.md.

    python tools/time_overlap.py                      # Sponza-like 262 144 and uniform 10 M
    python tools/time_overlap.py --n 2000000          # one uniform mesh
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bvh_pkg  # noqa: E402
from _srchash import kernel_source_hash  # noqa: E402
from time_query import timed  # noqa: E402

SIZES = (("small", 0.02), ("medium", 0.10), ("large", 0.50))


def query_boxes(pkg, lo, hi, m, frac, seed):
    rng = np.random.default_rng(seed)
    ext = hi - lo
    c = lo + rng.random((m, 3)) * ext
    f = np.asarray(frac, dtype=np.float64).reshape(-1, 1) if np.ndim(frac) else frac
    h = rng.random((m, 3)) * f * ext
    b = np.zeros(m, dtype=pkg.AABB)
    b["min"] = (c - h).astype(np.float32); b["max"] = (c + h).astype(np.float32)
    return b


def centre_points(pkg, boxes):
    p = np.zeros(len(boxes), dtype=pkg.POINT_QUERY)
    lo, hi = boxes["min"].astype(np.float64), boxes["max"].astype(np.float64)
    p["point"] = (0.5 * (lo + hi)).astype(np.float32)
    p["radius"] = (0.5 * np.linalg.norm(hi - lo, axis=1)).astype(np.float32)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one uniform mesh of this size instead of the default two")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--boxes", type=int, default=1_000_000)
    ap.add_argument("--target-results", type=int, default=1 << 28, help="results per call a workload is sized for (its number of boxes shrinks to meet it)")
    ap.add_argument("--budget-s", type=float, default=0.5, help="seconds one round of timed calls may take: calls longer than budget / reps are repeated less often (at least twice)")
    ap.add_argument("--max-total", type=int, default=1 << 30, help="largest result count that is filled (4 bytes each)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    meshes = [("uniform", a.n)] if a.n else [("sponza", 262_144), ("uniform", 10_000_000)]
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    m = a.boxes
    rows = []

    TOO_LARGE = -10002

    def count_total(res, d_boxes, k, mode, d_off):
        """one count-only call that reads the total back: a total of 2^32 or more is reported with BVH_E_TOO_LARGE and is still the total"""
        total = C.c_uint64()
        rc = L.bvh_overlap(ctx.handle, C.byref(res), d_boxes, k, mode, d_off.ptr, None, 0, C.byref(total))
        assert rc in (0, TOO_LARGE), rc
        return int(total.value)

    def sized(res, d_boxes, k_max, mode):
        """the number of boxes (a prefix of the set) this workload runs with: a pilot of 4096 gives the mean results per query"""
        pilot = min(4096, k_max)
        d_off = ctx.alloc((pilot + 1) * 4)
        mean = count_total(res, d_boxes, pilot, mode, d_off) / pilot
        d_off.free()
        return int(min(k_max, max(pilot, a.target_results / max(mean, 1e-9))))

    def measure(res, d_boxes, k, mode, reps):
        """-> dict(boxes, total, count_ms, fill_ms or None): count-only and count + fill alternate, two rounds of reps each after one warm call"""
        d_off = ctx.alloc((k + 1) * 4)
        total = count_total(res, d_boxes, k, mode, d_off)
        t0 = time.perf_counter()
        count_total(res, d_boxes, k, mode, d_off)                     # (warm now; the call waits for the total, so the host clock sees its length)
        reps = int(min(reps, max(2, a.budget_s / max(time.perf_counter() - t0, 1e-6))))     # long calls (scene-sized boxes) get fewer repetitions
        out = {"boxes": k, "total": total, "mean_results": total / k, "reps": reps}
        cnt = lambda i: L.bvh_overlap(ctx.handle, C.byref(res), d_boxes, k, mode, d_off.ptr, None, 0, None)
        d_prims = ctx.alloc(max(total, 1) * 4) if total <= min(a.max_total, 0xFFFFFFFF) else None
        fill = (lambda i: L.bvh_overlap(ctx.handle, C.byref(res), d_boxes, k, mode, d_off.ptr, d_prims.ptr, total, None)) if d_prims else None
        if fill:
            assert fill(0) == 0
        c_ms, f_ms = [], []
        for _ in range(2):
            c_ms.append(timed(stream, cnt, reps))
            if fill:
                f_ms.append(timed(stream, fill, reps))
        out["count_ms"] = min(c_ms); out["count_ms_runs"] = c_ms
        out["count_us_per_query"] = out["count_ms"] * 1e3 / k
        out["fill_ms"] = min(f_ms) if fill else None; out["fill_ms_runs"] = f_ms
        if fill:
            out["results_per_s"] = total / out["fill_ms"] * 1e3
        d_off.free()
        if d_prims:
            d_prims.free()
        return out

    def dump():
        os.makedirs(a.out, exist_ok=True)
        doc = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "boxes": m, "target_results": a.target_results, "budget_s": a.budget_s,
               "rows": rows}
        with open(os.path.join(a.out, "overlap.json"), "w") as f:
            json.dump(doc, f, indent=1)
        with open(os.path.join(a.out, "overlap.md"), "w") as f:
            f.write(render(doc))

    for kind, n in meshes:
        tris = pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 1)
        v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        ctx.reserve(n)
        d_tris = ctx.upload(tris)
        sets = {name: query_boxes(pkg, lo, hi, m, frac, 1 + i) for i, (name, frac) in enumerate(SIZES)}
        rng = np.random.default_rng(7)
        mixed_frac = np.array([f for _, f in SIZES])[rng.integers(0, 3, size=m)]
        sets["mixed"] = query_boxes(pkg, lo, hi, m, mixed_frac, 5)
        d_sets = {k: ctx.upload(b) for k, b in sets.items()}
        d_pts = {k: ctx.upload(centre_points(pkg, b)) for k, b in sets.items()}
        d_sorted = ctx.alloc(m * 24)
        d_hits = ctx.alloc(m * 32)
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
            res = b.result
            row = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(res.layout), "state": "built"}
            for name in sets:
                k = sized(res, d_sets[name].ptr, m, pkg.OVERLAP_BOXES)
                row[name] = measure(res, d_sets[name].ptr, k, pkg.OVERLAP_BOXES, a.reps)
                pq = lambda i: L.bvh_closest_point(ctx.handle, C.byref(res), None, d_pts[name].ptr, k, d_hits.ptr, pkg.QUERY_ANY)
                assert pq(0) == 0
                row[name]["point_any_ms"] = timed(stream, pq, a.reps)
            # the mixed set's prefix again, sorted by box volume on the host; and what the same numbers of small / medium / large boxes cost in launches of one size
            k = row["mixed"]["boxes"]
            mx = sets["mixed"][:k]
            vol = np.prod(mx["max"].astype(np.float64) - mx["min"], axis=1)
            d_sorted.upload(mx[np.argsort(vol, kind="stable")])
            row["mixed_sorted"] = measure(res, d_sorted.ptr, k, pkg.OVERLAP_BOXES, a.reps)
            share = np.bincount(np.searchsorted([f for _, f in SIZES], mixed_frac[:k]), minlength=3)
            apart = sum(int(share[j]) * row[s]["count_us_per_query"] for j, (s, _) in enumerate(SIZES)) / 1e3
            row["mixed_over_uniform_sizes"] = row["mixed"]["count_ms"] / apart
            row["mixed_sorted_over_mixed"] = row["mixed_sorted"]["count_ms"] / row["mixed"]["count_ms"]
            row["self"] = measure(res, res.d_prim_aabbs, n, pkg.OVERLAP_SELF, max(a.reps // 2, 2))
            row["self"]["pairs_per_s"] = row["self"]["total"] / (row["self"]["fill_ms"] or row["self"]["count_ms"]) * 1e3
            # the kernels' shares in one count + fill call of the mixed set
            ctx.set_profiling(2)
            cap = row["mixed"]["total"] if row["mixed"]["fill_ms"] is not None else 0      # (a total too large to fill: the count pass's kernels only)
            d_off = ctx.alloc((k + 1) * 4); d_prims = ctx.alloc(cap * 4) if cap else None
            for i in range(3):
                assert L.bvh_overlap(ctx.handle, C.byref(res), d_sets["mixed"].ptr, k, 0, d_off.ptr, d_prims.ptr if d_prims else None, cap, None) == 0
            kt = ctx.kernel_times()
            ctx.set_profiling(0)
            d_off.free()
            if d_prims:
                d_prims.free()
            row["kernels_mixed"] = {k: ms / cnt for k, (ms, cnt) in kt.items()}
            rows.append(row)
            print(json.dumps(row), flush=True)
            dump()
            if kind == "sponza":                                       # the same small / medium sets after a refit of a jittered mesh and after an optimise
                jr = np.random.default_rng(11)
                moved = tris.copy()
                for f in ("v1", "v2", "v3"):
                    moved[f] = (moved[f] + jr.normal(0.0, 1e-3 * float((hi - lo).max()), moved[f].shape)).astype(np.float32)
                for state, step in (("refit", lambda: b.refit(moved)), ("refit + optimize(3)", lambda: b.optimize(3))):
                    step()
                    r2 = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(res.layout), "state": state}
                    for name in ("small", "medium", "mixed"):
                        r2[name] = measure(b.result, d_sets[name].ptr, row[name]["boxes"], pkg.OVERLAP_BOXES, a.reps)
                    r2["self"] = measure(b.result, b.result.d_prim_aabbs, n, pkg.OVERLAP_SELF, max(a.reps // 2, 2))
                    rows.append(r2)
                    print(json.dumps(r2), flush=True)
                    dump()
        for buf in [d_tris, d_hits, d_sorted] + list(d_sets.values()) + list(d_pts.values()):
            buf.free()
    ctx.close()
    dump()


def render(doc):
    def ms(x):
        return "not measured" if x is None else f"{x:.3f}"
    out = ["# bvh_overlap — measured times (MI355X, one device)\n",
           f"`python tools/time_overlap.py` (raw rows: `profiles/overlap.json`; machine code `{doc['_kernel_source_hash']}`, the `kernel_source_hash` of `bench.py`; "
           f"device {doc['device']}).  Query boxes: centres uniform in the scene box, half-widths a random fraction of 2 % (small), 10 % "
           f"(medium) or 50 % (large) of the scene extent per axis; mixed = a third of each in random order.  Each workload runs with {doc['boxes']} boxes, or with "
           f"fewer where that many would report more than {doc['target_results']} results per call (a pilot of 4096 boxes sizes it; the column says how many).  Times are ms per call, the smaller of two rounds of "
           f"{doc['reps']} calls (fewer, at least 2, where a call takes longer than {doc['budget_s'] / doc['reps'] * 1e3:.0f} ms) timed with HIP events on the context's stream, count-only (`d_prims` NULL) and count + fill alternating.  point any = "
           "`bvh_closest_point` `BVH_QUERY_ANY` for the same number of queries at the boxes' centres with radius = the half-diagonal, on the same tree, for "
           "orientation only.  None of these times is a pass criterion.\n",
           "| mesh | builder (layout) | state | set | boxes | mean results / query | count only | count + fill | results / s | point any |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        for name in ("small", "medium", "large", "mixed", "mixed_sorted"):
            if name in r:
                w = r[name]
                rate = f"{w['results_per_s'] / 1e9:.2f} G" if w.get("results_per_s") else "not measured"
                pa = ms(w.get("point_any_ms")) if "point_any_ms" in w else "—"
                out.append(f"| {r['mesh']} | {r['builder']} ({r['layout']}) | {r['state']} | {name} | {w['boxes']} | {w['mean_results']:.2f} | {ms(w['count_ms'])} | {ms(w['fill_ms'])} | {rate} | {pa} |")
    out += ["", "`BVH_OVERLAP_SELF` (`d_boxes` = the tree's own primitive boxes):\n", "| mesh | builder (layout) | state | pairs | count only | count + fill | pairs / s |", "|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        w = r["self"]
        t = w["fill_ms"] or w["count_ms"]
        out.append(f"| {r['mesh']} | {r['builder']} ({r['layout']}) | {r['state']} | {w['total']} | {ms(w['count_ms'])} | {ms(w['fill_ms'])} | {w['total'] / t * 1e3 / 1e6:.1f} M |")
    out += ["", "Divergence (one lane per query): count-only time of the mixed set over the time its small, medium and large boxes take in launches of one size each (their "
            "numbers times the per-query times above), and of the mixed set sorted by box volume on the host over the unsorted mixed set:\n",
            "| mesh | builder | mixed / same boxes in uniform-size launches | sorted mixed / mixed |", "|---|---|---|---|"]
    for r in doc["rows"]:
        if "mixed_over_uniform_sizes" in r:
            out.append(f"| {r['mesh']} | {r['builder']} | {r['mixed_over_uniform_sizes']:.2f} | {r['mixed_sorted_over_mixed']:.2f} |")
    out += ["", "Per-kernel events of one count + fill call of the mixed set (`bvh_ctx_kernel_times`, ms per launch; the events add launch gaps, so the sum exceeds the call's time above):\n"]
    for r in doc["rows"]:
        if "kernels_mixed" in r:
            out.append(f"* {r['mesh']} {r['builder']}: " + ", ".join(f"`{k}` {v:.3f}" for k, v in sorted(r["kernels_mixed"].items())))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
