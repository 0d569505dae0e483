#!/usr/bin/env python3
"""time of bvh_intersect_tris beside bvh_overlap on the same tree with the query mesh's stage-E boxes as the query boxes; one process, one device.

bvh_overlap with those boxes is the broad phase alone (the box pairs), bvh_intersect_tris is the broad phase with the f64 narrow phase run at the leaf (the
crossing pairs), so the ratio of the two times is what the narrow phase costs.  Cases: a bunny-like mesh (327 680) against itself shifted by (0.37, 0.11,
-0.23) times its extent, a Sponza-like mesh (262 144) against itself (BVH_TRIS_SELF / BVH_OVERLAP_SELF) and a uniform soup (2 M) against itself, each on an HPLOC
and on a single-pass LBVH tree.  Timed with HIP events around --reps calls on the context's stream, count-only (d_prims NULL) and count + fill (capacity = the
total), the two alternating; the smaller of two rounds.  Also recorded: both totals, the longest slice of either answer (one lane per query: a wave waits for
its longest slice) and the per-kernel events of one count + fill call.  Writes <out>/intersect_tris.json and <out>/intersect_tris.md.

    python tools/time_intersect_tris.py
    python tools/time_intersect_tris.py --scale 0.1     # every mesh a tenth of its size
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

SHIFT = (0.37, 0.11, -0.23)
TOO_LARGE = -10002


def shifted(pkg, tris):
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    d = (np.array(SHIFT) * (v.max(axis=0) - v.min(axis=0))).astype(np.float32)
    out = tris.copy()
    for f in ("v1", "v2", "v3"):
        out[f] = (tris[f] + d[None, :]).astype(np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="every mesh this fraction of its size")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-total", type=int, default=1 << 30, help="largest result count that is filled (4 bytes each)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    sz = lambda n: max(int(n * a.scale), 1024)
    cases = [("bunny against its shift", "bunny", sz(327_680), False), ("sponza self", "sponza", sz(262_144), True), ("uniform self", "uniform", sz(2_000_000), True)]
    rows = []

    def measure(call, m, reps):
        """call(d_off, d_prims or None, capacity, total_out or None) -> rc.  -> dict(total, longest, count_ms, fill_ms or None)"""
        d_off = ctx.alloc((m + 1) * 4)
        total = C.c_uint64()
        rc = call(d_off, None, 0, C.byref(total))
        assert rc in (0, TOO_LARGE), rc
        total = int(total.value)
        ctx.synchronize()
        off = d_off.download(np.uint32, m + 1).astype(np.int64)
        out = {"queries": m, "total": total, "mean": total / m, "longest": int(np.diff(off).max()) if total <= 0xFFFFFFFF else None}
        d_prims = ctx.alloc(max(total, 1) * 4) if total <= min(a.max_total, 0xFFFFFFFF) else None
        cnt = lambda i: call(d_off, None, 0, None)
        fill = (lambda i: call(d_off, d_prims, total, None)) if d_prims else None
        assert cnt(0) == 0 and (fill is None or fill(0) == 0)
        c_ms, f_ms = [], []
        for _ in range(2):
            c_ms.append(timed(stream, cnt, reps))
            if fill:
                f_ms.append(timed(stream, fill, reps))
        out["count_ms"] = min(c_ms); out["count_ms_runs"] = c_ms
        out["fill_ms"] = min(f_ms) if fill else None; out["fill_ms_runs"] = f_ms
        if fill:                                                      # the kernels' shares in one count + fill call
            ctx.set_profiling(2)
            for i in range(3):
                assert fill(i) == 0
            out["kernels"] = {k: ms / c for k, (ms, c) in ctx.kernel_times().items()}
            ctx.set_profiling(0)
        d_off.free()
        if d_prims:
            d_prims.free()
        return out

    def dump():
        os.makedirs(a.out, exist_ok=True)
        doc = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale, "shift": SHIFT, "rows": rows}
        with open(os.path.join(a.out, "intersect_tris.json"), "w") as f:
            json.dump(doc, f, indent=1)
        with open(os.path.join(a.out, "intersect_tris.md"), "w") as f:
            f.write(render(doc))

    for label, kind, n, self_mode in cases:
        tris = {"bunny": pkg.meshgen.bunny_like, "sponza": pkg.meshgen.sponza_like, "uniform": pkg.meshgen.uniform}[kind](n, {"bunny": 2, "sponza": 3, "uniform": 1}[kind])
        n = len(tris)
        ctx.reserve(n)
        d_tris = ctx.upload(tris)
        d_q = d_qboxes = d_scene = qin = None
        if not self_mode:                                             # the other mesh and its stage-E boxes
            d_q = ctx.upload(shifted(pkg, tris))
            d_qboxes, d_scene = ctx.alloc(n * 24), ctx.alloc(24)
            assert L.bvh_stage_extents(ctx.handle, d_q.ptr, n, d_qboxes.ptr, d_scene.ptr) == 0
            qin = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_q.ptr, None, None, 0, 0)
        for algo in (3, 1):
            b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
            res = b.result
            mode = 1 if self_mode else 0
            boxes = res.d_prim_aabbs if self_mode else d_qboxes.ptr
            tri_call = lambda off, prims, cap, tot: L.bvh_intersect_tris(ctx.handle, C.byref(res), None, C.byref(qin) if qin is not None else None, n, mode,
                                                                         off.ptr, prims.ptr if prims else None, cap, tot)
            box_call = lambda off, prims, cap, tot: L.bvh_overlap(ctx.handle, C.byref(res), boxes, n, mode, off.ptr, prims.ptr if prims else None, cap, tot)
            reps = a.reps if n < 1_000_000 else max(a.reps // 2, 2)
            row = {"case": label, "mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "layout": int(res.layout), "n": n,
                   "tris": measure(tri_call, n, reps), "boxes": measure(box_call, n, reps)}
            row["count_ratio"] = row["tris"]["count_ms"] / row["boxes"]["count_ms"]
            if row["tris"]["fill_ms"] and row["boxes"]["fill_ms"]:
                row["fill_ratio"] = row["tris"]["fill_ms"] / row["boxes"]["fill_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            dump()
        for buf in (d_tris, d_q, d_qboxes, d_scene):
            if buf is not None:
                buf.free()
    ctx.close()
    dump()


def render(doc):
    def ms(x):
        return "not measured" if x is None else f"{x:.3f}"
    out = ["# bvh_intersect_tris — measured times (MI355X, one device)\n",
           f"`python tools/time_intersect_tris.py` (raw rows: `profiles/intersect_tris.json`; machine code `{doc['_kernel_source_hash']}`, the `kernel_source_hash` of "
           f"`bench.py`; device {doc['device']}; mesh sizes times {doc['scale']}).  Each row is one tree.  crossing = `bvh_intersect_tris` (broad phase + f64 narrow phase "
           "in one walk), boxes = `bvh_overlap` on the same tree with the query mesh's stage-E boxes as the query boxes (the broad phase alone; self cases: the tree's "
           "own primitive boxes, `BVH_OVERLAP_SELF`).  Times are ms per call, the smaller of two rounds of "
           f"{doc['reps']} calls (half as many from 1 M triangles) timed with HIP events on the context's stream, count-only (`d_prims` NULL) and count + fill alternating.  "
           "ratio = crossing / boxes: the cost of the narrow phase.  None of these times is a pass criterion.\n",
           "| case | mesh | builder (layout) | crossing pairs | box pairs | longest slice (crossing / boxes) | crossing: count only | count + fill | boxes: count only | count + fill | ratio: count only | count + fill |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        t, b = r["tris"], r["boxes"]
        fr = f"{r['fill_ratio']:.2f}" if "fill_ratio" in r else "not measured"
        out.append(f"| {r['case']} | {r['mesh']} | {r['builder']} ({r['layout']}) | {t['total']} | {b['total']} | {t['longest']} / {b['longest']} | {ms(t['count_ms'])} | "
                   f"{ms(t['fill_ms'])} | {ms(b['count_ms'])} | {ms(b['fill_ms'])} | {r['count_ratio']:.2f} | {fr} |")
    out += ["", "Per-kernel events of one count + fill call (`bvh_ctx_kernel_times`, ms per launch; the events add launch gaps, so the sum exceeds the call's time above):\n"]
    for r in doc["rows"]:
        for which in ("tris", "boxes"):
            if "kernels" in r[which]:
                out.append(f"* {r['mesh']} {r['builder']} {'crossing' if which == 'tris' else 'boxes'}: " + ", ".join(f"`{k}` {v:.3f}" for k, v in sorted(r[which]["kernels"].items())))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
