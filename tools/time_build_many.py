#!/usr/bin/env python3
"""one bvh_build_many against a loop of bvh_build_ex over the same meshes; one process, one device.

Shapes: 16 384 meshes x 64 triangles, 4 096 x 256, 2 048 x 512 and a mixed batch of 2 .. 512 triangles per mesh (slices of one uniform cloud, 64-byte records),
for both LBVH builders.  The baseline is the loop an application writes today: bvh_build_ex per mesh on one context (existing, unchanged code; the single-pass
builder waits for its root index in every call, the two-pass one does not).  Both sides are timed with HIP events on the context's stream around the whole batch
— one warm-up batch, then --windows windows — and with the host's wall clock around the same region (stream drained before and after): the loop is bound by
launch latency and host work, which events alone would understate.  Median window (smallest – largest), ms per batch.  Nothing here is a pass criterion: a
shape where the batched call does not win is reported as such.  Writes <out>/build_many.json and <out>/build_many.md, stamped with the library's machine-code hash.

    python tools/time_build_many.py
    python tools/time_build_many.py --windows 3 --scale 4        # a quarter of the meshes per shape
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


def render(doc):
    out = ["# bvh_build_many — one batched call against a loop of bvh_build_ex (MI355X, one device)\n",
           f"`python tools/time_build_many.py` (raw rows: `profiles/build_many.json`; machine code `{doc['_kernel_source_hash']}`, the `kernel_source_hash` of "
           f"`bench.py`; device {doc['device']}).  Per batch, ms: HIP events on the context's stream around the whole batch and the host's wall clock around the "
           f"same region, one warm-up batch, then {doc['windows']} windows; median window (smallest – largest).  loop = bvh_build_ex per mesh on one context "
           "(existing code, the baseline); many = one bvh_build_many.  ratio = loop / many of the wall medians.  None of these numbers is a pass criterion.\n",
           "| shape | builder | meshes | triangles | loop events | loop wall | many events | many wall | ratio | Mtris/s many |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        def cell(t):
            return f"{t['median']:.3f} ({t['min']:.3f} – {t['max']:.3f})"
        out.append(f"| {r['shape']} | {r['builder']} | {r['n_meshes']} | {r['total']} | {cell(r['loop_events_ms'])} | {cell(r['loop_wall_ms'])} | "
                   f"{cell(r['many_events_ms'])} | {cell(r['many_wall_ms'])} | {r['ratio']:.1f} | {r['many_mtris_s']:.1f} |")
    return "\n".join(out) + "\n"


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "windows": [float(x) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide every shape's mesh count by this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    rng = np.random.default_rng(1)
    shapes = [("16384 x 64", np.full(16384 // a.scale, 64)), ("4096 x 256", np.full(4096 // a.scale, 256)), ("2048 x 512", np.full(2048 // a.scale, 512)),
              ("mixed 2..512", rng.integers(2, 513, 8192 // a.scale))]
    rows = []
    doc = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "windows": a.windows, "rows": rows}

    def dump():
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "build_many.json"), "w") as f:
            json.dump(doc, f, indent=1)
        with open(os.path.join(a.out, "build_many.md"), "w") as f:
            f.write(render(doc))

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ctx.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    ctx.reserve(1024)
    for name, counts in shapes:
        counts = counts.astype(np.int64)
        out_off, _, total = pkg.many_layout(counts)
        d_tris = ctx.upload(pkg.meshgen.uniform(total, 1))
        ranges = pkg.many_check_ranges(np.stack([out_off, counts], axis=1), total)
        n = len(ranges)
        inp = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_tris.ptr, None, None, 0, 0)
        subs = [pkg.BuildInput(pkg.TRI_PADDED64, 30, d_tris.ptr + 64 * int(f), None, None, 0, 0) for f in out_off]
        bufs = [ctx.alloc((2 * total - n) * 32), ctx.alloc(total * 24), ctx.alloc(n * 24), ctx.alloc(n * 4), ctx.alloc(total * 4), ctx.alloc(total * 4)]
        out = pkg.ManyOut(*[b.ptr for b in bufs])
        for algo in (pkg.ALGO_TWOPASS, pkg.ALGO_SINGLEPASS):
            res = pkg.Result()

            def loop():
                for m in range(n):
                    rc = L.bvh_build_ex(ctx.handle, algo, C.byref(subs[m]), int(counts[m]), C.byref(res), None)
                    assert rc == 0, rc

            def many():
                rc = L.bvh_build_many(ctx.handle, algo, C.byref(inp), total, ranges.ctypes.data, n, C.byref(out), None)
                assert rc == 0, rc
            t = {"loop": [], "many": []}
            for key, fn in (("loop", loop), ("many", many)):
                window(fn)                                            # warm-up
                for _ in range(a.windows):
                    t[key].append(window(fn))
            row = {"shape": name, "builder": pkg.ALGO_NAMES[algo], "n_meshes": n, "total": int(total)}
            for key in ("loop", "many"):
                row[f"{key}_events_ms"] = stats([x[0] for x in t[key]]); row[f"{key}_wall_ms"] = stats([x[1] for x in t[key]])
            row["ratio"] = row["loop_wall_ms"]["median"] / row["many_wall_ms"]["median"]
            row["many_mtris_s"] = total / row["many_wall_ms"]["median"] / 1e3
            rows.append(row)
            print(json.dumps(row), flush=True)
            dump()
        for b in bufs + [d_tris]:
            b.free()
    ctx.close()
    dump()


if __name__ == "__main__":
    main()
