#!/usr/bin/env python3
"""time of the all-instances crossing-pair query (bvh_scene_collide) against the loop of bvh_scene_intersect_tris(BVH_SCENE_TRIS_INSTANCE, k) over every
instance k that it replaces, one process, one device.  Writes <out>/scene_collide.json and <out>/scene_collide.md, stamped with the library's machine-code hash.

  (a) 64 instances   tools/time_scene_intersect_tris.py's 4 x 4 x 4 grid of the bunny-like and the Sponza-like mesh at 0.6 of its extent per axis (one HPLOC
                     BLAS), so that neighbours interpenetrate.
  (b) 4 096 bodies   of 512 triangles, each a BLAS of its own made by bvh_build_many, on a jittered 16 x 16 x 16 grid at 0.6 of a body's extent.

bvh_scene_collide, default and BVH_SCENE_COLLIDE_BOTH, in three modes — count only, unsorted fill, sorted fill — and the loop in the same three modes, which
finds every pair twice as BOTH does.  The loop's calls share one offsets array and one record array of the largest instance's total (a caller that kept every
answer would allocate more, not launch less).  HIP events on the context's stream, one warm-up of every shape, alternating windows, median.

    python tools/time_scene_collide.py
    python tools/time_scene_collide.py --reps 1 --windows 3 --scale 0.05 --bodies 512
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(ROOT)); sys.path.insert(0, ROOT)
import bvh_pkg  # noqa: E402
from bench import kernel_source_hash  # noqa: E402
from time_scene import kernel_split, stream_of  # noqa: E402
from time_scene_intersect_tris import MESHES, cube_instances  # noqa: E402
from time_scene_knn import windows  # noqa: E402
from time_scene_radius import distribution  # noqa: E402

SORTED, BOTH = 1, 2
INSTANCE = 1
PASSES = (("count", None), ("unsorted", 0), ("sorted", SORTED))


class Collider:
    """the three timed calls of bvh_scene_collide on one scene, the capacity taken from a first counting call"""

    def __init__(self, L, ctx, sc, rows, both):
        self.L, self.ctx, self.sc, self.rows, self.bit = L, ctx, sc, rows, BOTH if both else 0
        self.d_first, self.d_off = ctx.alloc((sc.n_instances + 1) * 4), ctx.alloc((rows + 1) * 4)
        n_rows, total = C.c_uint64(), C.c_uint64()
        assert L.bvh_scene_collide(sc.handle, self.bit, self.d_first.ptr, rows, self.d_off.ptr, None, 0, C.byref(n_rows), C.byref(total)) == 0
        assert n_rows.value == rows
        self.total = total.value
        self.d_prims = ctx.alloc(max(self.total, 1) * 8)

    def fn(self, flags):
        if flags is None:
            return lambda i: self.L.bvh_scene_collide(self.sc.handle, self.bit, self.d_first.ptr, self.rows, self.d_off.ptr, None, 0, None, None)
        return lambda i: self.L.bvh_scene_collide(self.sc.handle, self.bit | flags, self.d_first.ptr, self.rows, self.d_off.ptr, self.d_prims.ptr, self.total, None, None)

    def offsets(self):
        self.ctx.synchronize()
        return self.d_off.download(np.uint32, self.rows + 1)

    def free(self):
        self.d_first.free(); self.d_off.free(); self.d_prims.free()


class Loop:
    """bvh_scene_intersect_tris(INSTANCE, k) for every k: what a caller had to write before bvh_scene_collide.  leaves[k]: the rows of instance k's call"""

    def __init__(self, L, ctx, sc, leaves):
        self.L, self.ctx, self.sc, self.leaves = L, ctx, sc, [int(n) for n in leaves]
        self.d_off = ctx.alloc((max(self.leaves) + 1) * 4)
        total, self.totals = C.c_uint64(), []
        for k, n in enumerate(self.leaves):
            assert L.bvh_scene_intersect_tris(sc.handle, None, n, INSTANCE, k, 0, self.d_off.ptr, None, 0, C.byref(total)) == 0
            self.totals.append(total.value)
        self.total, self.cap = sum(self.totals), max(self.totals)
        self.d_prims = ctx.alloc(max(self.cap, 1) * 8)

    def fn(self, flags):
        f, h, o = self.L.bvh_scene_intersect_tris, self.sc.handle, self.d_off.ptr
        prims, cap, fl = (None, 0, 0) if flags is None else (self.d_prims.ptr, self.cap, flags)

        def run(i):
            rc = 0
            for k, n in enumerate(self.leaves):
                rc |= f(h, None, n, INSTANCE, k, fl, o, prims, cap, None)
            return rc
        return run

    def free(self):
        self.d_off.free(); self.d_prims.free()


def measure(L, ctx, stream, sc, leaves, n_windows, reps):
    """{default / both / loop: {pass: times}}, the slice distribution, the totals and the per-kernel split of a sorted BOTH call"""
    rows = int(sum(leaves))
    calls = {"default": Collider(L, ctx, sc, rows, False), "both": Collider(L, ctx, sc, rows, True), "loop": Loop(L, ctx, sc, leaves)}
    work = [(f"{label} {name}", stream, c.fn(fl)) for label, c in calls.items() for name, fl in PASSES]
    t = windows(work, n_windows, reps)
    out = {f"{label}_ms": {name: t[f"{label} {name}"] for name, _ in PASSES} for label in calls}
    assert calls["both"].fn(SORTED)(0) == 0
    out["slices"] = distribution(calls["both"].offsets())
    out["totals"] = {label: c.total for label, c in calls.items()}
    out["launches_of_the_loop"] = {"count": 3 * len(leaves), "fill": 6 * len(leaves)}     # (walk, deep and scan per pass; a filling call runs both passes)
    out["kernels"] = kernel_split(ctx, calls["both"].fn(SORTED), reps=2)
    for c in calls.values():
        c.free()
    return out


def jittered_grid(pkg, side, step, rng):
    inst = cube_instances(pkg, side, step)
    m = inst["object_to_world"].copy()
    m[:, [3, 7, 11]] += (rng.uniform(-0.2, 0.2, (len(m), 3)) * step).astype(np.float32)
    inst["object_to_world"] = m
    inst["blas"] = np.arange(len(inst), dtype=np.uint32)
    return inst


def write_md(out, path):
    cell = lambda t: f"{t['median']:.2f} ms [{t['min']:.2f} .. {t['max']:.2f}]"
    dist = lambda d: (f"{d['total']:,} records; empty {d['empty']:.3f}, mean {d['mean']:.2f}, p99 {d['p99']:.0f}, longest {d['max']}")
    L = [f"# Crossing triangle pairs of all instances at once on one MI355X (`tools/time_scene_collide.py --reps {out['reps']} --windows {out['windows']}`, "
         f"`profiles/scene_collide.json`; machine code `{out['_kernel_source_hash']}`, the `kernel_source_hash` of `bench.py`)", "",
         f"{out['device']}.  HIP events on the context's stream, one warm-up call of every shape, then {out['windows']} windows of {out['reps']} calls timed in "
         "alternation; median window per call, [smallest .. largest window].  count: a count-only call; unsorted / sorted: a call that counts and fills "
         "(capacity = the total, no read-back).  loop: `bvh_scene_intersect_tris(BVH_SCENE_TRIS_INSTANCE, k)` for every instance k from the host, which finds "
         "every pair twice, as `BVH_SCENE_COLLIDE_BOTH` does.", ""]
    for r in out["shapes"]:
        L += [f"## {r['title']}", "", f"{r['instances']:,} instances, {r['rows']:,} rows.  `BOTH` slices: {dist(r['slices'])}.  Totals: default {r['totals']['default']:,}, "
              f"`BOTH` {r['totals']['both']:,}, loop {r['totals']['loop']:,}.  The loop is {r['launches_of_the_loop']['count']:,} launches per counting pass and "
              f"{r['launches_of_the_loop']['fill']:,} per filling one.", "",
              "| call | loop over instances | `bvh_scene_collide`, `BOTH` | loop / `BOTH` | `bvh_scene_collide`, default | loop / default |", "|---|---|---|---|---|---|"]
        for name, _ in PASSES:
            lo, bo, de = r["loop_ms"][name], r["both_ms"][name], r["default_ms"][name]
            L.append(f"| {name} | {cell(lo)} | {cell(bo)} | {lo['median'] / bo['median']:.2f}x | {cell(de)} | {lo['median'] / de['median']:.2f}x |")
        L += ["", "Per kernel, sorted `BOTH` call (ms per launch, launches): " + ", ".join(f"`{k}` {v[0]:.4f} ({v[1]})" for k, v in sorted(r["kernels"].items())) + ".", ""]
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--meshes", nargs="*", default=["sponza", "bunny"], choices=sorted(MESHES))
    ap.add_argument("--scale", type=float, default=1.0, help="scales the meshes' triangle counts (a rehearsal at a small size)")
    ap.add_argument("--bodies", type=int, default=4096, help="bodies of shape (b): a cube number; 0 leaves the shape out")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(ROOT), "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    if not torch.cuda.is_available():
        sys.exit("time_scene_collide.py needs the GPU: there is no fallback")
    torch.cuda.init()
    out = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "shapes": []}

    def done(row):
        out["shapes"].append(row)
        print(json.dumps({"shape": row["title"], **{lab: {k: v["median"] for k, v in row[lab + "_ms"].items()} for lab in ("loop", "both", "default")},
                          "totals": row["totals"]}), flush=True)
        os.makedirs(a.out, exist_ok=True)                                 # (after every shape: what has been measured is on disk)
        with open(os.path.join(a.out, "scene_collide.json"), "w") as f:
            json.dump(out, f, indent=1)
        write_md(out, os.path.join(a.out, "scene_collide.md"))

    for key in a.meshes:                                                  # ---- (a) 64 interpenetrating instances of one large mesh
        title, n, gen = MESHES[key]
        tris = gen(pkg, max(int(n * a.scale), 64))
        n = len(tris)
        v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
        ext = v.max(axis=0) - v.min(axis=0)
        scene_ctx, bctx = pkg.Context(0), pkg.Context(0)
        d_tris = bctx.upload(tris)
        b = pkg.HPLOC().build(bctx, d_tris, on_device=True, n=n)
        inst = cube_instances(pkg, 4, 0.6 * ext)
        sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [b], inst)
        row = {"title": f"(a) 64 instances of the {title} mesh, {n:,} triangles (4 x 4 x 4 grid at 0.6 of the extent)", "instances": 64, "rows": 64 * n}
        row.update(measure(L, scene_ctx, stream_of(L, scene_ctx), sc, [n] * 64, a.windows, a.reps))
        sc.close(); d_tris.free(); scene_ctx.close(); bctx.close()
        done(row)

    if a.bodies:                                                          # ---- (b) thousands of small bodies, each a BLAS of its own
        side = round(a.bodies ** (1 / 3))
        count = side ** 3
        rng = np.random.default_rng(5)
        base = [pkg.meshgen.uniform(512, 100 + j) for j in range(64)]
        ext = np.ptp(np.concatenate([base[0]["v1"], base[0]["v2"], base[0]["v3"]]).astype(np.float64), axis=0)
        scene_ctx = pkg.Context(0)
        many = scene_ctx.build_many([base[m % 64] for m in range(count)])
        scene_ctx.synchronize()
        sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [many.blas(m) for m in range(count)], jittered_grid(pkg, side, 0.6 * ext, rng))
        row = {"title": f"(b) {count:,} bodies of 512 triangles (`bvh_build_many`; a jittered {side} x {side} x {side} grid at 0.6 of a body's extent)", "instances": count,
               "rows": sum(len(base[m % 64]) for m in range(count))}
        row.update(measure(L, scene_ctx, stream_of(L, scene_ctx), sc, [len(base[m % 64]) for m in range(count)], a.windows, a.reps))
        sc.close(); scene_ctx.close()
        done(row)


if __name__ == "__main__":
    main()
