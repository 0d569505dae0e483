#!/usr/bin/env python3
"""one bvh_build_many_ploc against (a) a loop of bvh_build_ex(BVH_PLOCPP) over the same meshes and (b) one bvh_build_many (single-pass LBVH), and (c) what the
better trees buy: the summed bvh_sah_cost of a sample of meshes from each batch, and bvh_scene_intersect over camera rays on a scene whose bottom-level trees
come from each batch.

Shapes (tools/time_build_many.py's): 16 384 meshes x 64 triangles, 4 096 x 256, 2 048 x 512 and a mixed batch of 8 192 meshes of 2 .. 512 triangles (slices of one
uniform cloud, 64-byte records, resident on the device).  The loop is the code an application writes today: bvh_build_ex per mesh on one context (existing,
unchanged code).  Every side is timed with HIP events on the context's stream around the whole batch and with the host's wall clock around the same region, the
stream drained before and after — one warm-up batch, then --windows windows (at least 3); median window (smallest - largest), ms per batch.
The scene: 64 instances on an 8 x 8 grid, one 512-triangle mesh each (bunny-like bodies), bottom-level trees = the slices of one bvh_build_many (single-pass) and
of one bvh_build_many_ploc over the same triangles; 1024 x 1024 pinhole rays from above the grid, closest hit; a window is --reps calls.
Every step that uses the GPU is a child process of its own under a time limit; a step that fails or runs out of time ends the run.  Nothing here is a pass
criterion: a row that comes out against the batched PLOC++ call is reported as such.  Writes <out>/build_many_ploc.json and <out>/build_many_ploc.md.

    python tools/time_build_many_ploc.py
    python tools/time_build_many_ploc.py --windows 3 --scale 4        # a quarter of the meshes per shape
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = ["16384 x 64", "4096 x 256", "2048 x 512", "mixed 2..512"]
W = 1024
SAH_SAMPLE = 256
STEP_LIMIT_S = 240


def shape_counts(k, scale):
    rng = np.random.default_rng(1)
    return [np.full(16384 // scale, 64), np.full(4096 // scale, 256), np.full(2048 // scale, 512), rng.integers(2, 513, 8192 // scale)][k].astype(np.int64)


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "windows": [float(x) for x in t]}


def cell(t):
    return f"{t['median']:.3f} ({t['min']:.3f} – {t['max']:.3f})"


def render(doc):
    out = ["# bvh_build_many_ploc — batched PLOC++ trees against the loop, against the LBVH batch, and what they buy (MI355X, one device)\n",
           f"`python tools/time_build_many_ploc.py` (raw rows: `profiles/build_many_ploc.json`; machine code `{doc['_kernel_source_hash']}`, the `kernel_source_hash` "
           f"of `bench.py`; device {doc['device']}).  Protocol: triangles resident in device memory; the stream drained before and after every window; one warm-up "
           f"batch, then {doc['windows']} windows; median window (smallest – largest); HIP events on the context's stream around the whole batch and the host's wall "
           "clock around the same region; every GPU step a process of its own under a time limit.  None of these numbers is a pass criterion.\n",
           "## (a) one bvh_build_many_ploc against the loop of bvh_build_ex(BVH_PLOCPP), (b) against one bvh_build_many (single-pass)\n",
           "ms per batch.  loop / ploc and ploc / lbvh are ratios of the wall medians.\n",
           "| shape | meshes | triangles | loop events | loop wall | many_ploc events | many_ploc wall | many (LBVH) events | many (LBVH) wall | loop / ploc | ploc / lbvh | Mtris/s ploc |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["rows"]:
        out.append(f"| {r['shape']} | {r['n_meshes']} | {r['total']} | {cell(r['loop_events_ms'])} | {cell(r['loop_wall_ms'])} | {cell(r['ploc_events_ms'])} | "
                   f"{cell(r['ploc_wall_ms'])} | {cell(r['lbvh_events_ms'])} | {cell(r['lbvh_wall_ms'])} | {r['loop_over_ploc']:.1f} | {r['ploc_over_lbvh']:.2f} | "
                   f"{r['ploc_mtris_s']:.1f} |")
    out += ["\n## (c) the payoff: SAH\n", f"bvh_sah_cost summed over a sample of {SAH_SAMPLE} meshes of the batch (the same meshes from both batches); lower is better.\n",
            "| shape | sampled meshes | SAH sum, LBVH batch | SAH sum, PLOC++ batch | PLOC++ / LBVH |", "|---|---|---|---|---|"]
    for r in doc["rows"]:
        out.append(f"| {r['shape']} | {r['sah_sample']} | {r['sah_lbvh']:.2f} | {r['sah_ploc']:.2f} | {r['sah_ploc'] / r['sah_lbvh']:.3f} |")
    s = doc.get("scene")
    if s:
        out += ["\n## (c) the payoff: rays\n",
                f"bvh_scene_intersect, {W} x {W} pinhole rays, closest hit, on {s['instances']} instances of {s['tris_per_mesh']}-triangle meshes ({s['hit_fraction'] * 100:.1f} % "
                f"of the rays hit; both scenes answer alike: {s['answers_equal']}); ms per call, windows of {s['reps']} calls.\n",
                "| bottom-level trees from | ms per call |", "|---|---|",
                f"| bvh_build_many (single-pass LBVH) | {cell(s['lbvh_ms'])} |", f"| bvh_build_many_ploc | {cell(s['ploc_ms'])} |",
                f"\nPLOC++ / LBVH = {s['ploc_ms']['median'] / s['lbvh_ms']['median']:.3f}."]
    return "\n".join(out) + "\n"


class Bench:
    def __init__(self):
        import torch
        import bvh_pkg
        self.torch = torch
        self.pkg = bvh_pkg.load(); self.L = self.pkg.lib()
        torch.cuda.init()
        self.device = torch.cuda.get_device_name(0)
        self.ctx = self.pkg.Context(0)
        self.stream = torch.cuda.ExternalStream(self.L.bvh_ctx_stream(self.ctx.handle), device=torch.device("cuda", 0))

    def window(self, fn):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.ctx.synchronize()
        t0 = time.perf_counter()
        e0.record(self.stream)
        fn()
        e1.record(self.stream)
        e1.synchronize()
        self.ctx.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    def windows(self, fn, count):
        self.window(fn)                                               # warm-up
        return [self.window(fn) for _ in range(count)]


def step_shape(k, a):
    b = Bench(); pkg, L, ctx = b.pkg, b.L, b.ctx
    counts = shape_counts(k, a.scale)
    out_off, _, total = pkg.many_layout(counts)
    d_tris = ctx.upload(pkg.meshgen.uniform(total, 1))
    ranges = pkg.many_check_ranges(np.stack([out_off, counts], axis=1), total)
    n = len(ranges)
    ctx.reserve(1024)
    subs = [pkg.BuildInput(pkg.TRI_PADDED64, 30, d_tris.ptr + 64 * int(f), None, None, 0, 0) for f in out_off]
    res = pkg.Result()

    def loop():
        for m in range(n):
            rc = L.bvh_build_ex(ctx.handle, pkg.ALGO_PLOCPP, C.byref(subs[m]), int(counts[m]), C.byref(res), None)
            assert rc == 0, rc
    lb = ctx.build_many((d_tris, ranges), algo=pkg.ALGO_SINGLEPASS, n_tris=total)
    pl = ctx.build_many_ploc((d_tris, ranges), n_tris=total)

    def many_lbvh():
        rc = L.bvh_build_many(ctx.handle, pkg.ALGO_SINGLEPASS, C.byref(lb.input), total, ranges.ctypes.data, n, C.byref(lb.out), None)
        assert rc == 0, rc

    def many_ploc():
        rc = L.bvh_build_many_ploc(ctx.handle, pkg.ALGO_PLOCPP, C.byref(pl.input), total, ranges.ctypes.data, n, C.byref(pl.out), None)
        assert rc == 0, rc
    t = {key: b.windows(fn, a.windows) for key, fn in (("loop", loop), ("ploc", many_ploc), ("lbvh", many_lbvh))}
    row = {"shape": SHAPES[k], "n_meshes": n, "total": int(total), "device": b.device}
    for key in t:
        row[f"{key}_events_ms"] = stats([x[0] for x in t[key]]); row[f"{key}_wall_ms"] = stats([x[1] for x in t[key]])
    row["loop_over_ploc"] = row["loop_wall_ms"]["median"] / row["ploc_wall_ms"]["median"]
    row["ploc_over_lbvh"] = row["ploc_wall_ms"]["median"] / row["lbvh_wall_ms"]["median"]
    row["ploc_mtris_s"] = total / row["ploc_wall_ms"]["median"] / 1e3
    ctx.synchronize()
    sample = np.random.default_rng(3).choice(n, min(SAH_SAMPLE, n), replace=False)
    row["sah_sample"] = len(sample)
    row["sah_lbvh"] = float(sum(lb.builder(int(m)).sah_cost() for m in sample))
    row["sah_ploc"] = float(sum(pl.builder(int(m)).sah_cost() for m in sample))
    lb.free(); pl.free(); d_tris.free(); ctx.close()
    return row


def step_scene(a):
    b = Bench(); pkg, L, ctx = b.pkg, b.L, b.ctx
    g, per = 8, 512
    meshes = [pkg.meshgen.bunny_like(per, 100 + k) for k in range(g * g)]
    v = np.concatenate([np.concatenate([t["v1"], t["v2"], t["v3"]]) for t in meshes]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    step = (hi - lo) * 1.1
    inst = np.zeros(g * g, dtype=pkg.INSTANCE)
    for k in range(g * g):
        inst["object_to_world"][k] = np.array([1, 0, 0, step[0] * (k % g), 0, 1, 0, 0, 0, 0, 1, step[2] * (k // g)], dtype=np.float32)
        inst["blas"][k] = k
    centre = np.array([lo[0] + 0.5 * g * step[0], 0.5 * (lo[1] + hi[1]), lo[2] + 0.5 * g * step[2]])
    eye = centre + np.array([0.0, 0.6 * g * step[0], -0.6 * g * step[2]])
    f = centre - eye; f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 1.0, 0.0]); r /= np.linalg.norm(r); u = np.cross(r, f)
    s = np.tan(np.radians(50.0) / 2)
    x, y = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(W) + 0.5) / W * 2 - 1, indexing="ij")
    d = f[None] + s * x.reshape(-1, 1) * r[None] + s * y.reshape(-1, 1) * u[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(W * W, dtype=pkg.RAY)
    rays["origin"] = eye.astype(np.float32); rays["direction"] = d.astype(np.float32); rays["tmax"] = 3.0e38
    d_rays = ctx.upload(rays); d_hits = ctx.alloc(W * W * pkg.INSTANCE_HIT.itemsize)
    out = {"instances": g * g, "tris_per_mesh": per, "reps": a.reps, "device": b.device}
    hits = {}
    for key, mt in (("lbvh", ctx.build_many(meshes, algo=pkg.ALGO_SINGLEPASS)), ("ploc", ctx.build_many_ploc(meshes))):
        ctx.synchronize()
        sc = pkg.Scene(ctx).build(pkg.ALGO_HPLOC, [mt.blas(m) for m in range(g * g)], inst)

        def query():
            for _ in range(a.reps):
                rc = L.bvh_scene_intersect(sc.handle, d_rays.ptr, W * W, d_hits.ptr, 0)
                assert rc == 0, rc
        t = b.windows(query, a.windows)
        out[f"{key}_ms"] = stats([x[0] / a.reps for x in t])
        hits[key] = d_hits.download(pkg.INSTANCE_HIT, W * W)
        sc.close(); mt.free()
    out["hit_fraction"] = float((hits["ploc"]["prim"] != pkg.INVALID).mean())
    out["answers_equal"] = bool(hits["ploc"].tobytes() == hits["lbvh"].tobytes())
    d_rays.free(); d_hits.free(); ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="scene queries per window")
    ap.add_argument("--scale", type=int, default=1, help="divide every shape's mesh count by this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process: shape:<k> or scene; the result goes to --json")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("at least 3 windows")
    if a.step:
        res = step_scene(a) if a.step == "scene" else step_shape(int(a.step.split(":")[1]), a)
        with open(a.json, "w") as f:
            json.dump(res, f)
        return 0
    from _srchash import kernel_source_hash
    doc = {"_kernel_source_hash": kernel_source_hash(), "device": None, "windows": a.windows, "rows": []}
    os.makedirs(a.out, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for step in [f"shape:{k}" for k in range(len(SHAPES))] + ["scene"]:
            path = os.path.join(tmp, "step.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--json", path, "--windows", str(a.windows), "--reps", str(a.reps), "--scale", str(a.scale)]
            try:
                rc = subprocess.run(cmd, timeout=STEP_LIMIT_S).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"step {step} ended with status {rc}: nothing more is started", file=sys.stderr)
                return rc
            with open(path) as f:
                res = json.load(f)
            print(json.dumps(res), flush=True)
            if step == "scene":
                doc["scene"] = res
            else:
                doc["rows"].append(res)
            doc["device"] = res["device"]
            with open(os.path.join(a.out, "build_many_ploc.json"), "w") as f:
                json.dump(doc, f, indent=1)
            with open(os.path.join(a.out, "build_many_ploc.md"), "w") as f:
                f.write(render(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
