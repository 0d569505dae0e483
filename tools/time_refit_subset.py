#!/usr/bin/env python3
"""time of bvh_refit_subset against the full bvh_refit_ex and a single-pass LBVH rebuild, one process, one device.

For each mesh (uniform 10 M, uniform 2 M, Sponza-like 262 144) and tree (single-pass LBVH, HPLOC): one build, then for every dirty fraction (1e-4 .. 1) and
both kinds of dirty set — clustered: a contiguous run of d_sorted_vals (one moving object); scattered: uniform random — --windows windows of --calls subset
refits each, HIP events on the context's stream around every window, alternating two device-resident vertex states.  A window of the full bvh_refit_ex on
the same tree follows every subset window, so a drift of the machine falls on both; the median window is the figure, the smallest and largest are kept as
the spread, and the crossover counts a row as beaten only where the two spreads do not overlap.  The parent plan and the leaf map are made by the warm-up
calls and excluded; their cost is reported separately (per-kernel events of one call that makes them).  The single-pass LBVH build of the mesh is the second
yardstick.  One more row per tree: the same call on a caller-owned copy of the arrays, which zeroes the words and makes plan and map on every call (work in
the ctx's capacity, not in n_dirty).  Small lists are three small launches per call: their rows measure the enqueue rate of this host, not kernel time.
Writes <out>/refit_subset.md.

    timeout -k 10 900 python tools/time_refit_subset.py                    # all three meshes
    timeout -k 10 300 python tools/time_refit_subset.py --mesh uniform:2000000
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
import bvh_pkg  # noqa: E402

FRACTIONS = [1e-4, 1e-3, 1e-2, 1e-1, 1.0]


def jitter(tris, seed, scale=1e-3):
    rng = np.random.default_rng(seed)
    t = tris.copy()
    for f in ("v1", "v2", "v3"):
        t[f] = (t[f] + rng.normal(0.0, scale, t[f].shape)).astype(np.float32)
    return t


def timed(stream, fn, reps):
    """mean ms per call of fn(i) over reps calls, HIP events around the whole loop"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    for i in range(reps):
        fn(i)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def windows(stream, fns, reps, count):
    """count rounds, in each one window of reps calls of every fn in turn: per fn {median, min, max} of the windows' ms per call"""
    t = [[] for _ in fns]
    for _ in range(count):
        for k, fn in enumerate(fns):
            t[k].append(timed(stream, fn, reps))
    return [{"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))} for x in t]


def cell(t):
    return f"{t['median']:.4f} ({t['min']:.4f} – {t['max']:.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", action="append", help="kind:n (uniform / sponza), repeatable; default: the three meshes of the table")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--builds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    meshes = [(m.split(":")[0], int(m.split(":")[1])) for m in a.mesh] if a.mesh else [("uniform", 10_000_000), ("uniform", 2_000_000), ("sponza", 262_144)]
    pkg = bvh_pkg.load(); L = pkg.lib()
    if not torch.cuda.is_available():
        sys.exit("time_refit_subset.py needs the GPU: there is no fallback")
    torch.cuda.init()
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    rows, yard, owned_rows = [], [], []
    for kind, n in meshes:
        tris = pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 1)
        ctx.reserve(n)
        d_a, d_b = ctx.upload(tris), ctx.upload(jitter(tris, 7))
        ins = [pkg.BuildInput(pkg.TRI_PADDED64, 30, d.ptr, None, None, 0, 0) for d in (d_b, d_a)]
        res = pkg.Result()

        def build(i, res=res):
            assert L.bvh_build(ctx.handle, pkg.ALGO_SINGLEPASS, d_a.ptr, n, 1, C.byref(res), None) == 0
        build(0); build(0)
        build_t = windows(stream, [build], a.builds, a.windows)[0]
        rng = np.random.default_rng(n)
        for algo in (pkg.ALGO_SINGLEPASS, pkg.ALGO_HPLOC):
            b = pkg.BUILDERS[algo]().build(ctx, d_a, on_device=True, n=n)
            res = b.result
            svals = np.empty(n, dtype=np.uint32)
            assert L.bvh_dev_download(ctx.handle, svals.ctypes.data, res.d_sorted_vals, svals.nbytes) == 0
            # every list is on the device before the first call: an upload through the ctx ends the cached plan and map
            lists = {}
            for frac in FRACTIONS:
                m = max(1, int(round(frac * n)))
                start = int(rng.integers(0, n - m + 1))
                lists[(frac, "clustered")] = (ctx.upload(svals[start:start + m].copy()), m)
                lists[(frac, "scattered")] = (ctx.upload(rng.choice(n, m, replace=False).astype(np.uint32)), m)
            # a caller-owned copy of the arrays (made now, for the last row: device copies through the ctx end the cached plan and map too)
            sizes = {"d_nodes": (2 * n - 1 if res.layout == 0 else n - 1) * pkg.BVH2_NODE.itemsize, "d_prim_aabbs": n * pkg.AABB.itemsize,
                     "d_scene_extent": pkg.AABB.itemsize}
            if res.layout == 1:
                sizes["d_leaves"] = n * pkg.PRIMREF.itemsize
            owned, copies = pkg.Result.from_buffer_copy(res), []
            for f, nbytes in sizes.items():
                copies.append(ctx.alloc(nbytes))
                assert L.bvh_dev_copy(ctx.handle, copies[-1].ptr, getattr(res, f), nbytes) == 0
                setattr(owned, f, copies[-1].ptr)
            # the plan and the map: per-kernel events of the one call that makes them
            ctx.synchronize(); ctx.set_profiling(2)
            d_p, m = lists[(1e-4, "scattered")]
            assert L.bvh_refit_subset(ctx.handle, C.byref(res), C.byref(ins[1]), d_p.ptr, m, None) == 0
            kt = {k: v[0] / v[1] for k, v in ctx.kernel_times().items()}
            ctx.set_profiling(0)
            plan_ms, map_ms = kt.get("k_refit_plan", float("nan")), kt.get("k_refit_leafmap", float("nan"))

            def full(i, res=res):
                assert L.bvh_refit_ex(ctx.handle, C.byref(res), C.byref(ins[i % 2]), None) == 0
            for i in range(4):
                full(i)
            full_t = windows(stream, [full], a.calls, a.windows)[0]
            yard.append({"mesh": kind, "n": n, "tree": pkg.ALGO_NAMES[algo], "full_refit_ms": full_t, "lbvh_single_build_ms": build_t,
                         "plan_ms": round(plan_ms, 4), "leafmap_ms": round(map_ms, 4)})
            print(json.dumps(yard[-1]), flush=True)
            for (frac, how), (d_p, m) in lists.items():
                def subset(i, res=res, d_p=d_p, m=m):
                    assert L.bvh_refit_subset(ctx.handle, C.byref(res), C.byref(ins[i % 2]), d_p.ptr, m, None) == 0
                for i in range(4):
                    subset(i)
                sub_t, ful_t = windows(stream, [subset, full], a.calls, a.windows)           # (a full-refit window after every subset window)
                rows.append({"mesh": kind, "n": n, "tree": pkg.ALGO_NAMES[algo], "set": how, "fraction": frac, "n_dirty": m, "subset_ms": sub_t,
                             "full_refit_ms": ful_t, "subset_over_full": round(sub_t["median"] / ful_t["median"], 3),
                             "us_per_dirty": round(1e3 * sub_t["median"] / m, 5), "beats_full": sub_t["max"] < ful_t["min"]})
                print(json.dumps(rows[-1]), flush=True)
            full(1)                                                   # (every box back to one vertex state)
            d_p, m = lists[(1e-3, "scattered")]

            def subset_owned(i, d_p=d_p, m=m):
                assert L.bvh_refit_subset(ctx.handle, C.byref(owned), C.byref(ins[i % 2]), d_p.ptr, m, None) == 0
            for i in range(4):
                subset_owned(i)
            own_t = windows(stream, [subset_owned], a.calls, a.windows)[0]
            mine = next(r for r in rows[::-1] if (r["set"], r["fraction"]) == ("scattered", 1e-3))
            owned_rows.append({"mesh": kind, "n": n, "tree": pkg.ALGO_NAMES[algo], "n_dirty": m, "caller_owned_ms": own_t, "own_tree_ms": mine["subset_ms"]})
            print(json.dumps(owned_rows[-1]), flush=True)
            ctx.synchronize()
            for d_p, _ in lists.values():
                d_p.free()
            for d in copies:
                d.free()
        d_a.free(); d_b.free()
    ctx.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "refit_subset.md"), "w") as f:
        f.write("# bvh_refit_subset vs the full bvh_refit_ex and a rebuild (tools/time_refit_subset.py)\n\n")
        f.write(f"{torch.cuda.get_device_name(0)}. {a.windows} windows of {a.calls} calls per row, alternating two device-resident vertex states, HIP events around "
                "every window on the\ncontext's stream; ms per call, median window (smallest – largest). A full-refit window follows every subset window; "
                "parent plan and leaf map cached\n(excluded, reported below). clustered: a contiguous run of d_sorted_vals; scattered: uniform random. "
                "Rows with small lists are three\nsmall launches per call and measure the host's enqueue rate rather than kernel time.\n\n")
        f.write("## Yardsticks (same run)\n\n| mesh | n | tree | full refit ms | LBVH-1 build ms | k_refit_plan ms | k_refit_leafmap ms |\n|---|---:|---|---:|---:|---:|---:|\n")
        for y in yard:
            f.write(f"| {y['mesh']} | {y['n']} | {y['tree']} | {cell(y['full_refit_ms'])} | {cell(y['lbvh_single_build_ms'])} | {y['plan_ms']:.4f} | {y['leafmap_ms']:.4f} |\n")
        f.write("\n## Subset refit\n\n| mesh | n | tree | set | fraction | n_dirty | subset ms | full refit ms | subset / full | us per dirty prim |\n|---|---:|---|---|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            f.write(f"| {r['mesh']} | {r['n']} | {r['tree']} | {r['set']} | {r['fraction']:g} | {r['n_dirty']} | {cell(r['subset_ms'])} | {cell(r['full_refit_ms'])} | "
                    f"{r['subset_over_full']:.3f} | {r['us_per_dirty']:.5f} |\n")
        f.write("\n## Crossover\n\nThe smallest measured dirty fraction at which the subset call no longer beats the full refit: its largest window is not below the "
                "full refit's smallest.\n\n| mesh | n | tree | set | crossover fraction |\n|---|---:|---|---|---|\n")
        for y in yard:
            for how in ("clustered", "scattered"):
                mine = [r for r in rows if (r["mesh"], r["n"], r["tree"], r["set"]) == (y["mesh"], y["n"], y["tree"], how)]
                over = [r["fraction"] for r in mine if not r["beats_full"]]
                f.write(f"| {y['mesh']} | {y['n']} | {y['tree']} | {how} | {('%g' % min(over)) if over else 'none up to 1'} |\n")
        f.write("\n## Caller-owned arrays\n\nThe scattered 1e-3 list on a caller-owned copy of the same arrays: every call zeroes the words (8 B x capacity) and makes "
                "the plan and the map again.\n\n| mesh | n | tree | n_dirty | caller-owned ms | ctx's own tree ms |\n|---|---:|---|---:|---:|---:|\n")
        for r in owned_rows:
            f.write(f"| {r['mesh']} | {r['n']} | {r['tree']} | {r['n_dirty']} | {cell(r['caller_owned_ms'])} | {cell(r['own_tree_ms'])} |\n")


if __name__ == "__main__":
    main()
