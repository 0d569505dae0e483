#!/usr/bin/env python3
"""time of convex-volume queries on instanced scenes (bvh_scene_cull), one process, one device.  Writes <out>/scene_cull.json and <out>/scene_cull.md,
stamped with the library's machine-code hash.

  one instance   one identity instance over the Sponza-like 262 144 mesh (HPLOC BLAS) against bvh_cull on the same tree with the same path: the bar of
                 DESIGN.md §8d (within 1.5x), on the camera frustum and on the tile frusta
  64 instances   the scenes of tools/time_scene_overlap.py — an 8 x 8 grid of one mesh, bunny-like 327 680 and Sponza-like 262 144 — under one camera
                 frustum and under the 120 x 68 tile frusta of a 1920 x 1080 view of the whole grid
  4 096 bodies   4 096 bvh_build_many trees of 512 triangles each on a 16 x 16 x 16 grid, the same two volume sets
Every case is measured count-only and count + fill (the capacity is the total, no read-back) through both forced walks.  Beside each: bvh_cull (group walk)
on one flat HPLOC build of the world triangles — time, record count, bytes held by the flat tree and its triangles against the scene's — and
Scene.cull_instances' call (bvh_cull on the top-level tree) alone.  (--skip-flat: without the flat builds.)
Method (tools/time_cull.py's): HIP events on the context's stream around --reps calls after one warm call; a call whose warm run took longer than --long-s
seconds on the host clock is not repeated: that run is its figure (marked "1 call, host clock").  The kernels' registers, scratch and LDS are read from
the compiler (-Rpass-analysis=kernel-resource-usage on csrc/scene_cull.hip) when hipcc is there.

    python tools/time_scene_cull.py
    python tools/time_scene_cull.py --scale 0.05 --reps 2 --skip-flat      # a rehearsal at a small size
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(ROOT)); sys.path.insert(0, ROOT)
import bvh_pkg  # noqa: E402
from _srchash import kernel_source_hash  # noqa: E402
from time_cull import look_at, perspective, window_planes  # noqa: E402
from time_query import timed  # noqa: E402
from time_scene import grid_instances  # noqa: E402
from time_scene_radius import world_copies  # noqa: E402

PATHS = (("lane", 1), ("group", 2))


def resource_usage():
    """{kernel: {vgprs, sgprs, scratch, lds, occupancy}} of csrc/scene_cull.hip as the Makefile compiles it, or {} without hipcc"""
    csrc = os.path.join(os.path.dirname(ROOT), "hip-bvh-construction_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return {}
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(os.path.dirname(ROOT), "include"), "-I" + csrc,
           "-mllvm", "-amdgpu-kernarg-preload-count=16", "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(csrc, "scene_cull.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void bvh::", "") or m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z\[\]/ ]+?): (\d+)", line)
        if m and name and m.group(1).strip() in keys:
            out[name][keys[m.group(1).strip()]] = int(m.group(2))
    return out


def view_volumes(pkg, lo, hi):
    """(camera frustum (1, 6, 4), the 120 x 68 tile frusta of the same 1920 x 1080 view (8160, 6, 4)) of a camera above a corner of [lo, hi] looking at its centre"""
    ext = hi - lo; diag = float(np.linalg.norm(ext)); ctr = 0.5 * (lo + hi)
    clip = perspective(np.radians(60.0), 16.0 / 9.0, 0.01 * diag, 2.0 * diag) @ look_at(hi + 0.1 * ext, ctr)
    tx, ty = 1920 // 16, -(-1080 // 16)
    ex = -1.0 + 2.0 * np.arange(tx + 1) * 16.0 / 1920.0; ey = np.minimum(-1.0 + 2.0 * np.arange(ty + 1) * 16.0 / 1080.0, 1.0)
    tiles = np.stack([window_planes(clip, ex[i], ex[i + 1], ey[j], ey[j + 1]) for j in range(ty) for i in range(tx)])
    return pkg.frustum_planes(clip)[None], tiles


class Timer:
    def __init__(self, L, ctx, reps, long_s):
        self.ctx, self.reps, self.long_s = ctx, reps, long_s
        self.stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))

    def ms(self, fn):
        """{ms, reps}: one warm call on the host clock; a short call is then timed with events over reps calls, a long one keeps the warm run's time"""
        self.ctx.synchronize()
        t0 = time.perf_counter()
        assert fn(0) == 0
        self.ctx.synchronize()
        warm = time.perf_counter() - t0
        if warm > self.long_s:
            return {"ms": warm * 1e3, "reps": 0}
        return {"ms": timed(self.stream, fn, self.reps), "reps": self.reps}


def measure(timer, ctx, planes, call, record_bytes, paths=PATHS):
    """call(path, d_planes, k, per, d_off, d_hits, capacity, total_out) -> rc; per path: total, count-only and count + fill figures"""
    k, per = planes.shape[0], planes.shape[1]
    d_planes, d_off = ctx.upload(np.ascontiguousarray(planes)), ctx.alloc((k + 1) * 4)
    out = {"volumes": k}
    for name, path in paths:
        total = C.c_uint64()
        assert call(path, d_planes.ptr, k, per, d_off.ptr, None, 0, C.byref(total)) == 0
        tot = int(total.value)
        d_hits = ctx.alloc(max(tot, 1) * record_bytes)
        out[name] = {"total": tot, "count": timer.ms(lambda i: call(path, d_planes.ptr, k, per, d_off.ptr, None, 0, None)),
                     "fill": timer.ms(lambda i: call(path, d_planes.ptr, k, per, d_off.ptr, d_hits.ptr, tot, None))}
        d_hits.free()
    d_planes.free(); d_off.free()
    return out


def cell(t):
    return f"{t['ms']:.3f} ms" + ("" if t["reps"] else " (1 call, host clock)")


def write_md(out, path):
    L = [f"# Convex-volume queries on instanced scenes on one MI355X (`tools/time_scene_cull.py --reps {out['reps']}`, `profiles/scene_cull.json`; machine code "
         f"`{out['_kernel_source_hash']}`, the `kernel_source_hash` of `bench.py`)", "",
         f"{out['device']}.  HIP events on the context's stream around {out['reps']} calls after one warm call; a call longer than {out['long_s']} s is run once and "
         "timed on the host clock.  count: a count-only call; fill: a call that counts and fills (capacity = the total, no read-back).", ""]
    for row in out["rows"]:
        L += [f"## {row['scene']}", "", f"Scene holds {row['scene_bytes']:,} bytes (BLAS nodes, leaves and triangles once, instance records, top-level tree)"
              + (f"; the flat HPLOC build of the {row['world_tris']:,} world triangles holds {row['flat_bytes']:,} bytes." if row.get("flat_bytes") else "."), ""]
        L += ["| volumes | call | `bvh_scene_cull` lane | `bvh_scene_cull` group | records | " + ("`bvh_cull`, same tree, lane | `bvh_cull`, same tree, group | lane ratio | group ratio |"
              if row.get("same_tree") else "`bvh_cull` flat, group | flat records | `Scene.cull_instances` (group) | instances passed |"),
              "|---|---|---|---|---|---|---|---|---|"]
        for case in row["cases"]:
            s = case["scene"]
            for p in ("count", "fill"):
                line = f"| {case['name']} ({s['volumes']:,}) | {p} | {cell(s['lane'][p])} | {cell(s['group'][p])} | {s['group']['total']:,} | "
                if row.get("same_tree"):
                    f = case["flat"]
                    line += (f"{cell(f['lane'][p])} | {cell(f['group'][p])} | {s['lane'][p]['ms'] / f['lane'][p]['ms']:.2f}x | "
                             f"{s['group'][p]['ms'] / f['group'][p]['ms']:.2f}x |")
                else:
                    f, t = case.get("flat"), case["tlas"]
                    line += (f"{cell(f['group'][p])} | {f['group']['total']:,} | " if f else "not built | | ") + f"{cell(t['group'][p])} | {t['group']['total']:,} |"
                L.append(line)
        L.append("")
    L += ["## Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", ""]
    if out["resources"]:
        L += ["| kernel | VGPRs | SGPRs | scratch (bytes / lane) | LDS (bytes / block) | occupancy (waves / SIMD) |", "|---|---|---|---|---|---|"]
        for name, r in out["resources"].items():
            L.append(f"| `{name}` | {r.get('vgprs')} | {r.get('sgprs')} | {r.get('scratch')} | {r.get('lds')} | {r.get('occupancy')} |")
    else:
        L.append("not measured (no hipcc where the tool ran)")
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--long-s", type=float, default=2.0, help="a call whose warm run takes longer is not repeated")
    ap.add_argument("--scale", type=float, default=1.0, help="mesh sizes and body count times this (a rehearsal)")
    ap.add_argument("--skip-flat", action="store_true", help="no flat HPLOC builds of the world triangles (device memory / time)")
    ap.add_argument("--skip-lane-camera", action="store_true", help="no lane walk of the single camera frustum on the 64-instance scenes (tens of seconds per call)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(ROOT), "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    out = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "long_s": a.long_s, "scale": a.scale,
           "resources": resource_usage(), "rows": []}
    scene_ctx, bctx = pkg.Context(0), pkg.Context(0)
    st, bt = Timer(L, scene_ctx, a.reps, a.long_s), Timer(L, bctx, a.reps, a.long_s)

    def dump():
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "scene_cull.json"), "w") as f:
            json.dump(out, f, indent=1)
        write_md(out, os.path.join(a.out, "scene_cull.md"))

    def scene_call(sc):
        return lambda path, p, k, per, o, h, cap, tot: L.bvh_scene_cull(sc.handle, p, k, per, path, o, h, cap, tot)

    def tree_call(ctx, res):
        return lambda path, p, k, per, o, h, cap, tot: L.bvh_cull(ctx.handle, C.byref(res), p, k, per, path, o, h, cap, tot)

    def bounds(tris, inst):
        v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
        t = inst["object_to_world"].reshape(-1, 3, 4)[:, :, 3].astype(np.float64)
        return v.min(axis=0) + t.min(axis=0), v.max(axis=0) + t.max(axis=0)

    def blas_bytes(n, layout):
        return (2 * n - 1) * 32 + (n * 32 if layout == 1 else 0) + n * 64

    def grid_case(label, tris, same_tree):
        n = len(tris)
        d_tris = bctx.upload(tris)
        b = pkg.HPLOC().build(bctx, d_tris, on_device=True, n=n)
        v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
        inst = grid_instances(pkg, 1 if same_tree else 8, (v.max(axis=0) - v.min(axis=0)) * 1.1)
        bctx.synchronize()
        sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [b], inst)
        row = {"scene": label, "same_tree": same_tree, "world_tris": n * len(inst), "scene_bytes": blas_bytes(n, int(b.result.layout)) + len(inst) * (64 + 64 + 24 + 64),
               "cases": []}
        flat_ctx = flat = d_world = None
        if not same_tree and not a.skip_flat:
            flat_ctx = pkg.Context(0)
            d_world = flat_ctx.upload(world_copies(pkg, tris, inst))
            flat = pkg.HPLOC().build(flat_ctx, d_world, on_device=True, n=n * len(inst))
            row["flat_bytes"] = blas_bytes(n * len(inst), int(flat.result.layout))
        camera, tiles = view_volumes(pkg, *bounds(tris, inst))
        for name, vols in (("camera", camera), ("tiles", tiles)):
            paths = (("group", 2),) if name == "camera" and not same_tree and a.skip_lane_camera else PATHS
            case = {"name": name, "scene": measure(st, scene_ctx, vols, scene_call(sc), 16, paths)}
            case["scene"].setdefault("lane", {"total": case["scene"]["group"]["total"], "count": {"ms": float("nan"), "reps": 0}, "fill": {"ms": float("nan"), "reps": 0}})
            if same_tree:
                case["flat"] = measure(bt, bctx, vols, tree_call(bctx, b.result), 8)
                case["same_total"] = case["flat"]["group"]["total"] == case["scene"]["group"]["total"]
            else:
                case["tlas"] = measure(st, scene_ctx, vols, tree_call(scene_ctx, sc.tlas()), 8, (("group", 2),))
                if flat is not None:
                    ft = Timer(L, flat_ctx, a.reps, a.long_s)
                    case["flat"] = measure(ft, flat_ctx, vols, tree_call(flat_ctx, flat.result), 8, (("group", 2),))
            row["cases"].append(case)
            print(json.dumps({"scene": label, "case": name, "scene_ms": {p: {k: case["scene"][p][k]["ms"] for k in ("count", "fill")} for p in ("lane", "group")},
                              "records": case["scene"]["group"]["total"]}), flush=True)
        out["rows"].append(row); dump()
        sc.close(); d_tris.free()
        if flat_ctx is not None:
            d_world.free(); flat_ctx.close()

    sponza = pkg.meshgen.sponza_like(max(int(262_144 * a.scale), 64), 3)
    bunny = pkg.meshgen.bunny_like(max(int(327_680 * a.scale), 64), 2)
    grid_case(f"one identity instance, Sponza-like {len(sponza):,}", sponza, True)
    grid_case(f"64 instances, bunny-like {len(bunny):,}", bunny, False)
    grid_case(f"64 instances, Sponza-like {len(sponza):,}", sponza, False)

    # ---- 4 096 bvh_build_many bodies of 512 triangles on a 16 x 16 x 16 grid
    side = max(int(round(16 * a.scale ** (1 / 3))), 2); bodies, per_body = side ** 3, 512
    tris = pkg.meshgen.uniform(bodies * per_body, 7)
    ranges = np.stack([np.arange(bodies) * per_body, np.full(bodies, per_body)], axis=1)
    mt = bctx.build_many((tris, ranges))
    bctx.synchronize()
    k = np.arange(bodies)
    inst = np.zeros(bodies, dtype=pkg.INSTANCE)
    m = np.zeros((bodies, 12), dtype=np.float32); m[:, 0] = m[:, 5] = m[:, 10] = 0.5
    m[:, 3] = k % side; m[:, 7] = (k // side) % side; m[:, 11] = k // (side * side)
    inst["object_to_world"] = m; inst["blas"] = k
    sc = pkg.Scene(scene_ctx).build(pkg.ALGO_HPLOC, [mt.blas(j) for j in range(bodies)], inst)
    row = {"scene": f"{bodies:,} bvh_build_many bodies of {per_body} triangles", "same_tree": False, "world_tris": bodies * per_body,
           "scene_bytes": bodies * blas_bytes(per_body, 0) + bodies * (64 + 64 + 24 + 64 + 64), "cases": []}
    flat_ctx = flat = None
    if not a.skip_flat:
        world = np.zeros(len(tris), dtype=pkg.meshgen.TRIANGLE)
        shift = np.repeat(m[:, [3, 7, 11]], per_body, axis=0)
        for f in ("v1", "v2", "v3"):
            world[f] = tris[f] * np.float32(0.5) + shift
        flat_ctx = pkg.Context(0)
        d_world = flat_ctx.upload(world)
        flat = pkg.HPLOC().build(flat_ctx, d_world, on_device=True, n=len(world))
        row["flat_bytes"] = blas_bytes(len(world), int(flat.result.layout))
    camera, tiles = view_volumes(pkg, np.zeros(3), np.full(3, side - 0.5))
    for name, vols in (("camera", camera), ("tiles", tiles)):
        case = {"name": name, "scene": measure(st, scene_ctx, vols, scene_call(sc), 16),
                "tlas": measure(st, scene_ctx, vols, tree_call(scene_ctx, sc.tlas()), 8, (("group", 2),))}
        if flat is not None:
            case["flat"] = measure(Timer(L, flat_ctx, a.reps, a.long_s), flat_ctx, vols, tree_call(flat_ctx, flat.result), 8, (("group", 2),))
        row["cases"].append(case)
        print(json.dumps({"scene": row["scene"], "case": name, "scene_ms": {p: {q: case["scene"][p][q]["ms"] for q in ("count", "fill")} for p in ("lane", "group")},
                          "records": case["scene"]["group"]["total"]}), flush=True)
    out["rows"].append(row); dump()
    sc.close()
    if flat_ctx is not None:
        flat_ctx.close()
    scene_ctx.close(); bctx.close()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("time_scene_cull.py needs the GPU: there is no fallback")
    main()
