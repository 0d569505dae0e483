#!/usr/bin/env python3
"""time of bvh_scene_closest_tris, one process, one device.  Writes <out>/scene_closest_tris.json and <out>/scene_closest_tris.md, stamped with the library's
machine-code hash.  Both sides of every comparison are measured in the same run, in alternating windows.

  (1) one identity instance against bvh_closest_tris on the BLAS: the same queries (the mesh moved by (0.37, 0.11, -0.23) of its extent, the pair of
      tools/time_closest_tris.py), the same HPLOC tree, bunny-like 327 680 and Sponza-like 262 144; closest unbounded, closest in the 2e-3 x diagonal band,
      any in the band.  The ratio is the cost of the two-level machinery (DESIGN.md 8d's bar for scene-over-flat is 1.5x).
  (2) BVH_SCENE_TRIS_INSTANCE on the 64-instance grids of tools/time_scene_collide.py (4 x 4 x 4 at 0.6 of the extent): instance 21 against the other 63,
      closest unbounded / closest band / any band; beside it bvh_scene_intersect_tris count-only on the same rows, and what a caller had before: ONE flat
      build of the 63 instances' world triangles plus bvh_closest_tris on it, with the bytes that flat copy takes (--no-flat leaves it out).

HIP events on the context's stream, one warm-up call of every shape, then --windows windows of --reps calls; the median window is the figure, the smallest
and largest are kept as the spread.  Reported numbers, not gates.

    python tools/time_scene_closest_tris.py
    python tools/time_scene_closest_tris.py --scale 0.05 --reps 1 --windows 3      # a rehearsal at a small size
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

SHIFT = (0.37, 0.11, -0.23)
QUERY_MODE, INSTANCE_MODE = 0, 1
KINDS = (("closest_inf", "closest, unbounded"), ("closest_band", "closest, band"), ("any_band", "any, band"))
QUERY_INSTANCE = 21


def kind_args(pkg, name, band):
    return (float("inf") if name.endswith("inf") else band), (pkg.QUERY_ANY if name.startswith("any") else pkg.QUERY_CLOSEST)


def extent_of(tris):
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    return v.max(axis=0) - v.min(axis=0)


def moved_by(pkg, tris, d):
    out = np.zeros(len(tris), dtype=pkg.meshgen.TRIANGLE)
    for f in ("v1", "v2", "v3"):
        out[f] = (tris[f] + d.astype(np.float32)[None, :]).astype(np.float32)
    return out


def answers(pkg, rec):
    hit = rec["prim"] != pkg.INVALID
    return {"hits": int(hit.sum()), "crossings": int((hit & (rec["feature"] == 15)).sum()),
            "distance": float(np.sqrt(np.float64(rec["dist2"][hit].min()))) if hit.any() else float("inf")}


def one_instance(pkg, L, key, scale, n_windows, reps):
    """(1): bvh_closest_tris on the BLAS against bvh_scene_closest_tris on one identity instance of it"""
    title, n, gen = MESHES[key]
    tris = gen(pkg, max(int(n * scale), 64))
    n = len(tris)
    ext = extent_of(tris)
    band = float(2e-3 * np.linalg.norm(ext))
    other = moved_by(pkg, tris, np.array(SHIFT) * ext)
    bctx, sctx = pkg.Context(0), pkg.Context(0)
    bctx.reserve(n)
    d_tris, d_fq, d_fh = bctx.upload(tris), bctx.upload(other), bctx.alloc(n * 16)
    d_sq, d_sh = sctx.upload(other), sctx.alloc(n * 16)
    b = pkg.HPLOC().build(bctx, d_tris, on_device=True, n=n)
    res = b.result
    inst = np.zeros(1, dtype=pkg.INSTANCE)
    inst["object_to_world"][0, [0, 5, 10]] = 1.0
    sc = pkg.Scene(sctx).build(pkg.ALGO_HPLOC, [b], inst)
    fin = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_fq.ptr, None, None, 0, 0)
    sin = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_sq.ptr, None, None, 0, 0)
    fs, ss = stream_of(L, bctx), stream_of(L, sctx)
    work, fns = [], {}
    for name, _ in KINDS:
        radius, q = kind_args(pkg, name, band)
        fns["flat " + name] = (lambda r, k: lambda i: L.bvh_closest_tris(bctx.handle, C.byref(res), None, C.byref(fin), n, r, d_fh.ptr, k))(radius, q)
        fns["scene " + name] = (lambda r, k: lambda i: L.bvh_scene_closest_tris(sc.handle, C.byref(sin), n, QUERY_MODE, 0, r, d_sh.ptr, k))(radius, q)
        work += [("flat " + name, fs, fns["flat " + name]), ("scene " + name, ss, fns["scene " + name])]
    t = windows(work, n_windows, reps)
    row = {"mesh": f"{title}, {n:,} triangles", "n": n, "band": band, "times": t}
    for name, _ in KINDS:
        assert fns["flat " + name](0) == 0 and fns["scene " + name](0) == 0
        bctx.synchronize(); sctx.synchronize()
        f, s = d_fh.download(pkg.TRI_HIT, n), d_sh.download(pkg.INSTANCE_TRI_HIT, n)
        row[name] = {"ratio": t["scene " + name]["median"] / t["flat " + name]["median"], **answers(pkg, s),
                     "same_hit_records": bool(name.startswith("any") or s[s["prim"] != pkg.INVALID].tobytes() == f[f["prim"] != pkg.INVALID].tobytes())}
    row["kernels"] = kernel_split(sctx, fns["scene closest_inf"], reps=2)
    sc.close()
    for buf in (d_tris, d_fq, d_fh, d_sq, d_sh):
        buf.free()
    sctx.close(); bctx.close()
    return row


def world_copy(pkg, tris, inst, skip):
    """the world triangles of every instance but ``skip`` (translations only: the grid of cube_instances), concatenated in instance order"""
    parts = [moved_by(pkg, tris, inst["object_to_world"][k][[3, 7, 11]].astype(np.float64)) for k in range(len(inst)) if k != skip]
    return np.concatenate(parts)


def instance_grid(pkg, L, key, scale, n_windows, reps, flat):
    """(2): instance 21 of the 4 x 4 x 4 grid against the other 63"""
    title, n, gen = MESHES[key]
    tris = gen(pkg, max(int(n * scale), 64))
    n = len(tris)
    ext = extent_of(tris)
    band = float(2e-3 * np.linalg.norm(ext))
    inst = cube_instances(pkg, 4, 0.6 * ext)
    bctx, sctx = pkg.Context(0), pkg.Context(0)
    d_tris = bctx.upload(tris)
    b = pkg.HPLOC().build(bctx, d_tris, on_device=True, n=n)
    sc = pkg.Scene(sctx).build(pkg.ALGO_HPLOC, [b], inst)
    d_hits, d_off = sctx.alloc(n * 16), sctx.alloc((n + 1) * 4)
    ss = stream_of(L, sctx)
    fns = {}
    for name, _ in KINDS:
        radius, q = kind_args(pkg, name, band)
        fns[name] = (lambda r, k: lambda i: L.bvh_scene_closest_tris(sc.handle, None, n, INSTANCE_MODE, QUERY_INSTANCE, r, d_hits.ptr, k))(radius, q)
    fns["tris_count"] = lambda i: L.bvh_scene_intersect_tris(sc.handle, None, n, INSTANCE_MODE, QUERY_INSTANCE, 0, d_off.ptr, None, 0, None)
    work = [(name, ss, fn) for name, fn in fns.items()]
    row = {"mesh": f"{title}, {n:,} triangles", "n": n, "band": band, "instances": len(inst),
           "scene_bytes": int(n * 64 + (2 * n - 1) * 32 + n * 28 + len(inst) * (64 + 64 + 24 + 32 + 28 + 8))}
    keep = []
    if flat:                                                              # what a caller had before: one flat tree over the other 63 instances' world triangles
        fctx = pkg.Context(0)
        world = world_copy(pkg, tris, inst, QUERY_INSTANCE)
        nw = len(world)
        fctx.reserve(nw)
        d_world = fctx.upload(world)
        d_rows = fctx.upload(moved_by(pkg, tris, inst["object_to_world"][QUERY_INSTANCE][[3, 7, 11]].astype(np.float64)))
        d_fh = fctx.alloc(n * 16)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fst = stream_of(L, fctx)
        fb = pkg.HPLOC().build(fctx, d_world, on_device=True, n=nw)       # warm-up build
        e0.record(fst)
        fb = pkg.HPLOC().build(fctx, d_world, on_device=True, n=nw)
        e1.record(fst); e1.synchronize()
        row["flat_build_ms"] = e0.elapsed_time(e1)
        row["flat_bytes"] = int(nw * 64 + (2 * nw - 1) * 32 + nw * 28)   # triangles, nodes, leaf records of the flat copy (the build's scratch not counted)
        fres = fb.result
        rin = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_rows.ptr, None, None, 0, 0)
        for name, _ in KINDS:
            radius, q = kind_args(pkg, name, band)
            fn = (lambda r, k: lambda i: L.bvh_closest_tris(fctx.handle, C.byref(fres), None, C.byref(rin), n, r, d_fh.ptr, k))(radius, q)
            work.append(("flat " + name, fst, fn))
        keep = [fctx, d_world, d_rows, d_fh]
    row["times"] = windows(work, n_windows, reps)
    for name, _ in KINDS:
        assert fns[name](0) == 0
        sctx.synchronize()
        row[name] = answers(pkg, d_hits.download(pkg.INSTANCE_TRI_HIT, n))
    assert fns["tris_count"](0) == 0
    sctx.synchronize()
    row["tris_rows"] = int((np.diff(d_off.download(np.uint32, n + 1).astype(np.int64)) > 0).sum())
    row["kernels"] = kernel_split(sctx, fns["closest_inf"], reps=2)
    sc.close(); d_hits.free(); d_off.free(); d_tris.free()
    for x in keep[1:]:
        x.free()
    if keep:
        keep[0].close()
    sctx.close(); bctx.close()
    return row


def write_md(out, path):
    cell = lambda t: f"{t['median']:.3f} [{t['min']:.3f} .. {t['max']:.3f}]"
    L = [f"# Mesh-to-scene distance on one MI355X (`tools/time_scene_closest_tris.py --reps {out['reps']} --windows {out['windows']}`, "
         f"`profiles/scene_closest_tris.json`; machine code `{out['_kernel_source_hash']}`, the `kernel_source_hash` of `bench.py`)", "",
         f"{out['device']}.  HIP events on the context's stream, one warm-up call of every shape, then {out['windows']} windows of {out['reps']} calls timed in "
         "alternation; median window per call in ms, [smallest .. largest window].  band: radius 2e-3 of the extent's diagonal.  Reported numbers, not gates.", "",
         "## One identity instance against `bvh_closest_tris` on the BLAS", "",
         f"The queries are the mesh moved by {SHIFT} of its extent, one per triangle; the same HPLOC tree on both sides.", "",
         "| mesh | call | `bvh_closest_tris` ms | `bvh_scene_closest_tris` ms | scene / flat | hits | crossings | same hit records |", "|---|---|---|---|---|---|---|---|"]
    for r in out["one_instance"]:
        for name, label in KINDS:
            a = r[name]
            L.append(f"| {r['mesh']} | {label} | {cell(r['times']['flat ' + name])} | {cell(r['times']['scene ' + name])} | {a['ratio']:.2f}x | {a['hits']:,} | "
                     f"{a['crossings']:,} | {'yes' if a['same_hit_records'] else 'NO'}{' (hit / miss)' if name.startswith('any') else ''} |")
    L.append("")
    for r in out["one_instance"]:
        L += [f"Per kernel, unbounded closest call on the scene, {r['mesh']} (ms per launch, launches): " +
              ", ".join(f"`{k}` {v[0]:.4f} ({v[1]})" for k, v in sorted(r["kernels"].items())) + ".", ""]
    L += ["## `BVH_SCENE_TRIS_INSTANCE`: instance 21 of a 4 x 4 x 4 grid at 0.6 of the extent against the other 63", "",
          "| mesh | call | `bvh_scene_closest_tris` ms | flat tree over the 63 + `bvh_closest_tris` ms | hits | crossings | distance |", "|---|---|---|---|---|---|---|"]
    for r in out["instance_grid"]:
        for name, label in KINDS:
            a = r[name]
            fl = cell(r["times"]["flat " + name]) if "flat " + name in r["times"] else "not measured"
            L.append(f"| {r['mesh']} | {label} | {cell(r['times'][name])} | {fl} | {a['hits']:,} | {a['crossings']:,} | {a['distance']:.6g} |")
    L.append("")
    for r in out["instance_grid"]:
        L += [f"{r['mesh']}: `bvh_scene_intersect_tris` count-only on the same rows {cell(r['times']['tris_count'])} ms, {r['tris_rows']:,} crossing rows.  "
              f"The scene holds {r['scene_bytes'] / 1e6:,.0f} MB" +
              (f"; the flat copy of the other 63 instances {r['flat_bytes'] / 1e6:,.0f} MB and one HPLOC build of it {r['flat_build_ms']:.1f} ms, again after every move."
               if "flat_bytes" in r else ".") +
              "  Per kernel, unbounded closest call (ms per launch, launches): " +
              ", ".join(f"`{k}` {v[0]:.4f} ({v[1]})" for k, v in sorted(r["kernels"].items())) + ".", ""]
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--meshes", nargs="*", default=["bunny", "sponza"], choices=sorted(MESHES))
    ap.add_argument("--scale", type=float, default=1.0, help="scales the meshes' triangle counts (a rehearsal at a small size)")
    ap.add_argument("--no-flat", action="store_true", help="leave out the flat build of the 63 instances' world triangles")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(ROOT), "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    if not torch.cuda.is_available():
        sys.exit("time_scene_closest_tris.py needs the GPU: there is no fallback")
    torch.cuda.init()
    out = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "one_instance": [],
           "instance_grid": []}

    def save():
        os.makedirs(a.out, exist_ok=True)                                 # (after every shape: what has been measured is on disk)
        with open(os.path.join(a.out, "scene_closest_tris.json"), "w") as f:
            json.dump(out, f, indent=1)
        write_md(out, os.path.join(a.out, "scene_closest_tris.md"))
    for key in a.meshes:
        row = one_instance(pkg, L, key, a.scale, a.windows, a.reps)
        out["one_instance"].append(row)
        print(json.dumps({"one_instance": row["mesh"], **{name: row[name] for name, _ in KINDS}}), flush=True)
        save()
    for key in a.meshes:
        row = instance_grid(pkg, L, key, a.scale, a.windows, a.reps, not a.no_flat)
        out["instance_grid"].append(row)
        print(json.dumps({"instance_grid": row["mesh"], **{name: {**row[name], "ms": row["times"][name]["median"]} for name, _ in KINDS}}), flush=True)
        save()


if __name__ == "__main__":
    main()
