#!/usr/bin/env python3
"""time of bvh_scene_radius_tris, one process, one device.  Writes <out>/scene_radius_tris.json and <out>/scene_radius_tris.md, stamped with the library's
machine-code hash.  Both sides of every comparison are measured in the same run, in alternating windows.

  (1) one identity instance against bvh_radius_tris on the BLAS: the same queries (the mesh moved by (0.37, 0.11, -0.23) of its extent, the pair of
      tools/time_radius_tris.py and tools/time_scene_closest_tris.py), the same HPLOC tree, bunny-like 327 680 and Sponza-like 262 144, in the 2e-3 x diagonal
      band: count only, unsorted fill, sorted fill.  The ratio is the cost of the two-level machinery (DESIGN.md 8d's bar for scene-over-flat is 1.5x).
  (2) BVH_SCENE_TRIS_INSTANCE on the 64-instance grids of tools/time_scene_closest_tris.py (4 x 4 x 4 at 0.6 of the extent): instance 21 against the other
      63 in the band, count only / unsorted fill / sorted fill; beside it bvh_scene_closest_tris (closest, band) and bvh_scene_intersect_tris count-only on
      the same rows.

HIP events on the context's stream, one warm-up call of every shape, then --windows windows of --reps calls; the median window is the figure, the smallest
and largest are kept as the spread.  Reported numbers, not gates.

    python tools/time_scene_radius_tris.py
    python tools/time_scene_radius_tris.py --scale 0.05 --reps 1 --windows 3      # a rehearsal at a small size
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
from time_scene_closest_tris import INSTANCE_MODE, QUERY_INSTANCE, QUERY_MODE, SHIFT, extent_of, moved_by  # noqa: E402
from time_scene_intersect_tris import MESHES, cube_instances  # noqa: E402
from time_scene_knn import windows  # noqa: E402

PASSES = (("count", "count only"), ("fill", "count + unsorted fill"), ("sorted", "count + sorted fill"))


def slices_of(off):
    c = np.diff(off.astype(np.int64))
    return {"records": int(c.sum()), "nonempty": int((c > 0).sum()), "longest": int(c.max()) if len(c) else 0}


def one_instance(pkg, L, key, scale, n_windows, reps):
    """(1): bvh_radius_tris on the BLAS against bvh_scene_radius_tris on one identity instance of it"""
    title, n, gen = MESHES[key]
    tris = gen(pkg, max(int(n * scale), 64))
    n = len(tris)
    ext = extent_of(tris)
    band = float(2e-3 * np.linalg.norm(ext))
    other = moved_by(pkg, tris, np.array(SHIFT) * ext)
    bctx, sctx = pkg.Context(0), pkg.Context(0)
    bctx.reserve(n)
    d_tris, d_fq, d_fo = bctx.upload(tris), bctx.upload(other), bctx.alloc((n + 1) * 4)
    d_sq, d_so = sctx.upload(other), sctx.alloc((n + 1) * 4)
    b = pkg.HPLOC().build(bctx, d_tris, on_device=True, n=n)
    res = b.result
    inst = np.zeros(1, dtype=pkg.INSTANCE)
    inst["object_to_world"][0, [0, 5, 10]] = 1.0
    sc = pkg.Scene(sctx).build(pkg.ALGO_HPLOC, [b], inst)
    fin = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_fq.ptr, None, None, 0, 0)
    sin = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_sq.ptr, None, None, 0, 0)
    total = C.c_uint64()
    assert L.bvh_scene_radius_tris(sc.handle, C.byref(sin), n, QUERY_MODE, 0, band, 0, d_so.ptr, None, 0, C.byref(total)) == 0
    cap = max(int(total.value), 1)
    d_fh, d_sh = bctx.alloc(cap * 16), sctx.alloc(cap * 16)
    fs, ss = stream_of(L, bctx), stream_of(L, sctx)
    work, fns = [], {}
    for name, _ in PASSES:
        fh, sh, flags = (None, None, 0) if name == "count" else (d_fh.ptr, d_sh.ptr, 1 if name == "sorted" else 0)
        fns["flat " + name] = (lambda h, fl: lambda i: L.bvh_radius_tris(bctx.handle, C.byref(res), None, C.byref(fin), n, band, fl, d_fo.ptr, h, cap, None))(fh, flags)
        fns["scene " + name] = (lambda h, fl: lambda i: L.bvh_scene_radius_tris(sc.handle, C.byref(sin), n, QUERY_MODE, 0, band, fl, d_so.ptr, h, cap, None))(sh, flags)
        work += [("flat " + name, fs, fns["flat " + name]), ("scene " + name, ss, fns["scene " + name])]
    t = windows(work, n_windows, reps)
    assert fns["flat sorted"](0) == 0 and fns["scene sorted"](0) == 0
    bctx.synchronize(); sctx.synchronize()
    fo, so = d_fo.download(np.uint32, n + 1), d_so.download(np.uint32, n + 1)
    same = bool(fo.tobytes() == so.tobytes() and d_fh.download(pkg.TRI_HIT, int(fo[-1])).tobytes() == d_sh.download(pkg.INSTANCE_TRI_HIT, int(so[-1])).tobytes())
    row = {"mesh": f"{title}, {n:,} triangles", "n": n, "band": band, "times": t, "same_bytes": same, **slices_of(so),
           "ratio": {name: t["scene " + name]["median"] / t["flat " + name]["median"] for name, _ in PASSES},
           "kernels": kernel_split(sctx, fns["scene sorted"], reps=2)}
    sc.close()
    for buf in (d_tris, d_fq, d_fo, d_fh, d_sq, d_so, d_sh):
        buf.free()
    sctx.close(); bctx.close()
    return row


def instance_grid(pkg, L, key, scale, n_windows, reps):
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
    d_off, d_xoff, d_closest = sctx.alloc((n + 1) * 4), sctx.alloc((n + 1) * 4), sctx.alloc(n * 16)
    total = C.c_uint64()
    assert L.bvh_scene_radius_tris(sc.handle, None, n, INSTANCE_MODE, QUERY_INSTANCE, band, 0, d_off.ptr, None, 0, C.byref(total)) == 0
    cap = max(int(total.value), 1)
    d_hits = sctx.alloc(cap * 16)
    ss = stream_of(L, sctx)
    fns = {}
    for name, _ in PASSES:
        h, flags = (None, 0) if name == "count" else (d_hits.ptr, 1 if name == "sorted" else 0)
        fns[name] = (lambda h, fl: lambda i: L.bvh_scene_radius_tris(sc.handle, None, n, INSTANCE_MODE, QUERY_INSTANCE, band, fl, d_off.ptr, h, cap, None))(h, flags)
    fns["closest_band"] = lambda i: L.bvh_scene_closest_tris(sc.handle, None, n, INSTANCE_MODE, QUERY_INSTANCE, band, d_closest.ptr, pkg.QUERY_CLOSEST)
    fns["tris_count"] = lambda i: L.bvh_scene_intersect_tris(sc.handle, None, n, INSTANCE_MODE, QUERY_INSTANCE, 0, d_xoff.ptr, None, 0, None)
    row = {"mesh": f"{title}, {n:,} triangles", "n": n, "band": band, "instances": len(inst),
           "times": windows([(name, ss, fn) for name, fn in fns.items()], n_windows, reps)}
    assert fns["sorted"](0) == 0 and fns["closest_band"](0) == 0
    sctx.synchronize()
    off = d_off.download(np.uint32, n + 1)
    hits, closest = d_hits.download(pkg.INSTANCE_TRI_HIT, int(off[-1])), d_closest.download(pkg.INSTANCE_TRI_HIT, n)
    nonempty = np.diff(off.astype(np.int64)) > 0
    row.update(slices_of(off))
    row["crossings"] = int((hits["feature"] == 15).sum())
    row["first_is_closest"] = bool(np.array_equal(nonempty, closest["prim"] != pkg.INVALID) and hits[off[:-1][nonempty]].tobytes() == closest[nonempty].tobytes())
    row["kernels"] = kernel_split(sctx, fns["sorted"], reps=2)
    sc.close()
    for buf in (d_hits, d_off, d_xoff, d_closest, d_tris):
        buf.free()
    sctx.close(); bctx.close()
    return row


def write_md(out, path):
    cell = lambda t: f"{t['median']:.3f} [{t['min']:.3f} .. {t['max']:.3f}]"
    L = [f"# Every triangle within a radius, on scenes, on one MI355X (`tools/time_scene_radius_tris.py --reps {out['reps']} --windows {out['windows']}`, "
         f"`profiles/scene_radius_tris.json`; machine code `{out['_kernel_source_hash']}`, the `kernel_source_hash` of `bench.py`)", "",
         f"{out['device']}.  HIP events on the context's stream, one warm-up call of every shape, then {out['windows']} windows of {out['reps']} calls timed in "
         "alternation; median window per call in ms, [smallest .. largest window].  Radius: 2e-3 of the extent's diagonal.  Reported numbers, not gates.", "",
         "## One identity instance against `bvh_radius_tris` on the BLAS", "",
         f"The queries are the mesh moved by {SHIFT} of its extent, one per triangle; the same HPLOC tree on both sides.", "",
         "| mesh | call | `bvh_radius_tris` ms | `bvh_scene_radius_tris` ms | scene / flat | records | non-empty slices | longest slice | same bytes |",
         "|---|---|---|---|---|---|---|---|---|"]
    for r in out["one_instance"]:
        for name, label in PASSES:
            L.append(f"| {r['mesh']} | {label} | {cell(r['times']['flat ' + name])} | {cell(r['times']['scene ' + name])} | {r['ratio'][name]:.2f}x | {r['records']:,} | "
                     f"{r['nonempty']:,} | {r['longest']:,} | {'yes' if r['same_bytes'] else 'NO'} |")
    L.append("")
    for r in out["one_instance"]:
        L += [f"Per kernel, sorted call on the scene, {r['mesh']} (ms per launch, launches): " +
              ", ".join(f"`{k}` {v[0]:.4f} ({v[1]})" for k, v in sorted(r["kernels"].items())) + ".", ""]
    L += ["## `BVH_SCENE_TRIS_INSTANCE`: instance 21 of a 4 x 4 x 4 grid at 0.6 of the extent against the other 63", "",
          "| mesh | call | ms | records | non-empty slices | longest slice | crossings | first record = `bvh_scene_closest_tris` |", "|---|---|---|---|---|---|---|---|"]
    for r in out["instance_grid"]:
        for name, label in PASSES:
            L.append(f"| {r['mesh']} | {label} | {cell(r['times'][name])} | {r['records']:,} | {r['nonempty']:,} | {r['longest']:,} | {r['crossings']:,} | "
                     f"{'yes' if r['first_is_closest'] else 'NO'} |")
    L.append("")
    for r in out["instance_grid"]:
        L += [f"{r['mesh']}: `bvh_scene_closest_tris` (closest, the same radius) on the same rows {cell(r['times']['closest_band'])} ms, `bvh_scene_intersect_tris` "
              f"count-only {cell(r['times']['tris_count'])} ms.  Per kernel, sorted call (ms per launch, launches): " +
              ", ".join(f"`{k}` {v[0]:.4f} ({v[1]})" for k, v in sorted(r["kernels"].items())) + ".", ""]
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--meshes", nargs="*", default=["bunny", "sponza"], choices=sorted(MESHES))
    ap.add_argument("--scale", type=float, default=1.0, help="scales the meshes' triangle counts (a rehearsal at a small size)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(ROOT), "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    if not torch.cuda.is_available():
        sys.exit("time_scene_radius_tris.py needs the GPU: there is no fallback")
    torch.cuda.init()
    out = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "one_instance": [],
           "instance_grid": []}

    def save():
        os.makedirs(a.out, exist_ok=True)                                 # (after every shape: what has been measured is on disk)
        with open(os.path.join(a.out, "scene_radius_tris.json"), "w") as f:
            json.dump(out, f, indent=1)
        write_md(out, os.path.join(a.out, "scene_radius_tris.md"))
    for key in a.meshes:
        row = one_instance(pkg, L, key, a.scale, a.windows, a.reps)
        out["one_instance"].append(row)
        print(json.dumps({"one_instance": row["mesh"], "ratio": row["ratio"], "records": row["records"], "same_bytes": row["same_bytes"]}), flush=True)
        save()
    for key in a.meshes:
        row = instance_grid(pkg, L, key, a.scale, a.windows, a.reps)
        out["instance_grid"].append(row)
        print(json.dumps({"instance_grid": row["mesh"], "records": row["records"], "first_is_closest": row["first_is_closest"],
                          **{name: row["times"][name]["median"] for name, _ in PASSES}}), flush=True)
        save()


if __name__ == "__main__":
    main()
