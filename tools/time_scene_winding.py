#!/usr/bin/env python3
"""time of bvh_scene_winding_prepare and bvh_scene_winding_number on the README's scenes; one process, one device.

  instancing  64 instances (an 8 x 8 grid, tools/time_scene.py's) of bunny-like 327 680 and of Sponza-like 262 144 against (a) bvh_winding_number on ONE flat
              HPLOC build of the 64 x n world triangles
  overhead    (b) one identity instance against the flat call on the BLAS itself
  bodies      4 096 bvh_build_many bodies of 512 triangles (bunny-like 512 at random similarity transforms), the scene alone
  prepare     (c) bvh_scene_winding_prepare in full and with BVH_SCENE_WINDING_KEEP_BLAS, on each scene
  error       (d) max |answer - f64 brute force over the world triangles| at each beta, on --check points of a reduced copy of the scene (the same instances over a
              small mesh of the same kind: the brute force is quadratic)
--points points (2^20) uniform in the scene box grown by a tenth, beta 2 / 3 / 4.  Timed with HIP events on the context's stream, one warm-up call, then --windows
windows of --reps calls in alternation; the median window is the figure, the smallest and largest are the spread.
Writes <out>/scene_winding.json and <out>/scene_winding.md.

    python tools/time_scene_winding.py
    python tools/time_scene_winding.py --skip-flat      # no flattened 64-copy builds (host memory / time)
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
from time_query import timed  # noqa: E402
from time_scene import grid_instances, stream_of  # noqa: E402

BETAS = (2.0, 3.0, 4.0)


def world_tris(tris, m34):
    """the scene's world triangles of one instance, in the header's order, f32"""
    m = np.asarray(m34, dtype=np.float32)
    out = tris.copy()
    for f in ("v1", "v2", "v3"):
        p = tris[f]
        out[f] = np.stack([((m[4 * i] * p[:, 0] + m[4 * i + 1] * p[:, 1]) + m[4 * i + 2] * p[:, 2]) + m[4 * i + 3] for i in range(3)], axis=1)
    return out


def box_points(pkg, lo, hi, m, seed):
    rng = np.random.default_rng(seed)
    ext = hi - lo
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    pts["point"] = (lo - 0.1 * ext + rng.random((m, 3)) * 1.2 * ext).astype(np.float32)
    pts["radius"] = np.inf
    return pts


def brute_force(wt, xyz, chunk=1 << 22):
    """f64 sum of the Van Oosterom-Strackee solid angles over 4 pi"""
    a0, b0, c0 = (wt[f].astype(np.float64) for f in ("v1", "v2", "v3"))
    out = np.zeros(len(xyz))
    step = max(1, chunk // len(wt))
    for s in range(0, len(xyz), step):
        q = xyz[s:s + step].astype(np.float64)[:, None, :]
        a, b, c = a0[None] - q, b0[None] - q, c0[None] - q
        num = (a * np.cross(b, c)).sum(axis=2)
        la, lb, lc = (np.linalg.norm(x, axis=2) for x in (a, b, c))
        den = la * lb * lc + (a * b).sum(axis=2) * lc + (b * c).sum(axis=2) * la + (c * a).sum(axis=2) * lb
        out[s:s + step] = (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)
    return out


def windows(stream, work, n_windows, reps):
    for _, fn in work:
        fn(0)                                                           # warm-up: every shape the windows use
    times = {name: [] for name, _ in work}
    for _ in range(n_windows):
        for name, fn in work:                                           # alternating
            times[name].append(timed(stream, fn, reps))
    return {name: {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))} for name, t in times.items()}


def scene_rows(pkg, L, a, sc, sc_ctx, stream, d_pts, d_w, m):
    def prep(flags):
        def fn(i):
            assert L.bvh_scene_winding_prepare(sc.handle, flags) == 0
        return fn

    def wind(beta):
        def fn(i):
            assert L.bvh_scene_winding_number(sc.handle, d_pts.ptr, m, beta, d_w.ptr) == 0
        return fn
    prep(0)(0)
    work = [("prepare_full", prep(0)), ("prepare_keep_blas", prep(pkg.SCENE_WINDING_KEEP_BLAS))] + [(f"beta{int(b)}", wind(b)) for b in BETAS]
    row = windows(stream, work, a.windows, a.reps)
    sc_ctx.set_profiling(2)
    prep(0)(0)
    for i in range(3):
        wind(2.0)(i)
    row["kernels"] = {k: (ms / cnt, cnt) for k, (ms, cnt) in sc_ctx.kernel_times().items()}
    sc_ctx.set_profiling(0)
    return row


def errors(pkg, blas_builder_ctx, small, inst, n_check, seed):
    """(d): the same instances over a small mesh, --check points, max |gpu - brute force| at each beta"""
    ctx = pkg.Context(0); sctx = pkg.Context(0)
    try:
        b = pkg.HPLOC().build(ctx, small)
        sc = pkg.Scene(sctx).build(pkg.ALGO_HPLOC, [b], inst)
        wt = np.concatenate([world_tris(small, inst["object_to_world"][k]) for k in range(len(inst))])
        v = np.concatenate([wt["v1"], wt["v2"], wt["v3"]]).astype(np.float64)
        pts = box_points(pkg, v.min(axis=0), v.max(axis=0), n_check, seed)
        bf = brute_force(wt, pts["point"])
        return {f"beta{int(beta)}": float(np.abs(sc.winding_number(pts, beta=beta).astype(np.float64) - bf).max()) for beta in BETAS}
    finally:
        sctx.close(); ctx.close()


def write_md(doc, path):
    def cell(t):
        return f"{t['median']:.3f} [{t['min']:.3f} .. {t['max']:.3f}]"
    out = ["# bvh_scene_winding_number: winding numbers on instanced scenes (tools/time_scene_winding.py)", "",
           f"{doc['device']}; {doc['points']:,} points per call, uniform in the scene box grown by a tenth; HIP events on the context's stream, one warm-up call, then "
           f"{doc['windows']} windows of {doc['reps']} calls in alternation; median window per call in ms, [smallest .. largest window].", "",
           "| scene | prepare ms | prepare KEEP_BLAS ms | beta 2 ms | beta 3 ms | beta 4 ms | flat beta 2 / 3 / 4 ms | scene / flat at beta 2 |", "|---|---|---|---|---|---|---|---|"]
    for r in doc["scenes"]:
        flat = r.get("flat")
        fl = " / ".join(f"{flat[f'beta{int(b)}']['median']:.3f}" for b in BETAS) if flat else "not measured"
        ratio = f"{r['beta2']['median'] / flat['beta2']['median']:.2f}" if flat else "n/a"
        out.append(f"| {r['name']} | {cell(r['prepare_full'])} | {cell(r['prepare_keep_blas'])} | {cell(r['beta2'])} | {cell(r['beta3'])} | {cell(r['beta4'])} | {fl} | {ratio} |")
    out += ["", "## one identity instance against bvh_winding_number on the BLAS", "", "| mesh | scene beta 2 / 3 / 4 ms | flat beta 2 / 3 / 4 ms | ratio at beta 2 | same bytes at beta 2 |",
            "|---|---|---|---|---|"]
    for r in doc["overhead"]:
        out.append(f"| {r['name']} | " + " / ".join(f"{r['scene'][f'beta{int(b)}']['median']:.3f}" for b in BETAS) + " | " +
                   " / ".join(f"{r['flat'][f'beta{int(b)}']['median']:.3f}" for b in BETAS) +
                   f" | {r['scene']['beta2']['median'] / r['flat']['beta2']['median']:.2f} | {r['same_bytes_fraction']:.6f} |")
    out += ["", "## max |answer - f64 brute force| on a reduced copy of each scene", "", "| scene | triangles per body | points | beta 2 | beta 3 | beta 4 |", "|---|---|---|---|---|---|"]
    for r in doc["scenes"]:
        e = r["error"]
        out.append(f"| {r['name']} | {e['small_n']} | {e['points']} | {e['beta2']:.4f} | {e['beta3']:.4f} | {e['beta4']:.4f} |")
    out.append("")
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=4096, help="points of the brute-force comparison")
    ap.add_argument("--bodies", type=int, default=4096)
    ap.add_argument("--skip-flat", action="store_true", help="no flattened 64-copy builds (host memory / time)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(ROOT), "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    m = a.points
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "points": m, "scenes": [], "overhead": []}
    sc_ctx = pkg.Context(0); s_scene = stream_of(L, sc_ctx)
    d_w = sc_ctx.alloc(m * 4)
    for kind, n, small_n in (("bunny", 327_680, 320), ("sponza", 262_144, 1024)):
        gen = pkg.meshgen.bunny_like if kind == "bunny" else (lambda k: pkg.meshgen.sponza_like(k, 3))
        tris = gen(n)
        bctx = pkg.Context(0); s_blas = stream_of(L, bctx)
        d_tris = bctx.upload(tris)
        b = pkg.HPLOC().build(bctx, d_tris, on_device=True, n=n)
        v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        # (b) one identity instance against the flat call on the BLAS
        one = grid_instances(pkg, 1, (0, 0, 0))
        sc = pkg.Scene(sc_ctx).build(pkg.ALGO_HPLOC, [b], one)
        pts = box_points(pkg, lo, hi, m, 1)
        d_sp, d_bp = sc_ctx.upload(pts), bctx.upload(pts)
        d_mom, d_bw = bctx.alloc((n - 1) * 32), bctx.alloc(m * 4)
        assert L.bvh_winding_prepare(bctx.handle, C.byref(b.result), None, d_mom.ptr) == 0
        flat_fn = lambda beta: (lambda i: L.bvh_winding_number(bctx.handle, C.byref(b.result), None, d_mom.ptr, d_bp.ptr, m, beta, d_bw.ptr))
        row = {"name": f"{kind}_{n}", "scene": scene_rows(pkg, L, a, sc, sc_ctx, s_scene, d_sp, d_w, m),
               "flat": windows(s_blas, [(f"beta{int(bt)}", flat_fn(bt)) for bt in BETAS], a.windows, a.reps)}
        assert L.bvh_scene_winding_number(sc.handle, d_sp.ptr, m, 2.0, d_w.ptr) == 0 and flat_fn(2.0)(0) == 0
        row["same_bytes_fraction"] = float((d_w.download(np.uint32, m) == d_bw.download(np.uint32, m)).mean())
        doc["overhead"].append(row); print(json.dumps(row), flush=True)
        sc.close()
        for x in (d_sp, d_bp, d_mom, d_bw):
            x.free()
        # (a) 64 instances against one flat build of the world triangles
        inst = grid_instances(pkg, 8, (hi - lo) * 1.1)
        t = inst["object_to_world"].reshape(-1, 3, 4)[:, :, 3].astype(np.float64)
        sc = pkg.Scene(sc_ctx).build(pkg.ALGO_HPLOC, [b], inst)
        pts = box_points(pkg, lo + t.min(axis=0), hi + t.max(axis=0), m, 2)
        d_sp = sc_ctx.upload(pts)
        row = {"name": f"64 x {kind}_{n}", **scene_rows(pkg, L, a, sc, sc_ctx, s_scene, d_sp, d_w, m)}
        row["error"] = {"small_n": small_n, "points": a.check, **errors(pkg, bctx, gen(small_n), inst, a.check, 3)}
        sc.close(); d_sp.free()
        if not a.skip_flat:
            flat = np.concatenate([world_tris(tris, inst["object_to_world"][k]) for k in range(64)])
            fctx = pkg.Context(0); s_flat = stream_of(L, fctx)
            fctx.reserve(64 * n)
            d_flat = fctx.upload(flat); del flat
            fb = pkg.HPLOC()
            assert L.bvh_build(fctx.handle, pkg.ALGO_HPLOC, d_flat.ptr, 64 * n, 1, C.byref(fb.result), None) == 0
            d_fm, d_fp, d_fw = fctx.alloc((64 * n - 1) * 32), fctx.upload(pts), fctx.alloc(m * 4)
            assert L.bvh_winding_prepare(fctx.handle, C.byref(fb.result), None, d_fm.ptr) == 0
            ffn = lambda beta: (lambda i: L.bvh_winding_number(fctx.handle, C.byref(fb.result), None, d_fm.ptr, d_fp.ptr, m, beta, d_fw.ptr))
            row["flat"] = windows(s_flat, [(f"beta{int(bt)}", ffn(bt)) for bt in BETAS], a.windows, a.reps)
            for x in (d_flat, d_fm, d_fp, d_fw):
                x.free()
            fctx.close()
        doc["scenes"].append(row); print(json.dumps({k: v for k, v in row.items() if k != "kernels"}), flush=True)
        d_tris.free(); bctx.close()
    # 4 096 bvh_build_many bodies of 512 triangles at random similarity transforms
    nb, per = a.bodies, 512
    body = pkg.meshgen.bunny_like(per)
    rng = np.random.default_rng(7)
    mctx = pkg.Context(0)
    many = mctx.build_many([body] * nb)
    side = int(np.ceil(nb ** (1 / 3)))
    mats = np.zeros((nb, 12), dtype=np.float32)
    for k in range(nb):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(0, 2 * np.pi)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        mats[k] = np.concatenate([rng.uniform(0.5, 1.5) * R, (np.array([k % side, (k // side) % side, k // (side * side)]) * 4.0)[:, None]], axis=1).reshape(12)
    inst = np.zeros(nb, dtype=pkg.INSTANCE); inst["object_to_world"] = mats; inst["blas"] = np.arange(nb)
    mctx.synchronize()
    sc = pkg.Scene(sc_ctx).build(pkg.ALGO_HPLOC, [many.blas(k) for k in range(nb)], inst)
    pts = box_points(pkg, np.full(3, -2.0), np.full(3, side * 4.0), m, 5)
    d_sp = sc_ctx.upload(pts)
    row = {"name": f"{nb} build_many bodies of {per}", **scene_rows(pkg, L, a, sc, sc_ctx, s_scene, d_sp, d_w, m)}
    sub = inst[:64].copy(); sub["blas"] = 0
    row["error"] = {"small_n": per, "points": a.check, **errors(pkg, mctx, body, sub, a.check, 6)}
    doc["scenes"].append(row); print(json.dumps({k: v for k, v in row.items() if k != "kernels"}), flush=True)
    sc.close(); d_sp.free(); many.free(); mctx.close()
    d_w.free(); sc_ctx.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "scene_winding.json"), "w") as f:
        json.dump(doc, f, indent=1)
    write_md(doc, os.path.join(a.out, "scene_winding.md"))


if __name__ == "__main__":
    main()
