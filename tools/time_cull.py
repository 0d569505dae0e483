#!/usr/bin/env python3
"""time of bvh_cull through both walks, with bvh_overlap of each volume's bounding box on the same tree beside it; one process, one device.

Workloads, on a Sponza-like mesh of 262 144 triangles and a uniform one of 10 M:
  camera  one camera frustum (eye outside a corner of the scene, looking at its centre, 60 degrees, 16:9), all four builders;
  tiles   the 120 x 68 frusta of the 16 x 16-pixel tiles of a 1920 x 1080 view of the same camera, all four builders;
  sweep   random small frusta (eye uniform in the scene box, random direction, 5 to 20 degrees, reaching 10 to 30 % of the scene diagonal), 1 / 16 / 256 /
          4096 / 65 536 of them, on the HPLOC tree: the crossover between the lane walk and the group walk that BVH_CULL_AUTO's rule stands for.
Every workload runs through BVH_CULL_LANE and BVH_CULL_GROUP, count-only (d_hits NULL) and count + fill (capacity = the total), timed with HIP events around
--reps calls on the context's stream; a call that takes longer than --budget-s / reps is repeated less often (at least once).  Beside them bvh_overlap,
count-only, with the bounding box of each volume (the box of the frustum's eight corners), and how much larger its set is.  Writes <out>/cull.json and
<out>/cull.md.  None of these numbers is a pass criterion.

    python tools/time_cull.py                      # both meshes
    python tools/time_cull.py --n 2000000          # one uniform mesh
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

SWEEP = (1, 16, 256, 4096, 65536)
PATHS = (("lane", 1), ("group", 2))


def perspective(fovy, aspect, near, far):
    """row-major clip matrix, column-vector convention, camera looking down -z, depth 0 .. 1"""
    f = 1.0 / np.tan(0.5 * fovy)
    m = np.zeros((4, 4))
    m[0, 0] = f / aspect; m[1, 1] = f; m[3, 2] = -1.0
    m[2, 2] = far / (near - far); m[2, 3] = near * far / (near - far)
    return m


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = target - eye; f /= np.linalg.norm(f)
    s = np.cross(f, up)
    if np.linalg.norm(s) < 1e-6:
        s = np.cross(f, (1.0, 0.0, 0.0))
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[:3, 3] = -m[:3, :3] @ eye
    return m


def window_planes(clip, x0, x1, y0, y1):
    """the six planes of the part of a clip matrix's frustum whose normalised device coordinates lie in [x0, x1] x [y0, y1] (depth 0 .. 1): a screen tile"""
    r0, r1, r2, r3 = np.asarray(clip, dtype=np.float64)
    return np.stack([r0 - x0 * r3, x1 * r3 - r0, r1 - y0 * r3, y1 * r3 - r1, r2, r3 - r2]).astype(np.float32)


def window_box(clip, x0, x1, y0, y1):
    """the bounding box (min xyz, max xyz) of the same volume's eight corners"""
    inv = np.linalg.inv(np.asarray(clip, dtype=np.float64))
    c = np.array([[x, y, z, 1.0] for x in (x0, x1) for y in (y0, y1) for z in (0.0, 1.0)]) @ inv.T
    p = c[:, :3] / c[:, 3:4]
    return np.concatenate([p.min(axis=0), p.max(axis=0)]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one uniform mesh of this size instead of the default two")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--budget-s", type=float, default=0.5, help="seconds one round of timed calls may take: longer calls are repeated less often (at least once)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = bvh_pkg.load(); L = pkg.lib()
    torch.cuda.init()
    meshes = [("uniform", a.n)] if a.n else [("sponza", 262_144), ("uniform", 10_000_000)]
    ctx = pkg.Context(0)
    stream = torch.cuda.ExternalStream(L.bvh_ctx_stream(ctx.handle), device=torch.device("cuda", 0))
    rows = []

    def measure(res, planes, boxes):
        """-> dict per path of (total, count_ms, fill_ms, reps), and the overlap count of the bounding boxes"""
        k, per = planes.shape[0], planes.shape[1]
        d_planes, d_boxes, d_off = ctx.upload(planes), ctx.upload(np.ascontiguousarray(boxes)), ctx.alloc((k + 1) * 4)
        out = {"volumes": k}
        total = C.c_uint64()
        for name, path in PATHS:
            t0 = time.perf_counter()
            assert L.bvh_cull(ctx.handle, C.byref(res), d_planes.ptr, k, per, path, d_off.ptr, None, 0, C.byref(total)) == 0   # (warm; the host clock sees its length)
            t0 = time.perf_counter()
            assert L.bvh_cull(ctx.handle, C.byref(res), d_planes.ptr, k, per, path, d_off.ptr, None, 0, C.byref(total)) == 0
            reps = int(min(a.reps, max(1, a.budget_s / max(time.perf_counter() - t0, 1e-6))))
            tot = int(total.value)
            d_hits = ctx.alloc(max(tot, 1) * 8)
            cnt = lambda i: L.bvh_cull(ctx.handle, C.byref(res), d_planes.ptr, k, per, path, d_off.ptr, None, 0, None)
            fill = lambda i: L.bvh_cull(ctx.handle, C.byref(res), d_planes.ptr, k, per, path, d_off.ptr, d_hits.ptr, tot, None)
            assert fill(0) == 0
            c_ms, f_ms = [], []
            for _ in range(2 if reps > 1 else 1):
                c_ms.append(timed(stream, cnt, reps)); f_ms.append(timed(stream, fill, reps))
            out[name] = {"total": tot, "reps": reps, "count_ms": min(c_ms), "fill_ms": min(f_ms), "count_ms_runs": c_ms, "fill_ms_runs": f_ms}
            d_hits.free()
        assert out["lane"]["total"] == out["group"]["total"]
        rc = L.bvh_overlap(ctx.handle, C.byref(res), d_boxes.ptr, k, 0, d_off.ptr, None, 0, C.byref(total))
        assert rc in (0, -10002), rc
        ov = lambda i: L.bvh_overlap(ctx.handle, C.byref(res), d_boxes.ptr, k, 0, d_off.ptr, None, 0, None)
        out["overlap_box"] = {"total": int(total.value), "count_ms": timed(stream, ov, out["lane"]["reps"])}
        out["overlap_over_cull"] = int(total.value) / max(out["lane"]["total"], 1)
        for buf in (d_planes, d_boxes, d_off):
            buf.free()
        return out

    def dump():
        os.makedirs(a.out, exist_ok=True)
        doc = {"_kernel_source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "budget_s": a.budget_s, "rows": rows}
        with open(os.path.join(a.out, "cull.json"), "w") as f:
            json.dump(doc, f, indent=1)
        with open(os.path.join(a.out, "cull.md"), "w") as f:
            f.write(render(doc))

    for kind, n in meshes:
        tris = pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 1)
        v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        del v
        ext = hi - lo; diag = float(np.linalg.norm(ext)); ctr = 0.5 * (lo + hi)
        ctx.reserve(n)
        d_tris = ctx.upload(tris)
        clip = perspective(np.radians(60.0), 16.0 / 9.0, 0.01 * diag, 2.0 * diag) @ look_at(hi + 0.1 * ext, ctr)
        camera = (pkg.frustum_planes(clip)[None], window_box(clip, -1.0, 1.0, -1.0, 1.0)[None])
        tx, ty = 1920 // 16, -(-1080 // 16)
        edges_x = -1.0 + 2.0 * np.arange(tx + 1) * 16.0 / 1920.0; edges_y = np.minimum(-1.0 + 2.0 * np.arange(ty + 1) * 16.0 / 1080.0, 1.0)
        tiles = (np.stack([window_planes(clip, edges_x[i], edges_x[i + 1], edges_y[j], edges_y[j + 1]) for j in range(ty) for i in range(tx)]),
                 np.stack([window_box(clip, edges_x[i], edges_x[i + 1], edges_y[j], edges_y[j + 1]) for j in range(ty) for i in range(tx)]))
        rng = np.random.default_rng(3)
        sp, sb = [], []
        for _ in range(max(SWEEP)):
            eye = lo + rng.random(3) * ext
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            c = perspective(np.radians(rng.uniform(5.0, 20.0)), 1.0, 0.001 * diag, rng.uniform(0.1, 0.3) * diag) @ look_at(eye, eye + d)
            sp.append(pkg.frustum_planes(c)); sb.append(window_box(c, -1.0, 1.0, -1.0, 1.0))
        sweep = (np.stack(sp), np.stack(sb))
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
            row = {"mesh": f"{kind}_{n}", "builder": pkg.ALGO_NAMES[algo], "n": n, "layout": int(b.result.layout)}
            row["camera"] = measure(b.result, *camera)
            row["tiles"] = measure(b.result, *tiles)
            if algo == 3:
                row["sweep"] = [measure(b.result, sweep[0][:k], sweep[1][:k]) for k in SWEEP]
            rows.append(row)
            print(json.dumps(row), flush=True)
            dump()
        d_tris.free()
    ctx.close()
    dump()


def render(doc):
    out = ["# bvh_cull — measured times (MI355X, one device)\n",
           f"`python tools/time_cull.py` (raw rows: `profiles/cull.json`; machine code `{doc['_kernel_source_hash']}`, the `kernel_source_hash` of `bench.py`; device "
           f"{doc['device']}).  camera = one frustum (eye outside a corner of the scene, looking at its centre, 60 degrees, 16:9); tiles = the 120 x 68 frusta of "
           "the 16 x 16-pixel tiles of a 1920 x 1080 view of that camera; sweep = random small frusta (5 to 20 degrees, reaching 10 to 30 % of the scene "
           f"diagonal).  Times are ms per call, the smaller of two rounds of {doc['reps']} calls (fewer, at least one, where a call takes longer than "
           f"{doc['budget_s'] / doc['reps'] * 1e3:.0f} ms) timed with HIP events on the context's stream; lane = `BVH_CULL_LANE` (one volume per lane), group = "
           "`BVH_CULL_GROUP` (one volume per workgroup of 256); count = `d_hits` NULL, fill = count + fill with capacity = the total.  overlap = `bvh_overlap`, "
           "count-only, with each volume's bounding box on the same tree; larger = its total over bvh_cull's.  None of these times is a pass criterion.\n",
           "| mesh | builder (layout) | workload | volumes | records | lane count | lane fill | group count | group fill | lane / group (fill) | overlap count | larger |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]

    def line(r, name, w):
        la, gr = w["lane"], w["group"]
        return (f"| {r['mesh']} | {r['builder']} ({r['layout']}) | {name} | {w['volumes']} | {la['total']} | {la['count_ms']:.3f} | {la['fill_ms']:.3f} | {gr['count_ms']:.3f} | "
                f"{gr['fill_ms']:.3f} | {la['fill_ms'] / gr['fill_ms']:.2f} | {w['overlap_box']['count_ms']:.3f} | {w['overlap_over_cull']:.2f} x |")
    for r in doc["rows"]:
        for name in ("camera", "tiles"):
            if name in r:
                out.append(line(r, name, r[name]))
    out += ["", "The sweep (the crossover between the walks; `BVH_CULL_AUTO` takes the group walk iff n_volumes <= 65 536 and n_leaves >= 1024):\n", out[2], out[3]]
    for r in doc["rows"]:
        for w in r.get("sweep", ()):
            out.append(line(r, "sweep", w))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
