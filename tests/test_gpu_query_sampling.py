"""A refused or empty query call consumes no tick of bvh_ctx_set_kernel_sampling's counter, for each query entry point that has an empty call.  With "every 3": the
first valid call is tick 0 and is sampled; a refused call (null query pointer) and an empty one (n = 0) follow; two more valid calls are then ticks 1 and 2 and
stay unsampled, so bvh_ctx_kernel_times reports what it reported after the first call alone.  Either of the two calls in between consuming a tick, or both,
makes one of the later calls tick 3 — a sampled one — and its kernels show up in the counts."""
import ctypes as C

import numpy as np
import pytest

from test_query import E_INVALID

pytestmark = pytest.mark.gpu

M, K, CAP = 8, 4, 2048            # queries per call, k of the knn calls, records the answer buffer holds (8 queries x 64 triangles x 2 instances = 1024)


@pytest.fixture(scope="module")
def env(pkg):
    """one 64-triangle mesh and its tree on one context, a two-instance scene of it on another, 8 rays / points / boxes on each"""
    tctx, sctx = pkg.Context(0), pkg.Context(0)
    tris = pkg.meshgen.uniform(64, 5)
    assert len(tris) == 64
    b = pkg.BUILDERS[pkg.ALGO_HPLOC]().build(tctx, tris)
    inst = np.zeros(2, dtype=pkg.INSTANCE)
    inst["object_to_world"][:] = np.eye(3, 4, dtype=np.float32).reshape(12)
    inst["object_to_world"][1, 3] = 0.5                   # the second instance: the same mesh, moved along x
    scene = pkg.Scene(sctx).build(pkg.ALGO_TWOPASS, [b], inst)
    cen = ((tris["v1"] + tris["v2"] + tris["v3"]) / np.float32(3.0))[:M].astype(np.float32)
    rays = np.zeros(M, dtype=pkg.RAY)
    rays["origin"], rays["direction"], rays["tmax"] = cen - np.float32([0, 0, 10]), np.float32([0, 0, 1]), np.float32(100.0)
    pts = np.zeros(M, dtype=pkg.POINT_QUERY)
    pts["point"], pts["radius"] = cen, np.float32(0.25)
    boxes = np.zeros(M, dtype=pkg.AABB)
    boxes["min"], boxes["max"] = cen - np.float32(0.1), cen + np.float32(0.1)
    e = {"pkg": pkg, "L": pkg.lib(), "tree": b, "scene": scene, "moments": b.winding_prepare(), "bufs": []}
    for name, c in (("t", tctx), ("s", sctx)):
        e[name] = {"ctx": c, "rays": c.upload(rays), "pts": c.upload(pts), "boxes": c.upload(boxes), "off": c.alloc((M + 1) * 4), "out": c.alloc(CAP * 32),
                   "counts": c.alloc(M * 4)}
        e["bufs"] += [v for k, v in e[name].items() if k != "ctx"]
    e["qtris"] = pkg.BuildInput(pkg.TRI_PADDED64, 30, b.result.d_tris, None, None, 0, 0)      # bvh_intersect_tris' other mesh: the tree's own triangles
    yield e
    for buf in e["bufs"]:
        buf.free()
    scene.close(); sctx.close(); tctx.close()


def entry_points(e):
    """{name: (the side whose context's counter the call ticks, which of its query arrays it takes, call(query pointer, n) -> return code)}"""
    L, t, s, tot = e["L"], e["t"], e["s"], C.c_uint64()
    h, res, sc = t["ctx"].handle, C.byref(e["tree"].result), e["scene"].handle
    return {
        "bvh_intersect": (t, "rays", lambda p, n: L.bvh_intersect(h, res, None, p, n, t["out"].ptr, 0)),
        "bvh_closest_point": (t, "pts", lambda p, n: L.bvh_closest_point(h, res, None, p, n, t["out"].ptr, 0)),
        "bvh_knn": (t, "pts", lambda p, n: L.bvh_knn(h, res, None, p, n, K, t["out"].ptr, t["counts"].ptr)),
        "bvh_winding_number": (t, "pts", lambda p, n: L.bvh_winding_number(h, res, None, e["moments"].ptr, p, n, 2.0, t["out"].ptr)),
        "bvh_overlap": (t, "boxes", lambda p, n: L.bvh_overlap(h, res, p, n, 0, t["off"].ptr, t["out"].ptr, CAP, C.byref(tot))),
        "bvh_intersect_tris": (t, "rays", lambda p, n: L.bvh_intersect_tris(h, res, None, C.byref(e["qtris"]) if p else None, n, 0, t["off"].ptr, t["out"].ptr, CAP,
                                                                    C.byref(tot))),
        "bvh_intersect_all": (t, "rays", lambda p, n: L.bvh_intersect_all(h, res, None, p, n, 1, t["off"].ptr, t["out"].ptr, CAP, C.byref(tot))),
        "bvh_radius_search": (t, "pts", lambda p, n: L.bvh_radius_search(h, res, None, p, n, 1, t["off"].ptr, t["out"].ptr, CAP, C.byref(tot))),
        "bvh_scene_intersect": (s, "rays", lambda p, n: L.bvh_scene_intersect(sc, p, n, s["out"].ptr, 0)),
        "bvh_scene_closest_point": (s, "pts", lambda p, n: L.bvh_scene_closest_point(sc, p, n, s["out"].ptr, 0)),
        "bvh_scene_knn": (s, "pts", lambda p, n: L.bvh_scene_knn(sc, p, n, K, s["out"].ptr, s["counts"].ptr)),
        "bvh_scene_intersect_all": (s, "rays", lambda p, n: L.bvh_scene_intersect_all(sc, p, n, 1, s["off"].ptr, s["out"].ptr, CAP, C.byref(tot))),
        "bvh_scene_radius_search": (s, "pts", lambda p, n: L.bvh_scene_radius_search(sc, p, n, 1, s["off"].ptr, s["out"].ptr, CAP, C.byref(tot))),
        "bvh_scene_overlap": (s, "boxes", lambda p, n: L.bvh_scene_overlap(sc, p, n, 1, s["off"].ptr, s["out"].ptr, CAP, C.byref(tot))),
    }


NAMES = ["bvh_intersect", "bvh_closest_point", "bvh_knn", "bvh_winding_number", "bvh_overlap", "bvh_intersect_tris", "bvh_intersect_all", "bvh_radius_search",
         "bvh_scene_intersect", "bvh_scene_closest_point", "bvh_scene_knn", "bvh_scene_intersect_all", "bvh_scene_radius_search", "bvh_scene_overlap"]


@pytest.mark.parametrize("name", NAMES)
def test_refused_and_empty_calls_consume_no_sampling_tick(env, name):
    side, kind, call = entry_points(env)[name]
    ctx, q = side["ctx"], side[kind].ptr                      # (bvh_intersect_tris: any non-null value stands for its other mesh)
    ctx.set_profiling(2)
    ctx.set_kernel_sampling(3)
    try:
        assert call(q, M) == 0                                # tick 0: sampled
        first = {k: v[1] for k, v in ctx.kernel_times().items()}
        assert first and all(first.values()), f"{name}: the first call after set_kernel_sampling recorded no kernel"
        assert call(None, M) == E_INVALID                     # refused: no tick
        assert call(q, 0) == 0                                # empty: no tick
        assert call(q, M) == 0 and call(q, M) == 0            # ticks 1 and 2 of 3: unsampled
        after = {k: v[1] for k, v in ctx.kernel_times().items()}
        assert after == first, f"{name}: a refused or empty call consumed a sampling tick: {first} -> {after}"
    finally:
        ctx.set_kernel_sampling(1)
        ctx.set_profiling(0)
