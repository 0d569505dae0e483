"""GPU: bvh_split_refs against the numpy restatement and the reference's goldens (byte for byte, every triangle format, light and heavy paths), count-only /
capacity / guard words / errors, bvh_remap_leaves, ray and point queries through split trees against the brute forces, and build parity of the identity case."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_split import (E_INVALID, F32, FLT_MAX, MAX_DEPTH, QUERY_CASES, as_primrefs, golden_cases, golden_mesh, largest_root_area, query_reference, root_boxes,
                        sort_refs, special_cases, split_refs_np)
from test_gpu_query import lbvh_result

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

GUARD = 64                      # bytes in front of and behind every array
PATTERN = 0xCD
E_TOO_LARGE = -10002


class Banded:
    """a device array between two guard bands, pre-filled with a byte pattern"""

    def __init__(self, ctx, nbytes, host=None):
        self.ctx, self.nbytes = ctx, int(nbytes)
        img = np.full(self.nbytes + 2 * GUARD, PATTERN, dtype=np.uint8)
        if host is not None:
            img[GUARD:GUARD + self.nbytes] = np.ascontiguousarray(host).view(np.uint8).ravel()
        self.image = img
        self.buf = ctx.upload(img)
        self.ptr = self.buf.ptr + GUARD

    def read(self):
        return self.buf.download(np.uint8, self.nbytes + 2 * GUARD)

    def payload(self, dtype, count):
        return self.read()[GUARD:GUARD + count * np.dtype(dtype).itemsize].view(dtype).copy()

    def guards_ok(self):
        got = self.read()
        return bool((got[:GUARD] == PATTERN).all() and (got[GUARD + self.nbytes:] == PATTERN).all())

    def untouched(self):
        return bool((self.read() == self.image).all())

    def free(self):
        self.buf.free()


def upload_input(pkg, ctx, tris, fmt):
    """-> (BuildInput, buffers to free)"""
    n = len(tris)
    if fmt == pkg.TRI_PADDED64:
        b = ctx.upload(tris)
        return pkg.BuildInput(fmt, 30, b.ptr, None, None, 0, 0), [b]
    v = np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1).astype("<f4")       # (n, 3, 3)
    if fmt == pkg.TRI_PACKED36:
        b = ctx.upload(np.ascontiguousarray(v.reshape(-1)))
        return pkg.BuildInput(fmt, 30, b.ptr, None, None, 0, 0), [b]
    verts = ctx.upload(np.ascontiguousarray(v.reshape(-1)))
    idx = ctx.upload(np.arange(3 * n, dtype=np.uint32))
    return pkg.BuildInput(fmt, 30, None, verts.ptr, idx.ptr, 3 * n, 0), [verts, idx]


def run_split(pkg, ctx, tris, sa, md, fmt=0, capacity=None, want_total=True):
    """count call, then a fill call with `capacity` (None: the exact total) into banded arrays.  Returns dict(rc, total, offsets, boxes, prims, guards, arrays)"""
    lib = pkg.lib()
    n = len(tris)
    inp, bufs = upload_input(pkg, ctx, tris, fmt)
    off = Banded(ctx, (n + 1) * 4)
    total = C.c_uint64(0)
    rc = lib.bvh_split_refs(ctx.handle, C.byref(inp), n, float(sa), int(md), off.ptr, None, None, 0, C.byref(total))
    assert rc == 0, rc
    counted = int(total.value)
    count_offsets = off.payload(np.uint32, n + 1)
    cap = counted if capacity is None else int(capacity)
    boxes = Banded(ctx, max(cap, 1) * 24); prims = Banded(ctx, max(cap, 1) * 4)
    off2 = Banded(ctx, (n + 1) * 4)
    total2 = C.c_uint64(0)
    rc = lib.bvh_split_refs(ctx.handle, C.byref(inp), n, float(sa), int(md), off2.ptr, boxes.ptr, prims.ptr, cap, C.byref(total2) if want_total else None)
    ctx.synchronize()
    out = {"rc": rc, "counted": counted, "total": int(total2.value), "count_offsets": count_offsets, "offsets": off2.payload(np.uint32, n + 1),
           "boxes": boxes.payload(pkg.AABB, min(cap, counted)), "prims": prims.payload(np.uint32, min(cap, counted)),
           "guards": off.guards_ok() and off2.guards_ok() and boxes.guards_ok() and prims.guards_ok(),
           "outputs_untouched": boxes.untouched() and prims.untouched()}
    for b in bufs + [off.buf, off2.buf, boxes.buf, prims.buf]:
        b.free()
    return out


def all_cases(pkg):
    cases = {}
    for c in golden_cases():
        sa = np.array([c["sa_max_bits"]], dtype=np.uint32).view(F32)[0]
        cases[f"{c['mesh']}_{c['k']}"] = (golden_mesh(pkg, c["mesh"]), sa, MAX_DEPTH, c)
    for name, (tris, sa, md) in special_cases(pkg).items():
        cases[name] = (tris, sa, md, None)
    return cases


CASE_NAMES = [f"{m}_{k}" for m in ("cornell32", "cornell82", "cornell382") for k in (8, 64)] + \
             ["n1", "n2_unsplit", "mesh70", "ulp_grid", "sliver", "depth3", "odd", "odd_deep"]


# ---- 1. the split against the restatement and the goldens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_split_equals_restatement_and_goldens(pkg, ctx, name):
    tris, sa, md, gold = all_cases(pkg)[name]
    offsets, boxes, prims, _ = split_refs_np(tris, sa, md)
    first = None
    for fmt in (pkg.TRI_PADDED64, pkg.TRI_PACKED36, pkg.TRI_INDEXED):
        got = run_split(pkg, ctx, tris, sa, md, fmt)
        assert got["rc"] == 0 and got["guards"]
        assert got["counted"] == got["total"] == int(offsets[-1]), (name, fmt, got["counted"], got["total"], int(offsets[-1]))
        assert got["count_offsets"].tobytes() == offsets.tobytes() == got["offsets"].tobytes(), (name, fmt)
        assert got["prims"].tobytes() == prims.tobytes(), (name, fmt)
        assert got["boxes"].tobytes() == boxes.tobytes(), (name, fmt)
        if first is None:
            first = got
        else:                                                     # the bytes do not depend on the triangle format
            assert got["boxes"].tobytes() == first["boxes"].tobytes() and got["prims"].tobytes() == first["prims"].tobytes()
    if gold is not None:
        want = np.fromfile(os.path.join(GOLDEN, gold["file"]), dtype=pkg.PRIMREF)
        assert sort_refs(as_primrefs(pkg, first["boxes"], first["prims"])).tobytes() == want.tobytes()
    # the Python binding: count, allocate, fill
    o, b, p, total = ctx.split_refs(tris=tris, sa_max=sa, max_depth=md)
    assert total == int(offsets[-1]) and o.tobytes() == offsets.tobytes() and b.tobytes() == boxes.tobytes() and p.tobytes() == prims.tobytes()


def test_same_bytes_on_every_call_and_identity(pkg, ctx, orc):
    tris, sa, md = special_cases(pkg)["mesh70"]
    a = run_split(pkg, ctx, tris, sa, md)
    b = run_split(pkg, ctx, tris, sa, md, want_total=False)       # asynchronous: no read-back
    assert b["rc"] == 0 and b["total"] == 0
    assert a["boxes"].tobytes() == b["boxes"].tobytes() and a["prims"].tobytes() == b["prims"].tobytes() and a["offsets"].tobytes() == b["offsets"].tobytes()
    # identity: max_depth 0, and sa_max = FLT_MAX on finite triangles: the reference's PrimRefs record for record
    tris = golden_mesh(pkg, "cornell382")
    expect = orc.primrefs(tris).tobytes()
    for s, d in ((F32(0.0), 0), (FLT_MAX, MAX_DEPTH)):
        got = run_split(pkg, ctx, tris, s, d)
        assert list(got["offsets"]) == list(range(len(tris) + 1))
        assert as_primrefs(pkg, got["boxes"], got["prims"]).tobytes() == expect


# ---- 2. count only, capacity, guard words, errors -----------------------------------------------------------------------------------------------------------
def test_capacity_too_small_skips_the_fill(pkg, ctx):
    tris, sa, md = special_cases(pkg)["mesh70"]
    offsets, _, _, _ = split_refs_np(tris, sa, md)
    total = int(offsets[-1])
    got = run_split(pkg, ctx, tris, sa, md, capacity=total - 1)
    assert got["rc"] == 0 and got["total"] == total and got["guards"]
    assert got["outputs_untouched"], "a skipped fill wrote into the output arrays"
    assert got["offsets"].tobytes() == offsets.tobytes()
    got = run_split(pkg, ctx, tris, sa, md, capacity=total + 5)   # more room than needed: the slack keeps its pattern
    assert got["rc"] == 0 and got["guards"] and got["total"] == total


def test_errors_write_nothing(pkg, ctx):
    lib = pkg.lib()
    tris, sa, md = special_cases(pkg)["mesh70"]
    n = len(tris)
    inp, bufs = upload_input(pkg, ctx, tris, pkg.TRI_PADDED64)
    off = Banded(ctx, (n + 1) * 4); boxes = Banded(ctx, 4096 * 24); prims = Banded(ctx, 4096 * 4)
    total = C.c_uint64(99)
    bad_fmt = pkg.BuildInput(7, 30, inp.d_tris, None, None, 0, 0)
    no_tris = pkg.BuildInput(pkg.TRI_PADDED64, 30, None, None, None, 0, 0)
    calls = [
        (None, inp, n, 1.0, 16, off.ptr, boxes.ptr, prims.ptr, 4096),
        (ctx.handle, None, n, 1.0, 16, off.ptr, boxes.ptr, prims.ptr, 4096),
        (ctx.handle, inp, n, 1.0, 16, None, boxes.ptr, prims.ptr, 4096),
        (ctx.handle, bad_fmt, n, 1.0, 16, off.ptr, boxes.ptr, prims.ptr, 4096),
        (ctx.handle, no_tris, n, 1.0, 16, off.ptr, boxes.ptr, prims.ptr, 4096),
        (ctx.handle, inp, 0, 1.0, 16, off.ptr, boxes.ptr, prims.ptr, 4096),
        (ctx.handle, inp, 1 << 30, 1.0, 16, off.ptr, None, None, 0),
        (ctx.handle, inp, n, float("nan"), 16, off.ptr, boxes.ptr, prims.ptr, 4096),
        (ctx.handle, inp, n, -1.0, 16, off.ptr, boxes.ptr, prims.ptr, 4096),
        (ctx.handle, inp, n, 1.0, 17, off.ptr, boxes.ptr, prims.ptr, 4096),
        (ctx.handle, inp, n, 1.0, 16, off.ptr, boxes.ptr, None, 4096),            # exactly one output NULL
        (ctx.handle, inp, n, 1.0, 16, off.ptr, None, prims.ptr, 4096),
        (ctx.handle, inp, n, 1.0, 16, off.ptr, boxes.ptr, boxes.ptr + 240, 4096),  # the outputs overlap each other
        (ctx.handle, inp, n, 1.0, 16, prims.ptr + 16, boxes.ptr, prims.ptr, 4096),  # d_offsets inside d_ref_prims
        (ctx.handle, inp, n, 1.0, 16, inp.d_tris + 64, boxes.ptr, prims.ptr, 4096),  # d_offsets inside the input
        (ctx.handle, inp, n, 1.0, 16, off.ptr, inp.d_tris, prims.ptr, 4096),        # d_ref_boxes over the input
    ]
    for k, (h, i, nn, s, d, o, b, p, cap) in enumerate(calls):
        rc = lib.bvh_split_refs(h, C.byref(i) if i is not None else None, nn, s, d, o, b, p, cap, C.byref(total))
        assert rc == E_INVALID, (k, rc)
    ctx.synchronize()
    assert total.value == 99 and off.untouched() and boxes.untouched() and prims.untouched()
    assert bufs[0].download(np.uint8, tris.nbytes).tobytes() == tris.tobytes()
    for b in bufs + [off.buf, boxes.buf, prims.buf]:
        b.free()


# ---- 3. bvh_remap_leaves -----------------------------------------------------------------------------------------------------------------------------------
def leaf_prims(d):
    n = len(d["sorted_vals"])
    return d["nodes"]["left"][n - 1:].copy() if d["layout"] == 0 else d["leaves"]["prim"].copy()


def without_leaf_prims(d):
    n = len(d["sorted_vals"])
    nodes = d["nodes"].copy(); leaves = None if d["leaves"] is None else d["leaves"].copy()
    if d["layout"] == 0:
        nodes["left"][n - 1:] = 0
    else:
        leaves["prim"] = 0
    return nodes.tobytes() + (b"" if leaves is None else leaves.tobytes())


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_remap_leaves(pkg, ctx, algo):
    lib = pkg.lib()
    tris = golden_mesh(pkg, "cornell382")
    sa = F32(largest_root_area(tris) * F32(1.0 / 64))
    d_off, d_boxes, d_prims, total = ctx.split_refs(tris=tris, sa_max=sa, keep_on_device=True)
    ref_prims = d_prims.download(np.uint32, total)
    try:
        b = pkg.BUILDERS[algo]().build_boxes(ctx, d_boxes, n=total)
        before = b.download()
        assert sorted(leaf_prims(before)) == list(range(total))
        # errors change nothing
        assert lib.bvh_remap_leaves(ctx.handle, C.byref(b.result), None, total) == E_INVALID
        assert lib.bvh_remap_leaves(ctx.handle, None, d_prims.ptr, total) == E_INVALID
        written = (b.result.d_nodes + (total - 1) * 32) if b.result.layout == 0 else b.result.d_leaves
        assert lib.bvh_remap_leaves(ctx.handle, C.byref(b.result), written + 8, total) == E_INVALID       # the map inside the leaf records
        bad = pkg.Result.from_buffer_copy(b.result); bad.root = total
        assert lib.bvh_remap_leaves(ctx.handle, C.byref(bad), d_prims.ptr, total) == E_INVALID
        same = b.download()
        assert same["nodes"].tobytes() == before["nodes"].tobytes() and (same["leaves"] is None or same["leaves"].tobytes() == before["leaves"].tobytes())
        # a short map: q >= n_map is left as it is
        half = total // 2
        b.remap_leaves(d_prims, n_map=half)
        mid = b.download()
        q = leaf_prims(before)
        assert np.array_equal(leaf_prims(mid), np.where(q < half, ref_prims[np.minimum(q, half - 1)], q))
        assert without_leaf_prims(mid) == without_leaf_prims(before)
        # rebuild (same boxes: same tree), then the whole map
        b = pkg.BUILDERS[algo]().build_boxes(ctx, d_boxes, n=total)
        again = b.download()
        assert again["nodes"].tobytes() == before["nodes"].tobytes()
        b.remap_leaves(d_prims, n_map=total)
        after = b.download()
        assert np.array_equal(leaf_prims(after), ref_prims[q])
        assert without_leaf_prims(after) == without_leaf_prims(before)
        assert after["root"] == before["root"] and after["sorted_vals"].tobytes() == before["sorted_vals"].tobytes()
        assert leaf_prims(after).max() < len(tris)
    finally:
        for bfr in (d_off, d_boxes, d_prims):
            bfr.free()


@pytest.mark.parametrize("algo", [0, 3])
def test_remap_drops_the_cached_leaf_map(pkg, algo):
    """through bvh_refit_subset's public behaviour: on the ctx's own tree its leaf map is cached; after a relabelling by a permutation a stale map would send a
    moved triangle's box to the leaf that USED to carry its index"""
    c = pkg.Context(0)
    try:
        tris = pkg.meshgen.uniform(300, 4)
        n = len(tris)
        d_tris = c.upload(tris)
        d_off, d_boxes, d_prims, total = c.split_refs(tris=d_tris, n=n, sa_max=0.0, max_depth=0, keep_on_device=True)
        assert total == n
        b = pkg.BUILDERS[algo]().build_boxes(c, d_boxes, n=n)
        b.refit_subset(np.array([5], dtype=np.uint32), tris=d_tris)               # makes and caches the leaf map (nothing moved: same boxes)
        before = b.download()
        perm = np.arange(n, dtype=np.uint32)[::-1].copy()
        b.remap_leaves(perm)
        moved = tris.copy()
        for f in ("v1", "v2", "v3"):
            moved[f][7] += np.float32(0.25)
        d_tris.upload(moved)
        b.refit_subset(np.array([7], dtype=np.uint32), tris=d_tris)
        after = b.download()
        labels = leaf_prims(after)
        assert np.array_equal(labels, perm[leaf_prims(before)])
        j = int(np.nonzero(labels == 7)[0][0])                    # the leaf that carries index 7 NOW
        lo, hi = root_boxes(moved[7:8])
        rec = after["nodes"][n - 1 + j] if after["layout"] == 0 else after["leaves"][j]
        old = before["nodes"][n - 1 + j] if before["layout"] == 0 else before["leaves"][j]
        assert np.array_equal(rec["min"], lo[0]) and np.array_equal(rec["max"], hi[0])
        assert not np.array_equal(old["min"], lo[0])
        stale = int(np.nonzero(leaf_prims(before) == 7)[0][0])    # the leaf a stale map would have written
        rec_s = after["nodes"][n - 1 + stale] if after["layout"] == 0 else after["leaves"][stale]
        old_s = before["nodes"][n - 1 + stale] if before["layout"] == 0 else before["leaves"][stale]
        assert stale != j and rec_s["min"].tobytes() == old_s["min"].tobytes() and rec_s["max"].tobytes() == old_s["max"].tobytes()
        for bfr in (d_tris, d_off, d_boxes, d_prims):
            bfr.free()
    finally:
        c.close()


# ---- 4. queries through split trees --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def raw_intersect(pkg, ctx, result, inp, rays, kind):
    d_rays = ctx.upload(rays); hits = ctx.alloc(len(rays) * 16)
    try:
        assert pkg.lib().bvh_intersect(ctx.handle, C.byref(result), C.byref(inp), d_rays.ptr, len(rays), hits.ptr, kind) == 0
        return hits.download(pkg.HIT, len(rays))
    finally:
        d_rays.free(); hits.free()


def raw_closest_point(pkg, ctx, result, inp, pts, kind):
    d_pts = ctx.upload(pts); hits = ctx.alloc(len(pts) * 32)
    try:
        assert pkg.lib().bvh_closest_point(ctx.handle, C.byref(result), C.byref(inp), d_pts.ptr, len(pts), hits.ptr, kind) == 0
        return hits.download(pkg.POINT_HIT, len(pts))
    finally:
        d_pts.free(); hits.free()


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
@pytest.mark.parametrize("name", list(QUERY_CASES))
def test_queries_through_split_trees(pkg, ctx, scene_ctx, name, algo):
    q = query_reference(pkg, name)
    tris, rays, pts = q["tris"], q["rays"], q["points"]
    rw, pw = q["ray_well"], q["point_well"]
    assert rw.mean() >= 0.99 and pw.mean() >= 0.99
    ref, pref = q["bf"]["closest"], q["pbf"]["closest"]
    # the unsplit tree's answers
    u = pkg.BUILDERS[algo]().build(ctx, tris)
    unsplit = u.intersect(rays, "closest")
    unsplit_pts = u.closest_point(pts, query="closest")
    # the split tree (the build above is gone: the same arena)
    b = pkg.BUILDERS[algo]().build_split(ctx, tris, q["sa_max"])
    off, boxes, prims = b.split_arrays()
    assert off.tobytes() == q["offsets"].tobytes() and boxes.tobytes() == q["boxes"].tobytes() and prims.tobytes() == q["prims"].tobytes()
    assert b.result.n_leaves == len(prims) > len(tris)
    inp = pkg.BuildInput(pkg.TRI_PADDED64, 30, b._split["tris"].ptr, None, None, 0, 0)
    keep = []
    results = [("as built", b.result)]
    if b.result.layout == 1:
        results.append(("lbvh layout", lbvh_result(pkg, ctx, b, keep)))           # the relabelled tree in the other layout
    for label, res in results:
        what = f"{name} algo {algo} {label}"
        c = raw_intersect(pkg, ctx, res, inp, rays, pkg.QUERY_CLOSEST)
        a = raw_intersect(pkg, ctx, res, inp, rays, pkg.QUERY_ANY)
        assert c[rw].tobytes() == ref[rw].tobytes(), f"{what}: closest differs from the brute force on {np.count_nonzero((c != ref) & rw)} split-well-conditioned rays"
        assert c[rw].tobytes() == unsplit[rw].tobytes(), f"{what}: closest differs from the unsplit tree's"
        assert ((a["prim"] != pkg.INVALID) == q["bf"]["hit"])[rw].all(), f"{what}: any-hit hit/miss differs"
        assert (a["prim"][a["prim"] != pkg.INVALID] < len(tris)).all()
        cp = raw_closest_point(pkg, ctx, res, inp, pts, pkg.QUERY_CLOSEST)
        ap = raw_closest_point(pkg, ctx, res, inp, pts, pkg.QUERY_ANY)
        assert cp[pw].tobytes() == pref[pw].tobytes(), f"{what}: closest point differs from the brute force on {np.count_nonzero((cp != pref) & pw)} queries"
        assert cp[pw].tobytes() == unsplit_pts[pw].tobytes(), f"{what}: closest point differs from the unsplit tree's"
        assert ((ap["prim"] != pkg.INVALID) == q["pbf"]["hit"])[pw].all(), f"{what}: any-hit hit/miss differs (points)"
    # the binding passes the kept triangles by default
    mine = b.intersect(rays, "closest")
    assert mine[rw].tobytes() == ref[rw].tobytes()
    assert b.closest_point(pts, query="closest")[pw].tobytes() == pref[pw].tobytes()
    # as the single identity-instance BLAS of a scene (on another ctx: a BLAS may not live in the scene's arena)
    inst = np.zeros(1, dtype=pkg.INSTANCE)
    inst["object_to_world"][0] = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    ctx.synchronize()
    sc = pkg.Scene(scene_ctx).build(algo, [(b, inp)], inst)
    sh = sc.intersect(rays, "closest")
    for f in ("t", "u", "v", "prim"):
        assert np.array_equal(sh[f][rw].view(np.uint32), mine[f][rw].view(np.uint32)), f"{name} algo {algo}: the scene's {f} differs"
    assert (sh["instance"][rw & (mine["prim"] != pkg.INVALID)] == 0).all()
    sc.close()
    for k in keep:
        k.free()
    b._free_split()


# ---- 5. build parity ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_identity_refs_build_the_same_tree(pkg, ctx, algo):
    """bvh_build_boxes over the max_depth = 0 output is byte-identical to bvh_build_ex on the triangles: pins the root-box rule"""
    for tris in (golden_mesh(pkg, "cornell382"), pkg.meshgen.uniform(1000, 6), pkg.meshgen.sponza_like(1000, 3)):
        n = len(tris)
        d_tris = ctx.upload(tris)
        want = pkg.BUILDERS[algo]().build_ex(ctx, n, tris=d_tris).download()
        d_off, d_boxes, d_prims, total = ctx.split_refs(tris=d_tris, n=n, sa_max=0.0, max_depth=0, keep_on_device=True)
        assert total == n and np.array_equal(d_prims.download(np.uint32, n), np.arange(n, dtype=np.uint32))
        got = pkg.BUILDERS[algo]().build_boxes(ctx, d_boxes, n=n).download()
        assert got["root"] == want["root"] and got["nodes"].tobytes() == want["nodes"].tobytes()
        assert (got["leaves"] is None) == (want["leaves"] is None) and (got["leaves"] is None or got["leaves"].tobytes() == want["leaves"].tobytes())
        assert got["sorted_keys"].tobytes() == want["sorted_keys"].tobytes() and got["sorted_vals"].tobytes() == want["sorted_vals"].tobytes()
        assert got["scene"].tobytes() == want["scene"].tobytes()
        for bfr in (d_tris, d_off, d_boxes, d_prims):
            bfr.free()
