"""GPU: bvh_refit_subset (new boxes for the listed primitives' leaves and their paths to the root only) on all four builders' trees: equal to a full
refit when nothing else moved, equal to the numpy restatement, and nothing off the dirty paths is written."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_refit import jitter, mesh, stage_e
from test_refit_subset import dirty_path_mask, reference_refit_subset

pytestmark = pytest.mark.gpu

ALGOS = [0, 1, 2, 3]
E_INVALID = -10001
GUARD = 256                    # guard bytes in front of and behind every caller-owned array
GUARD_BYTE = 0xA5


def move_subset(a, prims, seed, scale=1e-3):
    """mesh a with only the listed triangles jittered"""
    b = a.copy()
    p = np.unique(np.asarray(prims, dtype=np.int64)); p = p[p < len(a)]
    b[p] = jitter(a, seed, scale)[p]
    return b


def dl(pkg, ctx, ptr, dtype, count):
    out = np.empty(count, dtype=dtype)
    assert pkg.lib().bvh_dev_download(ctx.handle, out.ctypes.data, ptr, out.nbytes) == 0
    return out


def snap(pkg, ctx, r):
    """every array of result r that a refit may write, and those it may not"""
    n = r.n_leaves
    out = {"nodes": dl(pkg, ctx, r.d_nodes, pkg.BVH2_NODE, 2 * n - 1 if r.layout == 0 else n - 1),
           "leaves": dl(pkg, ctx, r.d_leaves, pkg.PRIMREF, n) if r.layout == 1 else None,
           "boxes": dl(pkg, ctx, r.d_prim_aabbs, pkg.AABB, n), "scene": dl(pkg, ctx, r.d_scene_extent, pkg.AABB, 1),
           "root": r.root, "layout": r.layout}
    if r.d_sorted_vals:
        out["svals"] = dl(pkg, ctx, r.d_sorted_vals, np.uint32, n)
        out["skeys"] = dl(pkg, ctx, r.d_sorted_keys, np.uint64 if r.key_bits == 64 else np.uint32, n)
    return out


def same_bytes(x, y, what=""):
    for f in ("nodes", "leaves", "boxes", "scene"):
        if x[f] is None:
            assert y[f] is None
        else:
            assert x[f].tobytes() == y[f].tobytes(), f"{what}: {f} differ"


def untouched(after, before, what=""):
    """links, prims, root and the sorted arrays"""
    assert after["root"] == before["root"]
    n = len(after["boxes"])
    assert np.array_equal(after["nodes"]["left"], before["nodes"]["left"]) and np.array_equal(after["nodes"]["right"], before["nodes"]["right"]), what
    if after["leaves"] is not None:
        assert np.array_equal(after["leaves"]["prim"], before["leaves"]["prim"]), what
    assert np.array_equal(after["svals"], before["svals"]) and np.array_equal(after["skeys"], before["skeys"]), what
    assert n == len(before["boxes"])


def expected(pkg, ctx, before, b_mesh, prims):
    n = len(b_mesh)
    eb, _ = stage_e(pkg, ctx, b_mesh)
    ref_n, ref_l, ref_b, scene = reference_refit_subset(before["nodes"], before["leaves"], before["root"], n, before["layout"], before["boxes"], eb, prims)
    sc = np.zeros(1, dtype=pkg.AABB); sc["min"][0] = scene[0]; sc["max"][0] = scene[1]
    return {"nodes": ref_n, "leaves": ref_l, "boxes": ref_b, "scene": sc}


def sibling_pair(s):
    """the two primitives of some internal node whose children are both leaves"""
    n = len(s["boxes"]); ni = n - 1
    le, ri = s["nodes"]["left"][:ni].astype(np.int64), s["nodes"]["right"][:ni].astype(np.int64)
    k = int(np.nonzero((le >= ni) & (ri >= ni))[0][0])
    if s["layout"] == 0:
        return np.array([s["nodes"]["left"][le[k]], s["nodes"]["left"][ri[k]]], dtype=np.uint32)
    return np.array([s["leaves"]["prim"][le[k] - ni], s["leaves"]["prim"][ri[k] - ni]], dtype=np.uint32)


def choices(s, n, seed):
    rng = np.random.default_rng(seed)
    run = max(2, n // 8)
    start = int(rng.integers(0, n - run + 1))
    return {"one": np.array([rng.integers(0, n)], dtype=np.uint32),
            "all": np.arange(n, dtype=np.uint32),
            "random": rng.choice(n, max(1, n // 100), replace=False).astype(np.uint32),
            "run": s["svals"][start:start + run].copy(),
            "siblings": sibling_pair(s)}


@pytest.fixture(scope="module")
def ctx2(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def run_subset(pkg, ctx, algo, a, b_mesh, prims):
    """build a on ctx, refit_subset(prims) with b_mesh: (builder, before, after)"""
    n = len(a)
    d_b = ctx.upload(b_mesh)
    bld = pkg.BUILDERS[algo]().build(ctx, a)
    before = snap(pkg, ctx, bld.result)
    bld.refit_subset(np.asarray(prims, dtype=np.uint32), tris=d_b)
    assert bld.result.d_tris == d_b.ptr
    after = snap(pkg, ctx, bld.result)
    d_b.free()
    assert n == len(after["boxes"])
    return bld, before, after


# ---- equality with the full refit and with the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", ["uniform_2", "uniform_3", "uniform_511", "uniform_512", "uniform_513", "uniform_1025", "uniform_20000"])
def test_subset_equals_full_refit(pkg, ctx, ctx2, name, algo):
    a = mesh(pkg, name); n = len(a)
    s0 = snap(pkg, ctx, pkg.BUILDERS[algo]().build(ctx, a).result)
    for what, prims in choices(s0, n, 17 * n + algo).items():
        b_mesh = move_subset(a, prims, 3 + algo)
        _, before, after = run_subset(pkg, ctx, algo, a, b_mesh, prims)
        full = pkg.BUILDERS[algo]().build(ctx2, a).refit(b_mesh)
        same_bytes(after, snap(pkg, ctx2, full.result), f"{what} vs full refit")
        same_bytes(after, expected(pkg, ctx, before, b_mesh, prims), f"{what} vs restatement")
        untouched(after, before, what)


@pytest.mark.parametrize("algo", [1, 3])                          # once per layout
def test_subset_equals_full_refit_sponza(pkg, ctx, ctx2, algo):
    a = mesh(pkg, "sponza_262144"); n = len(a)
    s0 = snap(pkg, ctx, pkg.BUILDERS[algo]().build(ctx, a).result)
    ch = choices(s0, n, 5)
    for what in ("random", "run"):
        prims = ch[what]
        b_mesh = move_subset(a, prims, 8)
        _, before, after = run_subset(pkg, ctx, algo, a, b_mesh, prims)
        full = pkg.BUILDERS[algo]().build(ctx2, a).refit(b_mesh)
        same_bytes(after, snap(pkg, ctx2, full.result), f"{what} vs full refit")
        same_bytes(after, expected(pkg, ctx, before, b_mesh, prims), f"{what} vs restatement")
        untouched(after, before, what)


# ---- caller-owned arrays between guard words ----------------------------------------------------------------------------------------------------------------
class Owned:
    """guarded caller-owned copies of a tree's arrays (host arrays given), as a bvh_result"""

    def __init__(self, pkg, ctx, r, arrays):
        self.pkg, self.ctx, self.bufs, self.sizes = pkg, ctx, {}, {}
        self.result = pkg.Result.from_buffer_copy(r)
        for f, host in arrays.items():
            if host is None:
                continue
            raw = np.full(host.nbytes + 2 * GUARD, GUARD_BYTE, dtype=np.uint8)
            raw[GUARD:GUARD + host.nbytes] = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
            self.bufs[f] = ctx.upload(raw); self.sizes[f] = host.nbytes
            setattr(self.result, f, self.bufs[f].ptr + GUARD)
        self.result.d_sorted_keys = None; self.result.d_sorted_vals = None

    def guards_intact(self):
        for f, buf in self.bufs.items():
            raw = buf.download(np.uint8, self.sizes[f] + 2 * GUARD)
            if not ((raw[:GUARD] == GUARD_BYTE).all() and (raw[GUARD + self.sizes[f]:] == GUARD_BYTE).all()):
                return False
        return True

    def free(self):
        for buf in self.bufs.values():
            buf.free()


def owned_copy(pkg, ctx, r, s, nodes=None, leaves=None):
    return Owned(pkg, ctx, r, {"d_nodes": s["nodes"] if nodes is None else nodes, "d_leaves": s["leaves"] if leaves is None else leaves,
                               "d_prim_aabbs": s["boxes"], "d_scene_extent": s["scene"]})


@pytest.mark.parametrize("algo", [1, 3])
def test_only_the_paths_are_written(pkg, algo):
    """every box off the dirty paths is junk (min 7, max -7) before the call and the same junk after it; a box on a path is the union of its children's
    current boxes, junk included: a full refit in disguise fails here"""
    a = mesh(pkg, "uniform_20000"); n = len(a); ni = n - 1
    c = pkg.Context(0)
    try:
        bld = pkg.BUILDERS[algo]().build(c, a)
        s = snap(pkg, c, bld.result)
        layout = s["layout"]
        prims = np.random.default_rng(31).choice(n, 64, replace=False).astype(np.uint32)
        on_path, leaf_dirty = dirty_path_mask(s["nodes"], s["leaves"], s["root"], n, layout, prims)
        assert 64 < on_path.sum() < ni // 4
        junk_n = s["nodes"].copy(); junk_l = None if s["leaves"] is None else s["leaves"].copy()
        junk_n["min"][:ni][~on_path] = 7.0; junk_n["max"][:ni][~on_path] = -7.0
        if layout == 0:
            junk_n["min"][ni:][~leaf_dirty] = 7.0; junk_n["max"][ni:][~leaf_dirty] = -7.0
        else:
            junk_l["min"][~leaf_dirty] = 7.0; junk_l["max"][~leaf_dirty] = -7.0
        own = owned_copy(pkg, c, bld.result, s, junk_n, junk_l)
        b_mesh = move_subset(a, prims, 4, 0.05)
        d_b, d_p = c.upload(b_mesh), c.upload(prims)
        inp = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_b.ptr, None, None, 0, 0)
        for _ in range(2):                                            # (a second call makes its plan and map again, from the same arrays)
            assert pkg.lib().bvh_refit_subset(c.handle, C.byref(own.result), C.byref(inp), d_p.ptr, len(prims), None) == 0
        got = snap(pkg, c, own.result)
        assert own.guards_intact()
        keep = np.concatenate([~on_path, ~leaf_dirty]) if layout == 0 else ~on_path
        assert got["nodes"][keep].tobytes() == junk_n[keep].tobytes(), "a node off the dirty paths was written"
        if layout == 1:
            assert got["leaves"][~leaf_dirty].tobytes() == junk_l[~leaf_dirty].tobytes(), "a leaf off the dirty paths was written"
        eb, _ = stage_e(pkg, c, b_mesh)
        listed = np.zeros(n, dtype=bool); listed[prims] = True
        assert got["boxes"][~listed].tobytes() == s["boxes"][~listed].tobytes() and got["boxes"][listed].tobytes() == eb[listed].tobytes()
        lo = got["nodes"]["min"] if layout == 0 else np.concatenate([got["nodes"]["min"], got["leaves"]["min"]])
        hi = got["nodes"]["max"] if layout == 0 else np.concatenate([got["nodes"]["max"], got["leaves"]["max"]])
        leaf_prim = (got["nodes"]["left"][ni:] if layout == 0 else got["leaves"]["prim"]).astype(np.int64)
        dj = np.nonzero(leaf_dirty)[0]
        assert lo[ni + dj].tobytes() == eb["min"][leaf_prim[dj]].tobytes() and hi[ni + dj].tobytes() == eb["max"][leaf_prim[dj]].tobytes()
        p = np.nonzero(on_path)[0]
        le, ri = got["nodes"]["left"][p].astype(np.int64), got["nodes"]["right"][p].astype(np.int64)
        assert np.array_equal(lo[p], np.fmin(lo[le], lo[ri])) and np.array_equal(hi[p], np.fmax(hi[le], hi[ri]))
        assert np.array_equal(got["scene"]["min"][0], lo[s["root"]]) and np.array_equal(got["scene"]["max"][0], hi[s["root"]])
        same_bytes(got, expected(pkg, c, {**s, "nodes": junk_n, "leaves": junk_l}, b_mesh, prims), "junk tree vs restatement")
        assert bld.checksum() == pkg.checksum_host(s["nodes"], s["leaves"], s["root"]), "the ctx's own arrays were touched"
        for d in (d_b, d_p):
            d.free()
        own.free()
    finally:
        c.close()


@pytest.mark.parametrize("algo", [0, 2])
def test_duplicates_and_bad_indices(pkg, algo):
    a = mesh(pkg, "uniform_20000"); n = len(a)
    rng = np.random.default_rng(41)
    prims = rng.choice(n, 200, replace=False).astype(np.uint32)
    bad = np.array([n, n + 5, 0xFFFFFFFF], dtype=np.uint32)
    lists = {"clean": prims,
             "tripled": rng.permutation(np.concatenate([prims, prims, prims, bad, bad])).astype(np.uint32),
             "repeated": rng.permutation(np.concatenate([prims, np.full(4096, prims[7], dtype=np.uint32), bad])).astype(np.uint32),
             "one_4096_times": None}
    b_mesh = move_subset(a, prims, 6, 0.02)
    c = pkg.Context(0)
    try:
        bld = pkg.BUILDERS[algo]().build(c, a)
        s = snap(pkg, c, bld.result)
        d_b = c.upload(b_mesh)
        inp = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_b.ptr, None, None, 0, 0)
        results = {}
        for what, lst in lists.items():
            if lst is None:
                lst = np.full(4096, prims[3], dtype=np.uint32)
            own = owned_copy(pkg, c, bld.result, s)
            d_p = c.upload(lst)
            assert pkg.lib().bvh_refit_subset(c.handle, C.byref(own.result), C.byref(inp), d_p.ptr, len(lst), None) == 0
            results[what] = snap(pkg, c, own.result)
            assert own.guards_intact(), what
            d_p.free(); own.free()
        same_bytes(results["tripled"], results["clean"], "tripled"); same_bytes(results["repeated"], results["clean"], "repeated")
        same_bytes(results["clean"], expected(pkg, c, s, b_mesh, prims), "clean vs restatement")
        same_bytes(results["one_4096_times"], expected(pkg, c, s, b_mesh, prims[3:4]), "one index 4096 times vs restatement")
        # the ctx's own tree, the same lists back to back: the owner / pending words are clean after each
        for what in ("tripled", "repeated", "clean"):
            bld = pkg.BUILDERS[algo]().build(c, a)
            bld.refit_subset(lists[what], tris=d_b)
            same_bytes(snap(pkg, c, bld.result), results["clean"], f"own tree, {what}")
        d_b.free()
    finally:
        c.close()


@pytest.mark.parametrize("algo", [1, 3])
def test_marks_of_malformed_arrays_do_not_reach_the_next_call(pkg, ctx2, algo):
    """caller-owned arrays in which two internal nodes name each other as child: the mark walker of a leaf below them stops on its own mark and the climb
    walker stops there too, so marks stay behind.  The call ends, in bounds, with unspecified boxes — and the next call, on the ctx's own valid tree, is a
    correct subset refit: it equals the full refit."""
    a = mesh(pkg, "uniform_20000"); n = len(a); ni = n - 1
    c = pkg.Context(0)
    try:
        bld = pkg.BUILDERS[algo]().build(c, a)
        s = snap(pkg, c, bld.result)
        le, ri = s["nodes"]["left"][:ni].astype(np.int64), s["nodes"]["right"][:ni].astype(np.int64)
        par = np.full(2 * n - 1, -1, dtype=np.int64); par[le] = np.arange(ni); par[ri] = np.arange(ni)
        inner = np.arange(ni)
        ok = ((le >= ni) | (ri >= ni)) & (par[inner] >= 0)
        ok[ok] &= par[par[inner[ok]]] >= 0
        x = int(np.nonzero(ok)[0][0]); y = int(par[x]); g = int(par[y])               # x has a leaf child, y is x's parent, g is y's
        leaf_side = "left" if le[x] >= ni else "right"
        other_side = "right" if leaf_side == "left" else "left"
        leaf, orphan = int(s["nodes"][leaf_side][x]), s["nodes"][other_side][x]
        bad = s["nodes"].copy()
        bad[other_side][x] = y                                        # x names y, y names x ...
        bad["left" if le[g] == y else "right"][g] = orphan            # ... and nobody else names either
        p = s["nodes"]["left"][leaf] if s["layout"] == 0 else s["leaves"]["prim"][leaf - ni]
        b_mesh = jitter(a, 12)
        d_b = c.upload(b_mesh)
        own = owned_copy(pkg, c, bld.result, s, nodes=bad)
        d_p = c.upload(np.array([p], dtype=np.uint32))
        inp = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_b.ptr, None, None, 0, 0)
        assert pkg.lib().bvh_refit_subset(c.handle, C.byref(own.result), C.byref(inp), d_p.ptr, 1, None) == 0
        c.synchronize()
        assert own.guards_intact()
        assert bld.checksum() == pkg.checksum_host(s["nodes"], s["leaves"], s["root"]), "the ctx's own arrays were touched"
        d_p.free(); own.free()
        bld.refit_subset(np.arange(n, dtype=np.uint32), tris=d_b)     # every node of the ctx's own tree is on a path, the two above included
        full = pkg.BUILDERS[algo]().build(ctx2, a).refit(b_mesh)
        same_bytes(snap(pkg, c, bld.result), snap(pkg, ctx2, full.result), "own tree after a call on malformed arrays vs full refit")
        d_b.free()
    finally:
        c.close()


# ---- input formats ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [1, 3])
def test_subset_input_formats_agree(pkg, ctx, algo):
    a = mesh(pkg, "uniform_20000"); n = len(a)
    prims = np.random.default_rng(51).choice(n, 300, replace=False).astype(np.uint32)
    bm = move_subset(a, prims, 7, 0.01)
    bm["v1"][prims[0]] = np.nan; bm["v2"][prims[1]][1] = np.inf; bm["v3"][prims[2]][2] = -np.inf          # stage E's clamp, in every format
    for f in ("v1", "v2", "v3"):
        v = bm[f]; v[prims[3]] = np.nan; bm[f] = v
    v = np.stack([bm["v1"], bm["v2"], bm["v3"]], axis=1).astype(np.float32)
    d_pad = ctx.upload(bm); d_packed = ctx.upload(np.ascontiguousarray(v.reshape(n, 9)))
    d_verts = ctx.upload(np.ascontiguousarray(v.reshape(3 * n, 3))); d_idx = ctx.upload(np.arange(3 * n, dtype=np.uint32))
    results = []
    for fmt in ("padded", "packed", "indexed"):
        b = pkg.BUILDERS[algo]().build(ctx, a)
        if fmt == "padded":
            b.refit_subset(prims, tris=d_pad)
        elif fmt == "packed":
            b.refit_subset(prims, tris=d_packed, tri_format=pkg.TRI_PACKED36)
        else:
            b.refit_subset(prims, vertices=d_verts, indices=d_idx, n_vertices=3 * n, tri_format=pkg.TRI_INDEXED)
            assert b.result.d_tris == d_verts.ptr
        results.append(snap(pkg, ctx, b.result))
    eb, _ = stage_e(pkg, ctx, bm)
    assert results[0]["boxes"][prims].view(np.uint32).tobytes() == eb[prims].view(np.uint32).tobytes()
    for r in results[1:]:
        for f in ("nodes", "leaves", "boxes", "scene"):
            assert (r[f] is None and results[0][f] is None) or r[f].view(np.uint8).tobytes() == results[0][f].view(np.uint8).tobytes(), f
    # in == NULL: the tree's own d_tris
    b = pkg.BUILDERS[algo]().build(ctx, d_pad, on_device=True, n=n)
    b.refit_subset(prims)
    assert b.result.d_tris == d_pad.ptr
    for d in (d_pad, d_packed, d_verts, d_idx):
        d.free()


# ---- after bvh_optimize; kernel names; the cached plan and map -------------------------------------------------------------------------------------------------
def profiled_subset(pkg, c, bld, inp, d_p, m):
    c.set_profiling(2)
    assert pkg.lib().bvh_refit_subset(c.handle, C.byref(bld.result), C.byref(inp), d_p.ptr, m, C.byref(bld.timings)) == 0
    kt = c.kernel_times()
    tm = (bld.timings.ms_extents, bld.timings.ms_build, bld.timings.ms_total, bld.timings.sampled)
    c.set_profiling(0)
    return kt, tm


@pytest.mark.parametrize("algo", [1, 3])
@pytest.mark.parametrize("optimised", [False, True])
def test_kernel_names_and_cached_plan(pkg, algo, optimised):
    a = mesh(pkg, "uniform_20000"); n = len(a)
    prims = np.random.default_rng(61).choice(n, 500, replace=False).astype(np.uint32)
    b1, b2 = move_subset(a, prims, 1, 0.01), move_subset(a, prims, 2, 0.01)
    c = pkg.Context(0)
    try:
        bld = pkg.BUILDERS[algo]().build(c, a)
        if optimised:
            bld.optimize(3)
        d_1, d_2, d_p = c.upload(b1), c.upload(b2), c.upload(prims)         # (uploads through the ctx end the cached plan: all of them before the calls)
        before = snap(pkg, c, bld.result)
        kt1, tm1 = profiled_subset(pkg, c, bld, pkg.BuildInput(pkg.TRI_PADDED64, 30, d_1.ptr, None, None, 0, 0), d_p, len(prims))
        kt2, tm2 = profiled_subset(pkg, c, bld, pkg.BuildInput(pkg.TRI_PADDED64, 30, d_2.ptr, None, None, 0, 0), d_p, len(prims))
        subset = {"k_refit_subset_boxes", "k_refit_subset_mark", "k_refit_subset_climb"}
        assert set(kt1) == subset | {"k_refit_plan", "k_refit_leafmap"}, kt1
        assert set(kt2) == subset, kt2
        for kt in (kt1, kt2):
            assert "k_refit_climb" not in kt and not any(k.startswith("k_extents") for k in kt)
        for tm in (tm1, tm2):
            assert tm[3] == 1 and tm[0] > 0 and tm[1] > 0 and abs(tm[2] - (tm[0] + tm[1])) <= 1e-6 * tm[2]
        after = snap(pkg, c, bld.result)
        same_bytes(after, expected(pkg, c, before, b2, prims), "second call vs restatement")      # (b1 and b2 move the same triangles)
        bld.refit(d_2, on_device=True, n=n)                           # the full refit of the same (optimised) tree
        same_bytes(after, snap(pkg, c, bld.result), "subset vs full refit of the same tree")
        for d in (d_1, d_2, d_p):
            d.free()
    finally:
        c.close()


# ---- the words are clean afterwards ----------------------------------------------------------------------------------------------------------------------------
def make_rays(pkg, tris, m, seed):
    rng = np.random.default_rng(seed)
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    o = lo - 0.5 * ext + rng.random((m, 3)) * 2.0 * ext
    d = lo + rng.random((m, 3)) * ext - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros(m, dtype=pkg.RAY)
    r["origin"] = o.astype(np.float32); r["direction"] = d.astype(np.float32); r["tmin"] = 0.0; r["tmax"] = np.float32(3.0e38)
    return r


def test_scratch_is_clean_afterwards(pkg, ctx2):
    a = mesh(pkg, "uniform_20000"); n = len(a)
    rng = np.random.default_rng(71)
    c = pkg.Context(0)
    try:
        for algo in (1, 3):
            bld = pkg.BUILDERS[algo]().build(c, a)
            cur = a
            sv = snap(pkg, c, bld.result)["svals"]
            d_c = None
            for k in range(20):
                m = (1, 2, 37, 200, 2000, n)[k % 6]
                prims = sv[:m].copy() if k % 2 else rng.choice(n, m, replace=False).astype(np.uint32)
                cur = move_subset(cur, prims, 100 + k, 0.01)
                d_new = c.upload(cur)
                bld.refit_subset(prims, tris=d_new)
                c.synchronize()
                if d_c is not None:
                    d_c.free()
                d_c = d_new                                       # (the tree's d_tris: alive until the queries below are done)
            fresh = pkg.BUILDERS[algo]().build(ctx2, a).refit(cur)
            assert bld.checksum() == fresh.checksum(), f"algo {algo}: 20 subset refits"
            same_bytes(snap(pkg, c, bld.result), snap(pkg, ctx2, fresh.result), f"algo {algo}: 20 subset refits")
            rays = make_rays(pkg, cur, 4096, 5)
            c3 = pkg.Context(0)                                   # (a build on ctx2 would overwrite fresh's tree, which lives in ctx2's arena)
            try:
                built = pkg.BUILDERS[algo]().build(c3, cur)
                assert bld.intersect(rays, "closest").tobytes() == built.intersect(rays, "closest").tobytes()
            finally:
                c3.close()
            c.synchronize(); d_c.free()
            b2 = jitter(cur, 9)
            assert bld.refit(b2).checksum() == fresh.refit(b2).checksum(), f"algo {algo}: full refit afterwards"
            assert bld.optimize(3).checksum() == fresh.optimize(3).checksum(), f"algo {algo}: optimize afterwards"
        for algo in ALGOS:
            assert pkg.BUILDERS[algo]().build(c, a).checksum() == pkg.BUILDERS[algo]().build(ctx2, a).checksum(), f"rebuild with algo {algo}"
    finally:
        c.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [1, 3])
def test_subset_errors_change_nothing(pkg, algo):
    a = mesh(pkg, "uniform_20000"); n = len(a)
    prims = np.arange(0, n, 7, dtype=np.uint32)
    bm = move_subset(a, prims, 14, 0.01)
    c = pkg.Context(0)
    try:
        c.reserve(n)
        b = pkg.BUILDERS[algo]().build(c, a)
        L = pkg.lib()
        d_b, d_p = c.upload(bm), c.upload(prims)
        r = b.result
        before = snap(pkg, c, r)
        ok_in = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_b.ptr, None, None, 0, 0)
        m = len(prims)

        def variant(**kw):
            v = pkg.Result.from_buffer_copy(r)
            for k, x in kw.items():
                setattr(v, k, x)
            return v
        bad = [variant(n_leaves=1), variant(n_leaves=0), variant(layout=2), variant(d_nodes=None), variant(d_prim_aabbs=None), variant(d_scene_extent=None),
               variant(root=n - 1), variant(n_leaves=n + 1)]                  # (n + 1: above the ctx's capacity)
        bad.append(variant(d_leaves=None) if r.layout == 1 else variant(layout=1, d_leaves=None))
        for v in bad:
            assert L.bvh_refit_subset(c.handle, C.byref(v), C.byref(ok_in), d_p.ptr, m, None) == E_INVALID
        assert L.bvh_refit_subset(None, C.byref(r), C.byref(ok_in), d_p.ptr, m, None) == E_INVALID
        assert L.bvh_refit_subset(c.handle, None, C.byref(ok_in), d_p.ptr, m, None) == E_INVALID
        for inp in (pkg.BuildInput(7, 30, d_b.ptr, None, None, 0, 0), pkg.BuildInput(pkg.TRI_PADDED64, 30, None, None, None, 0, 0),
                    pkg.BuildInput(pkg.TRI_PACKED36, 30, d_b.ptr + 4, None, None, 0, 0), pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_b.ptr, None, 0, 0)):
            assert L.bvh_refit_subset(c.handle, C.byref(r), C.byref(inp), d_p.ptr, m, None) == E_INVALID
        assert L.bvh_refit_subset(c.handle, C.byref(variant(d_tris=None)), None, d_p.ptr, m, None) == E_INVALID      # NULL in, and no triangles in the tree
        assert L.bvh_refit_subset(c.handle, C.byref(r), C.byref(ok_in), None, m, None) == E_INVALID
        assert L.bvh_refit_subset(c.handle, C.byref(r), C.byref(ok_in), d_p.ptr, 1 << 30, None) == E_INVALID
        assert L.bvh_refit_subset(c.handle, C.byref(r), C.byref(ok_in), d_p.ptr, 0xFFFFFFFF, None) == E_INVALID
        # the list inside an array the call writes
        overlapping = [r.d_prim_aabbs, r.d_prim_aabbs + 24 * n - 4, r.d_nodes + 64, r.d_scene_extent]
        if r.layout == 1:
            overlapping.append(r.d_leaves + 28)
        for p in overlapping:
            assert L.bvh_refit_subset(c.handle, C.byref(r), C.byref(ok_in), p, 1, None) == E_INVALID
        assert L.bvh_refit_subset(c.handle, C.byref(r), C.byref(ok_in), r.d_prim_aabbs - 4 * m + 4, m, None) == E_INVALID
        c.synchronize()
        same_bytes(snap(pkg, c, r), before, "after the errors")
        # an empty list: 0, nothing touched (not even d_tris)
        tris_before = r.d_tris
        assert L.bvh_refit_subset(c.handle, C.byref(r), C.byref(ok_in), d_p.ptr, 0, None) == 0
        assert L.bvh_refit_subset(c.handle, C.byref(r), C.byref(ok_in), None, 0, None) == 0
        c.synchronize()
        assert r.d_tris == tris_before
        same_bytes(snap(pkg, c, r), before, "after an empty list")
        # and the same arguments without a mistake work
        assert L.bvh_refit_subset(c.handle, C.byref(r), C.byref(ok_in), d_p.ptr, m, None) == 0
        same_bytes(snap(pkg, c, r), expected(pkg, c, before, bm, prims), "the valid call")
        d_b.free(); d_p.free()
    finally:
        c.close()


# ---- a caller-owned stream ---------------------------------------------------------------------------------------------------------------------------------------
def test_subset_on_a_caller_owned_stream(pkg, ctx):
    import torch
    a = mesh(pkg, "uniform_20000"); n = len(a)
    prims = np.random.default_rng(81).choice(n, 400, replace=False).astype(np.uint32)
    bm = move_subset(a, prims, 16, 0.01)
    _, _, default = run_subset(pkg, ctx, 3, a, bm, prims)
    s = torch.cuda.Stream()
    c = pkg.Context(0, s.cuda_stream)
    try:
        assert c.stream == s.cuda_stream
        _, _, mine = run_subset(pkg, c, 3, a, bm, prims)
        same_bytes(mine, default, "caller-owned stream vs default")
    finally:
        c.close()
