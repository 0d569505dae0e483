"""GPU: bvh_refit / bvh_refit_ex (the tree's boxes recomputed from moved triangles, topology kept) on all four builders' trees."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from test_refit import reference_refit

pytestmark = pytest.mark.gpu

ALGOS = [0, 1, 2, 3]
E_INVALID = -10001


def no_negzero(tris):
    """-0.0 -> +0.0 in every coordinate: the order of a signed-zero min / max then cannot matter"""
    t = tris.copy()
    for f in ("v1", "v2", "v3"):
        a = t[f]; a[a == 0] = 0.0; t[f] = a
    return t


def jitter(tris, seed, scale=1e-3):
    rng = np.random.default_rng(seed)
    t = tris.copy()
    for f in ("v1", "v2", "v3"):
        t[f] = (t[f] + rng.normal(0.0, scale, t[f].shape)).astype(np.float32)
    return no_negzero(t)


def permuted(tris, seed):
    return tris[np.random.default_rng(seed).permutation(len(tris))].copy()


_MESHES = {}


def mesh(pkg, name):
    if name not in _MESHES:
        kind, n = name.split("_")
        n = int(n)
        _MESHES[name] = no_negzero(pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 11 + n % 7))
    return _MESHES[name]


def stage_e(pkg, ctx, tris):
    """bvh_stage_extents of tris: (prim boxes AABB[n], scene AABB[1])"""
    n = len(tris)
    d_t = ctx.upload(tris); d_b = ctx.alloc(n * pkg.AABB.itemsize); d_s = ctx.alloc(pkg.AABB.itemsize)
    assert pkg.lib().bvh_stage_extents(ctx.handle, d_t.ptr, n, d_b.ptr, d_s.ptr) == 0
    out = d_b.download(pkg.AABB, n), d_s.download(pkg.AABB, 1)
    for b in (d_t, d_b, d_s):
        b.free()
    return out


def _download(pkg, ctx, ptr, dtype, count):
    out = np.empty(count, dtype=dtype)
    assert pkg.lib().bvh_dev_download(ctx.handle, out.ctypes.data, ptr, out.nbytes) == 0
    return out


def check_moved(pkg, orc, ctx, b, before, tris_b):
    """b was refit to tris_b: links / prims / root untouched, leaf and prim boxes bitwise stage E's, scene extent stage E's, internal boxes = the
    numpy reference refit"""
    n = len(tris_b)
    got = b.download()
    assert got["root"] == before["root"]
    assert np.array_equal(got["nodes"]["left"], before["nodes"]["left"]) and np.array_equal(got["nodes"]["right"], before["nodes"]["right"])
    if got["leaves"] is not None:
        assert np.array_equal(got["leaves"]["prim"], before["leaves"]["prim"])
    assert np.array_equal(got["sorted_keys"], before["sorted_keys"]) and np.array_equal(got["sorted_vals"], before["sorted_vals"])
    eb, es = stage_e(pkg, ctx, tris_b)
    pb = _download(pkg, ctx, b.result.d_prim_aabbs, pkg.AABB, n)
    assert pb.tobytes() == eb.tobytes()
    assert got["scene"].tobytes() == es.tobytes()
    ref_n, ref_l = reference_refit(before["nodes"], before["leaves"], before["root"], n, before["layout"], eb)
    if got["layout"] == 0:
        assert got["nodes"][n - 1:].tobytes() == ref_n[n - 1:].tobytes()          # leaf records bitwise
    else:
        assert got["leaves"].tobytes() == ref_l.tobytes()
    for f in ("min", "max"):
        assert np.array_equal(got["nodes"][f][:n - 1], ref_n[f][:n - 1])
    return got


# ---- refit to the same mesh -------------------------------------------------------------------------------------------
SAME_SIZES = ["uniform_2", "uniform_3", "uniform_511", "uniform_512", "uniform_513", "uniform_1025", "sponza_262144", "uniform_2000000", "uniform_10000000"]


@pytest.mark.parametrize("name", SAME_SIZES)
def test_refit_back_to_the_same_mesh_reproduces_the_build(pkg, ctx, name):
    a = mesh(pkg, name)
    bm = permuted(a, 5) if len(a) > 3 else jitter(a, 5)
    for algo in ALGOS:
        b = pkg.BUILDERS[algo]().build(ctx, a)
        ck = b.checksum()
        b.refit(bm)
        if len(a) > 3:
            assert b.checksum() != ck
        b.refit(a)
        assert b.checksum() == ck, f"algo {algo}"


# ---- refit to a moved mesh ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform_513", "uniform_20000", "sponza_262144", "uniform_2000000"])
@pytest.mark.parametrize("move", ["jitter", "permute"])
def test_refit_to_a_moved_mesh(pkg, orc, ctx, name, move):
    a = mesh(pkg, name)
    bm = jitter(a, 9) if move == "jitter" else permuted(a, 9)
    for algo in ALGOS:
        b = pkg.BUILDERS[algo]().build(ctx, a)
        before = b.download()
        b.refit(bm)
        check_moved(pkg, orc, ctx, b, before, bm)


# ---- input formats, 60-bit keys -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_refit_input_formats_agree(pkg, orc, ctx, algo):
    a = mesh(pkg, "uniform_30000"); n = len(a)
    bm = jitter(a, 3)
    v = np.stack([bm["v1"], bm["v2"], bm["v3"]], axis=1).astype(np.float32)          # (n, 3, 3)
    d_pad = ctx.upload(bm); d_packed = ctx.upload(np.ascontiguousarray(v.reshape(n, 9)))
    d_verts = ctx.upload(np.ascontiguousarray(v.reshape(3 * n, 3))); d_idx = ctx.upload(np.arange(3 * n, dtype=np.uint32))
    results = []
    for fmt in ("padded_host", "padded_dev", "packed", "indexed"):
        b = pkg.BUILDERS[algo]().build(ctx, a)
        if fmt == "padded_host":
            b.refit(bm)
        elif fmt == "padded_dev":
            b.refit(d_pad, on_device=True, n=n)
        elif fmt == "packed":
            b.refit_ex(n=n, tris=d_packed, tri_format=pkg.TRI_PACKED36)
        else:
            b.refit_ex(n=n, vertices=d_verts, indices=d_idx, n_vertices=3 * n, tri_format=pkg.TRI_INDEXED)
        got = b.download()
        results.append((got["nodes"].tobytes(), None if got["leaves"] is None else got["leaves"].tobytes(), got["scene"].tobytes(),
                        _download(pkg, ctx, b.result.d_prim_aabbs, pkg.AABB, n).tobytes()))
    assert all(r == results[0] for r in results[1:])
    # a tree built with 60-bit keys
    d_a = ctx.upload(a)
    b = pkg.BUILDERS[algo]().build_ex(ctx, n, tris=d_a, morton_bits=60)
    before = b.download()
    assert b.result.key_bits == 64
    b.refit(d_pad, on_device=True, n=n)
    check_moved(pkg, orc, ctx, b, before, bm)
    for d in (d_pad, d_packed, d_verts, d_idx, d_a):
        d.free()


# ---- consumers of the refit tree ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_consumers_see_the_refit_tree(pkg, orc, ctx, algo):
    a = no_negzero(pkg.meshgen.load_tri(os.path.join(ROOT, "tests", "golden", "cornell382.tri")))
    bm = jitter(a, 21, 2e-3)
    n = len(a)
    b = pkg.BUILDERS[algo]().build(ctx, a)
    b.refit(bm)
    got = b.download()
    assert orc.validate_bvh2(got["nodes"], got["leaves"], got["root"], n, got["layout"]) == 0
    s_ref = orc.sah_bvh2(got["nodes"], got["leaves"], got["root"], n, got["layout"])[0]
    assert abs(b.sah_cost() - s_ref) <= 1e-9 * max(1.0, s_ref)
    wide, prims, total = b.collapse4()
    ow, opn, ototal = orc.collapse4(got["nodes"], got["leaves"], got["root"], n, got["layout"])
    assert total == ototal and orc.topology_hash4(wide, prims, total, n) == orc.topology_hash4(ow, opn, ototal, n)
    boxes = _download(pkg, ctx, b.result.d_prim_aabbs, pkg.AABB, n)
    c_got = orc.sah_bvh4(wide, prims, boxes, total, n)[0]; c_orc = orc.sah_bvh4(ow, opn, boxes, ototal, n)[0]
    assert abs(c_got - c_orc) <= 1e-9 * c_orc
    cam, xf = pkg.cornell_view()
    W = 256
    rgba, rays = b.render(bm, cam, xf, W)
    assert rgba[3::4].sum() > 255 * 1000, "the view must actually see geometry"
    onodes = got["nodes"] if got["layout"] == 0 else orc.ploc_to_lbvh_layout(got["nodes"], got["leaves"])
    img, overflow = orc.trace_while(rays, bm, onodes, xf, got["root"], W, n - 1)
    assert overflow == 0
    assert np.array_equal(rgba, img), f"{np.count_nonzero(rgba != img)} of {rgba.size} bytes differ"


# ---- the cached parent plan -----------------------------------------------------------------------------------------------
def test_plan_follows_a_rebuild_with_another_topology(pkg):
    n = 100_000
    a = mesh(pkg, "uniform_100000"); a2 = permuted(jitter(a, 1, 0.05), 2); b2 = jitter(a2, 3)
    c1, c2 = pkg.Context(0), pkg.Context(0)
    try:
        h = pkg.HPLOC().build(c1, a)
        h.refit(jitter(a, 4))
        p = pkg.PLOCNew().build(c1, a2)                           # same n, same d_nodes, another topology
        assert p.result.d_nodes == h.result.d_nodes
        p.refit(b2)
        fresh = pkg.PLOCNew().build(c2, a2).refit(b2)
        assert p.checksum() == fresh.checksum()
        assert p.download()["nodes"].tobytes() == fresh.download()["nodes"].tobytes()
    finally:
        c1.close(); c2.close()


def test_plan_follows_a_two_pass_emit_that_reuses_the_parent_scratch(pkg, orc):
    """bvh_emit_lbvh_two's one-launch path writes the ctx's parent array (not its nodes): the plan of the ctx's own tree must be made again"""
    a = mesh(pkg, "uniform_20000"); n = len(a)
    c = pkg.Context(0)
    try:
        h = pkg.HPLOC().build(c, a)
        ck = h.checksum()
        h.refit(jitter(a, 6))
        h.refit(a)
        assert h.checksum() == ck
        small = pkg.meshgen.uniform(5000, 8); m = len(small)
        fe = orc.front_end(small)
        d_b = c.upload(fe["boxes"]); d_k = c.upload(fe["skeys"]); d_v = c.upload(fe["svals"]); d_n = c.alloc((2 * m - 1) * 32)
        with c.options(lbvh="single"):
            assert pkg.lib().bvh_emit_lbvh_two(c.handle, d_b.ptr, d_k.ptr, d_v.ptr, m, d_n.ptr) == 0
        c.synchronize()
        ref = orc.build_tree(0, small)
        assert d_n.download(pkg.BVH2_NODE, 2 * m - 1).tobytes() == ref["nodes"].tobytes()
        h.refit(jitter(a, 6))
        h.refit(a)
        assert h.checksum() == ck
        for d in (d_b, d_k, d_v, d_n):
            d.free()
    finally:
        c.close()


# ---- the self-cleaning scratch ----------------------------------------------------------------------------------------------
def test_scratch_stays_clean_over_many_refits(pkg, orc):
    a = mesh(pkg, "uniform_20000"); n = len(a)
    bm = jitter(a, 12)
    c = pkg.Context(0)
    try:
        d_a, d_b = c.upload(a), c.upload(bm)
        expect = {}
        for algo in ALGOS:
            b = pkg.BUILDERS[algo]().build(c, a)
            ck_a = b.checksum()
            b.refit(bm)
            expect[algo] = (ck_a, b.checksum())
        options = [dict(), dict(lbvh="single", hploc="async"), dict(lbvh="block", hploc="block"), dict(ploc="iter")]
        refits = 0
        for rnd in range(5):
            for algo in ALGOS:
                with c.options(**options[(rnd + algo) % len(options)]):
                    b = pkg.BUILDERS[algo]().build(c, d_a, on_device=True, n=n)
                    for k in range(25):                           # back to back, no synchronisation in between
                        lib = pkg.lib()
                        assert lib.bvh_refit(c.handle, C.byref(b.result), d_b.ptr if k % 2 == 0 else d_a.ptr, 1, None) == 0
                        refits += 1
                    assert b.checksum() == expect[algo][1], (rnd, algo)
                    b.refit(d_a, on_device=True, n=n)
                    assert b.checksum() == expect[algo][0], (rnd, algo)
        assert refits == 500
        small = no_negzero(pkg.meshgen.load_tri(os.path.join(ROOT, "tests", "golden", "cornell382.tri")))
        with c.options(lbvh="single"):
            t = pkg.TwoPassLbvh().build(c, small)
        ref = orc.build_tree(0, small)
        assert t.checksum() == pkg.checksum_host(ref["nodes"], None, 0)
        d_a.free(); d_b.free()
    finally:
        c.close()


def test_build_after_refit_gives_the_golden_tree(pkg, orc, ctx):
    """a refit rewrites the result's own scene-extent slot only: the next build (which uses the other slot, reset by the previous build) is unaffected"""
    a = mesh(pkg, "uniform_20000"); n = len(a)
    for algo in (1, 0):
        ref = orc.build_tree(algo, a)
        b = pkg.BUILDERS[algo]().build(ctx, a)
        b.refit(jitter(a, 2, 0.5))
        b2 = pkg.BUILDERS[algo]().build(ctx, a)
        b3 = pkg.BUILDERS[algo]().build(ctx, a)
        for x in (b2, b3):
            assert x.checksum() == pkg.checksum_host(ref["nodes"], None, ref["root"])


# ---- caller-owned arrays --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_refit_of_caller_owned_arrays(pkg, algo):
    a = mesh(pkg, "uniform_20000"); n = len(a)
    bm = jitter(a, 13)
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        ck_a = b.checksum()
        r = b.result
        n_nodes = 2 * n - 1 if r.layout == 0 else n - 1
        own = {}
        for f, size in (("d_nodes", n_nodes * 32), ("d_leaves", n * 28 if r.layout == 1 else 0), ("d_prim_aabbs", n * 24), ("d_scene_extent", 24)):
            if size:
                own[f] = c.alloc(size)
                assert pkg.lib().bvh_dev_copy(c.handle, own[f].ptr, getattr(r, f), size) == 0
        mine = pkg.Result.from_buffer_copy(r)
        for f, buf in own.items():
            setattr(mine, f, buf.ptr)
        for _ in range(2):                                        # (a second call makes its plan again)
            assert pkg.lib().bvh_refit(c.handle, C.byref(mine), bm.ctypes.data, 0, None) == 0
        c.synchronize()
        assert b.checksum() == ck_a, "the ctx's own arrays were touched"
        ck_mine = C.c_uint64()
        assert pkg.lib().bvh_checksum(c.handle, C.byref(mine), C.byref(ck_mine)) == 0
        b.refit(bm)
        assert ck_mine.value == b.checksum()
        assert _download(pkg, c, mine.d_prim_aabbs, pkg.AABB, n).tobytes() == _download(pkg, c, r.d_prim_aabbs, pkg.AABB, n).tobytes()
        for buf in own.values():
            buf.free()
    finally:
        c.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [1, 3])
def test_refit_errors_change_nothing(pkg, algo):
    a = mesh(pkg, "uniform_20000"); n = len(a)
    bm = jitter(a, 14)
    c = pkg.Context(0)
    try:
        c.reserve(n)
        b = pkg.BUILDERS[algo]().build(c, a)
        ck = b.checksum()
        L = pkg.lib()
        d_b = c.upload(bm)
        r = b.result

        def variant(**kw):
            v = pkg.Result.from_buffer_copy(r)
            for k, x in kw.items():
                setattr(v, k, x)
            return v
        bad = [variant(n_leaves=1), variant(n_leaves=0), variant(layout=2), variant(d_nodes=None), variant(d_prim_aabbs=None), variant(d_scene_extent=None),
               variant(root=n - 1), variant(n_leaves=n + 1)]
        if r.layout == 1:
            bad.append(variant(d_leaves=None))
        else:
            bad.append(variant(layout=1, d_leaves=None))
        for v in bad:
            assert L.bvh_refit(c.handle, C.byref(v), d_b.ptr, 1, None) == E_INVALID
            assert L.bvh_refit_ex(c.handle, C.byref(v), C.byref(pkg.BuildInput(pkg.TRI_PADDED64, 30, d_b.ptr, None, None, 0, 0)), None) == E_INVALID
        assert L.bvh_refit(None, C.byref(r), d_b.ptr, 1, None) == E_INVALID
        assert L.bvh_refit(c.handle, None, d_b.ptr, 1, None) == E_INVALID
        assert L.bvh_refit(c.handle, C.byref(r), None, 1, None) == E_INVALID
        assert L.bvh_refit_ex(c.handle, C.byref(r), None, None) == E_INVALID
        for inp in (pkg.BuildInput(7, 30, d_b.ptr, None, None, 0, 0), pkg.BuildInput(pkg.TRI_PADDED64, 30, None, None, None, 0, 0),
                    pkg.BuildInput(pkg.TRI_PACKED36, 30, d_b.ptr + 4, None, None, 0, 0), pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_b.ptr, None, 0, 0)):
            assert L.bvh_refit_ex(c.handle, C.byref(r), C.byref(inp), None) == E_INVALID
        c.synchronize()
        assert b.checksum() == ck
        # n_leaves above the capacity: refused, the arena is not re-allocated — the last result stays valid
        big = pkg.meshgen.uniform(n + 1, 3)
        assert L.bvh_refit(c.handle, C.byref(variant(n_leaves=n + 1)), big.ctypes.data, 0, None) == E_INVALID
        assert b.checksum() == ck
        b.refit(bm)
        assert b.checksum() != ck
        d_b.free()
    finally:
        c.close()


# ---- non-finite coordinates --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_refit_with_nan_and_inf_coordinates(pkg, orc, ctx, algo):
    a = mesh(pkg, "uniform_20000"); n = len(a)
    bm = jitter(a, 15)
    rng = np.random.default_rng(15)
    for val in (np.nan, np.inf, -np.inf):
        idx = rng.choice(n, 40, replace=False)
        for k, i in enumerate(idx):
            f = ("v1", "v2", "v3")[k % 3]
            v = bm[f][i].copy()
            if k % 4 == 0:
                v[:] = val                        # a whole vertex
            else:
                v[k % 3] = val                    # one coordinate
            bm[f][i] = v
            if k % 10 == 0:                       # all three vertices on one axis
                for g in ("v1", "v2", "v3"):
                    w = bm[g][i].copy(); w[1] = val; bm[g][i] = w
    b = pkg.BUILDERS[algo]().build(ctx, a)
    before = b.download()
    b.refit(bm)
    got = b.download()
    eb, _ = stage_e(pkg, ctx, bm)
    pb = _download(pkg, ctx, b.result.d_prim_aabbs, pkg.AABB, n)
    assert pb.view(np.uint32).tobytes() == eb.view(np.uint32).tobytes()
    if got["layout"] == 0:
        prim = got["nodes"]["left"][n - 1:]
        leaf = got["nodes"][n - 1:]
    else:
        prim = got["leaves"]["prim"]; leaf = got["leaves"]
    for f in ("min", "max"):
        assert leaf[f].tobytes() == eb[f][prim].tobytes()
    assert orc.validate_bvh2(got["nodes"], got["leaves"], got["root"], n, got["layout"]) == 0
    ref_n, _ = reference_refit(before["nodes"], before["leaves"], before["root"], n, before["layout"], eb)
    for f in ("min", "max"):
        assert np.array_equal(got["nodes"][f][:n - 1], ref_n[f][:n - 1])
