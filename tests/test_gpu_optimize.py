"""GPU: bvh_optimize (treelet restructuring, in place) on all four builders' trees, byte for byte against the numpy restatement of tests/test_optimize.py."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_refit import check_moved, jitter, no_negzero
from test_optimize import reference_optimize
from test_query import brute_force, recompute

pytestmark = pytest.mark.gpu

ALGOS = [0, 1, 2, 3]
E_INVALID = -10001

_MESHES = {}


def mesh(pkg, name):
    if name not in _MESHES:
        kind, n = name.split("_")
        n = int(n)
        _MESHES[name] = no_negzero(pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 17 + n % 5))
    return _MESHES[name]


def own_copy(pkg, c, r, keep):
    """a caller-filled result over bvh_dev_alloc copies of r's nodes / leaves (the rest still points at r's arrays)"""
    n = r.n_leaves
    mine = pkg.Result.from_buffer_copy(r)
    for f, size in (("d_nodes", (2 * n - 1 if r.layout == 0 else n - 1) * 32), ("d_leaves", n * 28 if r.layout == 1 else 0)):
        if size:
            buf = c.alloc(size); keep.append(buf)
            assert pkg.lib().bvh_dev_copy(c.handle, buf.ptr, getattr(r, f), size) == 0
            setattr(mine, f, buf.ptr)
    return mine


def lbvh_copy(pkg, c, r, keep):
    """a caller-filled layout-0 result: bvh_to_lbvh_layout of a PLOC-layout tree"""
    n = r.n_leaves
    buf = c.alloc((2 * n - 1) * 32); keep.append(buf)
    assert pkg.lib().bvh_to_lbvh_layout(c.handle, C.byref(r), buf.ptr) == 0
    mine = pkg.Result.from_buffer_copy(r)
    mine.d_nodes = buf.ptr; mine.d_leaves = None; mine.layout = 0
    return mine


def download(pkg, c, r):
    n = r.n_leaves
    nodes = np.empty(2 * n - 1 if r.layout == 0 else n - 1, dtype=pkg.BVH2_NODE)
    assert pkg.lib().bvh_dev_download(c.handle, nodes.ctypes.data, r.d_nodes, nodes.nbytes) == 0
    leaves = None
    if r.layout == 1:
        leaves = np.empty(n, dtype=pkg.PRIMREF)
        assert pkg.lib().bvh_dev_download(c.handle, leaves.ctypes.data, r.d_leaves, leaves.nbytes) == 0
    return nodes, leaves


def checksum(pkg, c, r):
    v = C.c_uint64()
    assert pkg.lib().bvh_checksum(c.handle, C.byref(r), C.byref(v)) == 0
    return int(v.value)


def optimize_and_compare(pkg, c, r, rounds, what):
    n = r.n_leaves
    nodes, leaves = download(pkg, c, r)
    want = reference_optimize(nodes, leaves, r.root, n, r.layout, rounds)
    assert pkg.lib().bvh_optimize(c.handle, C.byref(r), rounds, None) == 0, what
    got_n, got_l = download(pkg, c, r)
    assert got_n.tobytes() == want.tobytes(), f"{what}: nodes differ from the restatement ({np.count_nonzero(got_n != want)} records)"
    if leaves is not None:
        assert got_l.tobytes() == leaves.tobytes(), f"{what}: leaves written"
    if n < 7:
        assert got_n.tobytes() == nodes.tobytes(), f"{what}: a tree of {n} leaves changed"
    return nodes, got_n


# ---- bit-exact against the restatement --------------------------------------------------------------------------------------------------------------
EXACT = ["uniform_2", "uniform_3", "uniform_6", "uniform_7", "uniform_8", "uniform_63", "uniform_64", "uniform_65", "uniform_1000", "uniform_20000",
         "sponza_65536"]


@pytest.mark.parametrize("name", EXACT)
def test_bit_exact_against_the_restatement(pkg, ctx, name):
    a = mesh(pkg, name)
    changed = 0
    for algo in ALGOS:
        for rounds in (1, 2, 3):
            keep = []
            try:
                b = pkg.BUILDERS[algo]().build(ctx, a)
                before, after = optimize_and_compare(pkg, ctx, b.result, rounds, f"{name} algo {algo} rounds {rounds}")
                changed += before.tobytes() != after.tobytes()
                if b.result.layout == 1:                       # the other layout: the same tree in LBVH layout, in arrays of the caller's
                    b2 = pkg.BUILDERS[algo]().build(ctx, a)
                    optimize_and_compare(pkg, ctx, lbvh_copy(pkg, ctx, b2.result, keep), rounds, f"{name} algo {algo} rounds {rounds} layout 0")
            finally:
                for buf in keep:
                    buf.free()
    if len(a) >= 63:
        assert changed > 0


def test_python_method_keeps_the_published_result(pkg, orc, ctx):
    a = mesh(pkg, "sponza_65536"); n = len(a)
    for algo in ALGOS:
        b = pkg.BUILDERS[algo]().build(ctx, a)
        s0 = b.sah_cost()
        got0 = b.download()
        assert b.optimize() is b
        got = b.download()
        want = reference_optimize(got0["nodes"], got0["leaves"], got0["root"], n, got0["layout"], 3)
        assert got["nodes"].tobytes() == want.tobytes()
        s1 = b.sah_cost()
        s_orc = orc.sah_bvh2(got["nodes"], got["leaves"], got["root"], n, got["layout"])[0]
        assert abs(s1 - s_orc) <= 1e-9 * s_orc and s1 <= s0
        if algo in (0, 1):
            assert s1 < 0.9 * s0, (algo, s0, s1)


def test_timings_and_kernel_names(pkg):
    a = mesh(pkg, "uniform_20000")
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[1]().build(c, a)
        c.set_profiling(2)
        b.optimize(3)
        t = b.timings
        assert t.ms_build > 0 and t.ms_total == t.ms_build and t.ms_extents == 0 and t.ms_morton == 0 and t.ms_sort == 0
        k = c.kernel_times()
        assert k["k_optimize"][1] == 3 and k["k_refit_plan"][1] == 1, k
        c.set_profiling(2)
        b.optimize(1)                                             # the plan of the ctx's own tree is kept
        k = c.kernel_times()
        assert k["k_optimize"][1] == 1 and "k_refit_plan" not in k, k
    finally:
        c.close()


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_two_copies_of_one_build_agree(pkg, ctx, algo):
    a = mesh(pkg, "sponza_65536")
    b = pkg.BUILDERS[algo]().build(ctx, a)
    keep = []
    try:
        x, y = own_copy(pkg, ctx, b.result, keep), own_copy(pkg, ctx, b.result, keep)
        for r in (x, y, b.result):
            assert pkg.lib().bvh_optimize(ctx.handle, C.byref(r), 3, None) == 0
        assert checksum(pkg, ctx, x) == checksum(pkg, ctx, y) == checksum(pkg, ctx, b.result)
    finally:
        for buf in keep:
            buf.free()


# ---- large trees ---------------------------------------------------------------------------------------------------------------------------------
def check_tree(nodes, leaves, root, n, layout):
    """vectorised: every index but the root is a child exactly once, every internal box is the exact fmin / fmax union of its children's boxes"""
    ni = n - 1
    left = nodes["left"][:ni].astype(np.int64); right = nodes["right"][:ni].astype(np.int64)
    kids = np.concatenate([left, right])
    assert kids.min() >= 0 and kids.max() < 2 * n - 1
    seen = np.bincount(kids, minlength=2 * n - 1)
    expect = np.ones(2 * n - 1, dtype=np.int64); expect[root] = 0
    assert np.array_equal(seen, expect)
    if layout == 0:
        lo, hi = nodes["min"], nodes["max"]
    else:
        lo = np.concatenate([nodes["min"], leaves["min"]]); hi = np.concatenate([nodes["max"], leaves["max"]])
    assert np.array_equal(lo[:ni], np.fmin(lo[left], lo[right])) and np.array_equal(hi[:ni], np.fmax(hi[left], hi[right]))


@pytest.mark.parametrize("n", [2_000_000, 10_000_000])
@pytest.mark.parametrize("algo", [1, 3])
def test_large_trees(pkg, ctx, n, algo):
    a = mesh(pkg, f"uniform_{n}")
    b = pkg.BUILDERS[algo]().build(ctx, a)
    before = b.download()
    s0 = b.sah_cost()
    b.optimize(3)
    got = b.download()
    check_tree(got["nodes"], got["leaves"], got["root"], n, got["layout"])
    assert got["root"] == before["root"]
    if got["layout"] == 0:
        assert got["nodes"][n - 1:].tobytes() == before["nodes"][n - 1:].tobytes()
    else:
        assert got["leaves"].tobytes() == before["leaves"].tobytes()
    s1 = b.sah_cost()
    assert s1 <= s0 * (1 + 1e-6)
    if algo == 1:
        assert s1 < s0 * (1 - 1e-3), (s0, s1)


# ---- consumers -----------------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("algo", ALGOS)
def test_consumers_see_the_optimised_tree(pkg, orc, ctx, algo):
    a = mesh(pkg, "sponza_20000"); n = len(a)
    rays = make_rays(pkg, a, 4096, 3)
    bf = brute_force(rays, a)
    well = bf["well"]
    assert well.mean() >= 0.99
    b = pkg.BUILDERS[algo]().build(ctx, a)
    closest0 = b.intersect(rays, "closest")
    b.optimize(3)
    got = b.download()
    assert orc.validate_bvh2(got["nodes"], got["leaves"], got["root"], n, got["layout"]) == 0
    # closest hits do not depend on the tree; any hits are accepted hits
    closest1 = b.intersect(rays, "closest")
    for f in ("t", "u", "v", "prim"):
        assert np.array_equal(closest1[f].view(np.uint32)[well], closest0[f].view(np.uint32)[well]), f
    anyhit = b.intersect(rays, "any")
    assert recompute(rays, a, closest1).all() and recompute(rays, a, anyhit).all()
    assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"])[well].all()
    # BVH4 collapse and the LBVH-layout adapter read the new tree
    wide, prims, total = b.collapse4()
    ow, opn, ototal = orc.collapse4(got["nodes"], got["leaves"], got["root"], n, got["layout"])
    assert total == ototal and orc.topology_hash4(wide, prims, total, n) == orc.topology_hash4(ow, opn, ototal, n)
    buf = ctx.alloc((2 * n - 1) * 32)
    try:
        assert pkg.lib().bvh_to_lbvh_layout(ctx.handle, C.byref(b.result), buf.ptr) == 0
        lb = buf.download(pkg.BVH2_NODE, 2 * n - 1)
    finally:
        buf.free()
    want = got["nodes"] if got["layout"] == 0 else orc.ploc_to_lbvh_layout(got["nodes"], got["leaves"])
    assert lb.tobytes() == want.tobytes()
    assert orc.validate_bvh2(lb, None, got["root"], n, 0) == 0
    # a jittered refit refits the NEW topology (a stale parent plan would union the old children)
    bm = jitter(a, 31)
    b.refit(bm)
    check_moved(pkg, orc, ctx, b, got, bm)


@pytest.mark.parametrize("algo", [0, 1])
def test_build_and_refit_after_optimise_are_unaffected(pkg, orc, ctx, algo):
    a = mesh(pkg, "uniform_20000")
    fresh = pkg.BUILDERS[algo]().build(ctx, a).checksum()
    b = pkg.BUILDERS[algo]().build(ctx, a)
    b.optimize(3)
    assert b.checksum() != fresh
    b2 = pkg.BUILDERS[algo]().build(ctx, a)
    assert b2.checksum() == fresh
    before = b2.download()
    bm = jitter(a, 41)
    b2.refit(bm)
    check_moved(pkg, orc, ctx, b2, before, bm)
    b2.refit(a)
    assert b2.checksum() == fresh


# ---- caller-owned arrays -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [1, 3])
def test_caller_owned_arrays(pkg, orc, algo):
    a = mesh(pkg, "uniform_20000")
    c = pkg.Context(0)
    keep = []
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        b.refit(a)                                                    # (the ctx's own tree has a cached plan now)
        ck = b.checksum()
        mine = own_copy(pkg, c, b.result, keep)
        optimize_and_compare(pkg, c, mine, 3, "caller-owned")
        assert b.checksum() == ck, "the ctx's own arrays were touched"
        # the ctx's own tree is not disturbed: optimised, it equals the copy; a refit then uses the right plan
        before = b.download()
        b.optimize(3)
        assert b.checksum() == checksum(pkg, c, mine)
        got = b.download()
        want = reference_optimize(before["nodes"], before["leaves"], before["root"], len(a), before["layout"], 3)
        assert got["nodes"].tobytes() == want.tobytes()
        bm = jitter(a, 51)
        b.refit(bm)
        check_moved(pkg, orc, c, b, got, bm)
    finally:
        for buf in keep:
            buf.free()
        c.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [1, 3])
def test_errors_change_nothing(pkg, algo):
    a = mesh(pkg, "uniform_20000"); n = len(a)
    c = pkg.Context(0)
    try:
        c.reserve(n)
        b = pkg.BUILDERS[algo]().build(c, a)
        ck = b.checksum()
        L = pkg.lib()
        r = b.result

        def variant(**kw):
            v = pkg.Result.from_buffer_copy(r)
            for k, x in kw.items():
                setattr(v, k, x)
            return v
        bad = [variant(n_leaves=1), variant(n_leaves=0), variant(layout=2), variant(d_nodes=None), variant(root=n - 1), variant(root=2 * n),
               variant(n_leaves=n + 1)]
        bad.append(variant(d_leaves=None) if r.layout == 1 else variant(layout=1, d_leaves=None))
        for v in bad:
            assert L.bvh_optimize(c.handle, C.byref(v), 3, None) == E_INVALID
        for rounds in (0, 9, 1 << 31):
            assert L.bvh_optimize(c.handle, C.byref(r), rounds, None) == E_INVALID
        assert L.bvh_optimize(None, C.byref(r), 3, None) == E_INVALID
        assert L.bvh_optimize(c.handle, None, 3, None) == E_INVALID
        c.synchronize()
        assert b.checksum() == ck
        assert L.bvh_optimize(c.handle, C.byref(r), 8, None) == 0     # (the bounds themselves are accepted)
        assert L.bvh_optimize(c.handle, C.byref(r), 1, None) == 0
        c.synchronize()
    finally:
        c.close()
