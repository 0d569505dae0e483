"""GPU: the stage-level entry points of INTEGRATION.md's stage-by-stage migration path, across the arguments a caller can pass, not only the ones
the builds pass internally.

* bvh_sort_pairs / bvh_sort_pairs64 (Oro::RadixSort::sort(src, dst, n, startBit, endBit, stream)) against a stable numpy argsort of the key field
  [start, end): caller values and implicit (NULL) values, single-pass and narrow-digit ranges, offset starts, every tile edge of both tile shapes, key
  patterns that stress the padding digit and stability, the helping path of the look-back, and a context's scratch state across calls;
* bvh_stage_morton64 at bit budgets 3 .. 60 and bvh_stage_morton_plan at budgets other than 30 on the log2f-boundary scenes, against the oracle;
* bvh_stage_extents_ex with out-of-range vertex indices and packed triangles at every staging-tile edge."""
import contextlib
import ctypes as C
import itertools

import numpy as np
import pytest

from test_gpu_parity import _flat
from test_gpu_round4 import _boundary_scene, _ulps
from test_gpu_round5 import WIDE_EXTENTS, _stretched

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

BVH_E_INVALID_ARG, BVH_E_TOO_LARGE = -10001, -10002
SENTINEL = 0xA5                      # output bytes before every call: a slot the kernel never wrote reads 0xA5A5A5A5
WIDE_MIN_N = 1_000_000               # SORT_WIDE_MIN_N: the wide tile shape from here on
WIDE_TILE = {np.uint32: 512 * 13, np.uint64: 512 * 10}   # pairs per wide tile (sort.hip SortWide: 512 threads x SORT_WIDE_IPT 13 / 10 keys)
WIDE_WHOLE = 1_064_960               # a whole number of wide tiles for both key types: 160 x 6656 (u32), 208 x 5120 (u64): the last tile has no padding
assert all(WIDE_WHOLE % t == 0 for t in WIDE_TILE.values()) and WIDE_WHOLE >= WIDE_MIN_N


@contextlib.contextmanager
def _freed(*bufs):
    """device buffers that are freed when the block ends, also when an assertion fails inside it"""
    try:
        yield bufs
    finally:
        for b in bufs:
            if b is not None:
                b.free()


# ---- sort ---------------------------------------------------------------------------------------------------------
def _field(keys, lo, hi):
    width = 8 * keys.itemsize
    if hi - lo == width:
        return keys
    t = keys.dtype.type
    return (keys >> t(lo % width)) & t((1 << (hi - lo)) - 1)


def _reference(keys, vals, lo, hi):
    """Oro::RadixSort's contract: stable ascending order on key bits [lo, hi); NULL values sort the identity"""
    order = np.argsort(_field(keys, lo, hi), kind="stable")
    return keys[order], (order.astype(np.uint32) if vals is None else vals[order])


def _rand(rng, n, dt):
    return np.frombuffer(rng.bytes(n * np.dtype(dt).itemsize), dtype=dt).copy()


def _keys(pattern, n, dt, lo, hi, rng):
    k = _rand(rng, n, dt)
    ones = np.iinfo(dt).max
    if pattern == "uniform":
        return k
    if pattern == "dups":                        # 37 distinct keys: long runs of equal fields, stability decides the order
        return _rand(rng, 37, dt)[rng.integers(0, 37, n)]
    if pattern == "equal":
        return np.full(n, k[0], dt)
    if pattern == "outside":                     # equal inside [lo, hi), random outside it: the output is the input order
        m = dt((((1 << (hi - lo)) - 1) << lo) & int(ones))
        return (k & ~m) | (k[0] & m)
    if pattern == "ones":                        # every third key all ones: the padding keys' digit, with n off the tile grid
        k[::3] = ones
        return k
    if pattern == "sorted":
        return np.sort(k)
    if pattern == "reverse":
        return np.sort(k)[::-1].copy()
    raise ValueError(pattern)


def _sort_on_device(pkg, ctx, keys, vals, lo, hi):
    """one bvh_sort_pairs(64) call with sentinel-filled outputs; returns (keys_out, vals_out) after checking that the inputs are unchanged"""
    L = pkg.lib()
    n = len(keys); kb = keys.itemsize
    fn = L.bvh_sort_pairs64 if kb == 8 else L.bvh_sort_pairs
    with _freed(ctx.upload(keys), ctx.upload(vals) if vals is not None else None,
                ctx.upload(np.full(n * kb, SENTINEL, np.uint8)), ctx.upload(np.full(n * 4, SENTINEL, np.uint8))) as (dk, dv, ok, ov):
        assert fn(ctx.handle, dk.ptr, dv.ptr if dv is not None else None, n, ok.ptr, ov.ptr, lo, hi) == 0
        got_k, got_v = ok.download(keys.dtype, n), ov.download(np.uint32, n)
        assert np.array_equal(dk.download(keys.dtype, n), keys), "input keys changed"
        if dv is not None:
            assert np.array_equal(dv.download(np.uint32, n), vals), "input values changed"
    return got_k, got_v


def _check_sort(pkg, ctx, keys, vals, lo, hi, what=""):
    got_k, got_v = _sort_on_device(pkg, ctx, keys, vals, lo, hi)
    ek, ev = _reference(keys, vals, lo, hi)
    tag = f"{keys.dtype} n={len(keys)} [{lo}, {hi}) {'caller values' if vals is not None else 'NULL values'} {what}"
    assert np.array_equal(got_k, ek), f"{tag}: {np.count_nonzero(got_k != ek)} keys differ"
    assert np.array_equal(got_v, ev), f"{tag}: {np.count_nonzero(got_v != ev)} values differ"


def _vals(rng, n, caller):
    return rng.permutation(n).astype(np.uint32) if caller else None


EMPTY = {np.uint32: [(7, 7), (32, 32)], np.uint64: [(13, 13), (64, 64)]}
SINGLE_NARROW = {np.uint32: [(0, 1), (0, 5), (3, 9), (31, 32)], np.uint64: [(0, 1), (0, 5), (3, 9), (31, 32), (60, 64), (63, 64)]}
SINGLE_FULL = {np.uint32: [(0, 8), (8, 16), (24, 32)], np.uint64: [(0, 8), (24, 32), (56, 64)]}
MULTI = {np.uint32: [(1, 31), (5, 32), (13, 29)], np.uint64: [(1, 31), (1, 63), (17, 49), (32, 64), (0, 63), (0, 60)]}
FULL = {np.uint32: [(0, 32)], np.uint64: [(0, 64)]}
RANGES = [(dt, r) for dt in (np.uint32, np.uint64) for table in (EMPTY, SINGLE_NARROW, SINGLE_FULL, MULTI, FULL) for r in table[dt]]


@pytest.mark.parametrize("caller", [False, True], ids=["null_vals", "caller_vals"])
@pytest.mark.parametrize("dt,rng_", RANGES, ids=[f"{np.dtype(dt).name}-{lo}-{hi}" for dt, (lo, hi) in RANGES])
def test_sort_bit_ranges(pkg, ctx, dt, rng_, caller):
    """every kind of bit range at a few small sizes, both tile-edge sides of the narrow 3072-key tile"""
    lo, hi = rng_
    rng = np.random.default_rng(np.dtype(dt).itemsize * 100_000 + lo * 1000 + hi * 10 + caller)
    for n, pattern in ((1, "uniform"), (65, "uniform"), (3073, "ones"), (6145, "dups"), (6145, "uniform")):
        keys = _keys(pattern, n, dt, lo, hi, rng)
        _check_sort(pkg, ctx, keys, _vals(rng, n, caller), lo, hi, pattern)


SIZES = [1, 2, 63, 64, 65, 3071, 3072, 3073, 6145, 999_999, WIDE_MIN_N, WIDE_WHOLE, WIDE_WHOLE + 1]
SIZE_RANGES = {np.uint32: [(0, 32), (3, 9), (5, 32)], np.uint64: [(0, 64), (0, 63), (17, 49), (60, 64)]}


@pytest.mark.parametrize("dt", [np.uint32, np.uint64], ids=["u32", "u64"])
@pytest.mark.parametrize("n", SIZES)
def test_sort_sizes(pkg, ctx, n, dt):
    """every tile edge of both shapes (3072-key narrow tiles below 1 M keys; 512 x 13 = 6656 (u32) / 512 x 10 = 5120 (u64) wide tiles from there, WIDE_WHOLE a
    whole number of them for both) at a few ranges, with caller values on every range and NULL values on the first"""
    rng = np.random.default_rng(n * 7 + np.dtype(dt).itemsize)
    keys = _keys("uniform", n, dt, 0, 0, rng)
    if n > 100:
        keys[::5] = keys[1]                                   # duplicates: stability shows
    for j, (lo, hi) in enumerate(SIZE_RANGES[dt]):
        _check_sort(pkg, ctx, keys, _vals(rng, n, True), lo, hi)
        if j == 0:
            _check_sort(pkg, ctx, keys, None, lo, hi)


PATTERNS = ["uniform", "dups", "equal", "outside", "ones", "sorted", "reverse"]


@pytest.mark.parametrize("n", [3073, WIDE_MIN_N + 1])
@pytest.mark.parametrize("dt", [np.uint32, np.uint64], ids=["u32", "u64"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_sort_key_patterns(pkg, ctx, pattern, dt, n):
    rng = np.random.default_rng(PATTERNS.index(pattern) * 1000 + n % 1000 + np.dtype(dt).itemsize)
    ranges = [(5, 27), (3, 9)] if dt == np.uint32 else [(11, 50), (60, 64), (0, 63)]
    if pattern != "outside":
        ranges = [(0, 8 * np.dtype(dt).itemsize)] + ranges
    for lo, hi in ranges:
        keys = _keys(pattern, n, dt, lo, hi, rng)
        vals = _vals(rng, n, True)
        if pattern == "outside":
            got_k, got_v = _sort_on_device(pkg, ctx, keys, vals, lo, hi)
            assert np.array_equal(got_k, keys) and np.array_equal(got_v, vals), f"[{lo}, {hi}): keys equal in the field must keep the input order"
            got_k, got_v = _sort_on_device(pkg, ctx, keys, None, lo, hi)
            assert np.array_equal(got_k, keys) and np.array_equal(got_v, np.arange(n, dtype=np.uint32))
        else:
            _check_sort(pkg, ctx, keys, vals, lo, hi, pattern)
            if lo == 0 and hi == 8 * np.dtype(dt).itemsize:
                _check_sort(pkg, ctx, keys, None, lo, hi, pattern)


@pytest.mark.parametrize("knobs", [8, 32, 40])
@pytest.mark.parametrize("n", [6145, WIDE_WHOLE + 1])
def test_sort_helping_path(pkg, ctx, sched_opts, knobs, n):
    """BVH_OPT_SORT_TEST_KNOBS forces the look-back's helping path (8: tiles in reverse order, 32: help at the first empty poll): u64 keys with caller
    values on a sub-range (first pass with caller values, narrow top digit), a u32 sub-range, on both tile shapes"""
    sched_opts(sort_knobs=knobs)
    rng = np.random.default_rng(knobs * 100 + n % 97)
    k64 = _keys("dups" if knobs == 40 else "uniform", n, np.uint64, 0, 0, rng)
    for lo, hi in ((3, 61), (17, 49)):
        _check_sort(pkg, ctx, k64, _vals(rng, n, True), lo, hi, f"knobs {knobs}")
    _check_sort(pkg, ctx, k64, None, 3, 61, f"knobs {knobs}")
    k32 = _keys("ones", n, np.uint32, 0, 0, rng)
    _check_sort(pkg, ctx, k32, _vals(rng, n, True), 5, 30, f"knobs {knobs}")


def test_sort_scratch_state_across_calls(pkg, orc, ctx):
    """no state leaks between calls on one context: wide, narrow, u64, u32 sorts with different ranges back to back, then a build; and a fresh context whose
    first call is a sort (its arena grows from nothing, then again for a larger sort)"""
    rng = np.random.default_rng(77)
    seq = [(WIDE_WHOLE + 1, np.uint32, (0, 32)), (3073, np.uint32, (3, 9)), (WIDE_MIN_N, np.uint64, (0, 63)), (6145, np.uint64, (60, 64)),
           (70_001, np.uint32, (1, 31)), (WIDE_WHOLE, np.uint64, (17, 49)), (65, np.uint32, (31, 32)), (999_999, np.uint64, (0, 64))]
    for n, dt, (lo, hi) in seq:
        keys = _keys("dups" if n % 2 else "uniform", n, dt, lo, hi, rng)
        _check_sort(pkg, ctx, keys, _vals(rng, n, n % 3 != 0), lo, hi, "sequence")
    tris = pkg.meshgen.uniform(50_000, 19)
    got = pkg.SinglePassLbvh().build(ctx, tris).download()
    ref = orc.build_tree(1, tris)
    assert np.array_equal(got["sorted_keys"], ref["skeys"]) and np.array_equal(got["sorted_vals"], ref["svals"])
    assert got["root"] == ref["root"] and got["nodes"].tobytes() == ref["nodes"].tobytes()

    c2 = pkg.Context(0)
    try:
        for n, dt, (lo, hi) in ((6145, np.uint64, (1, 63)), (WIDE_WHOLE + 1, np.uint64, (0, 64)), (3073, np.uint32, (0, 5))):
            keys = _keys("uniform", n, dt, lo, hi, rng)
            _check_sort(pkg, c2, keys, _vals(rng, n, True), lo, hi, "fresh context")
    finally:
        c2.close()


def test_sort_argument_errors(pkg, ctx):
    """argument checks return before any launch; n >= 2^30 is refused before the pointers are used (small valid buffers suffice)"""
    L = pkg.lib()
    n = 64
    with _freed(*(ctx.alloc(n * 8) for _ in range(4))) as buf:
        k_in, v_in, k_out, v_out = (b.ptr for b in buf)
        for fn, width in ((L.bvh_sort_pairs, 32), (L.bvh_sort_pairs64, 64)):
            for args in ((k_in, v_in, n, k_out, v_out, 9, 8),              # start > end
                         (k_in, v_in, n, k_out, v_out, 0, width + 1),      # end past the key
                         (k_in, v_in, n, k_out, v_out, -1, 8),             # negative start
                         (k_in, v_in, 0, k_out, v_out, 0, width),          # n == 0
                         (None, v_in, n, k_out, v_out, 0, width),          # NULL keys_in
                         (k_in, v_in, n, None, v_out, 0, width),           # NULL keys_out
                         (k_in, v_in, n, k_out, None, 0, width)):          # NULL vals_out
                assert fn(ctx.handle, *args) == BVH_E_INVALID_ARG, (width, args[2], args[5:])
            assert fn(ctx.handle, k_in, v_in, 1 << 30, k_out, v_out, 0, width) == BVH_E_TOO_LARGE
            assert fn(ctx.handle, k_in, None, 0xFFFFFFFF, k_out, v_out, 0, width) == BVH_E_TOO_LARGE
        ctx.synchronize()


# ---- Morton codes -----------------------------------------------------------------------------------------------------
BUDGETS = [3, 4, 5, 6, 29, 30, 31, 32, 45, 59, 60]


def _line(t):
    t = t.copy()
    for v in ("v1", "v2", "v3"):
        t[v][:, 1] = 0.5
        t[v][:, 2] = -2.0
    return t


# name -> (generator, whether the codes stay within the budget's interleave); the needle / planar WIDE_EXTENTS scenes have axis ratios beyond 2^32, and their
# codes wrap (the reference's u32 arithmetic).  A case builds only its own scene.
MORTON_SCENES = {"uniform_3001": (lambda pkg: pkg.meshgen.uniform(3001, 41), True),
                 "sponza_20k": (lambda pkg: pkg.meshgen.sponza_like(20_000, 3), True),
                 "flat_2000": (lambda pkg: _flat(pkg.meshgen.uniform(2000, 13)), True),
                 "line_2000": (lambda pkg: _line(pkg.meshgen.uniform(2000, 14)), True)}
for _i, _ext in enumerate(WIDE_EXTENTS):
    MORTON_SCENES[f"wide_{_i}"] = (lambda pkg, ext=_ext: _stretched(pkg, 5000, ext, 3), False)


@pytest.mark.parametrize("name", list(MORTON_SCENES))
def test_morton64_every_budget(pkg, orc, ctx, name):
    make, bounded = MORTON_SCENES[name]
    tris = make(pkg); n = len(tris)
    boxes, scene = orc.prim_bounds(tris)
    L = pkg.lib()
    with _freed(ctx.upload(boxes), ctx.upload(scene), ctx.alloc(n * 8)) as (d_box, d_scene, d_k):
        for tb in BUDGETS:
            d_k.upload(np.full(n * 8, SENTINEL, np.uint8))
            assert L.bvh_stage_morton64(ctx.handle, d_box.ptr, n, d_scene.ptr, d_k.ptr, tb) == 0
            got = d_k.download(np.uint64, n)
            ref = orc.morton_codes64(boxes, scene, tb)
            assert np.array_equal(got, ref), f"budget {tb}: {np.count_nonzero(got != ref)} of {n} keys differ from the oracle"
            if bounded:
                # the interleave keeps the reference's X * 4 + Y * 2 + Z layout at every budget: a budget that does not split evenly over the axes puts the
                # longer axes' top bits up to two places above it (the 30- and 60-bit budgets of the builds split evenly)
                assert int(ref.max()) < 2 ** (tb + 2), f"budget {tb}: a key beyond the budget's interleave"
                if tb % 6 == 0:
                    assert int(ref.max()) < 2 ** tb, f"budget {tb}: a key beyond the budget"
            plan = (C.c_int32 * 10)()
            assert L.bvh_stage_morton_plan(ctx.handle, d_scene.ptr, tb, plan) == 0
            po = orc.morton_plan(scene, tb)
            assert list(plan) == po["axis"] + po["bits"] + po["pre"] + [po["pre_sum"], po["swap"]], f"budget {tb}: device plan != oracle plan"
        for tb in (2, 61, 0, -1):
            assert L.bvh_stage_morton64(ctx.handle, d_box.ptr, n, d_scene.ptr, d_k.ptr, tb) == BVH_E_INVALID_ARG
            assert L.bvh_stage_morton_plan(ctx.handle, d_scene.ptr, tb, (C.c_int32 * 10)()) == BVH_E_INVALID_ARG


@pytest.mark.parametrize("budget", [60, 59, 45, 31])
def test_morton_plan_budgets_at_log2_boundaries(pkg, orc, ctx, budget):
    """test_gpu_round4's log2f-boundary scenes (families A (r, 1, 1) and B (2r, r, 1), r = 2^k (1 +- 2 ulp), every axis order) at budgets other than 30, up to
    ratios 2^61 (a 60-bit budget clamps the prefix bits at 60, not 30): the device's plan equals the oracle's plan for the same budget, and the device's u64 keys
    equal the oracle's.  The oracle takes the exact floor of log2 (the ratio's binary exponent), which is what the device's log2f truncates to."""
    L = pkg.lib()
    plan = (C.c_int32 * 10)()
    n = 96                                                     # (_boundary_scene's triangle count)
    scenes = 0; plan_diff = []; key_diff = []
    with _freed(ctx.alloc(n * 24), ctx.alloc(32), ctx.alloc(n * 8)) as (d_box, d_scene, d_keys):
        for perm in itertools.permutations(range(3)):
            for k in list(range(1, 31)) + [31, 32, 45, 59, 60, 61]:
                for d in (-2, -1, 0, 1, 2):
                    r = _ulps(np.float32(2.0) ** k, d)
                    for e in ((r, np.float32(1), np.float32(1)), (np.float32(2) * r, r, np.float32(1))):
                        tris = _boundary_scene(pkg, perm, e, n=n, seed=scenes)
                        boxes, scene = orc.prim_bounds(tris)
                        got_e = scene.view(np.float32)[3:6] - scene.view(np.float32)[0:3]
                        assert np.array_equal(np.sort(got_e), np.sort(np.asarray(e, np.float32))), "scene construction"
                        d_box.upload(boxes); d_scene.upload(scene); d_keys.upload(np.full(n * 8, SENTINEL, np.uint8))
                        assert L.bvh_stage_morton_plan(ctx.handle, d_scene.ptr, budget, plan) == 0
                        po = orc.morton_plan(scene, budget)
                        if list(plan) != po["axis"] + po["bits"] + po["pre"] + [po["pre_sum"], po["swap"]]:
                            plan_diff.append((perm, k, d, list(plan), po))
                        assert L.bvh_stage_morton64(ctx.handle, d_box.ptr, n, d_scene.ptr, d_keys.ptr, budget) == 0
                        if not np.array_equal(d_keys.download(np.uint64, n), orc.morton_codes64(boxes, scene, budget)):
                            key_diff.append((perm, k, d))
                        scenes += 1
    print(f"\nbudget {budget}: {scenes} boundary scenes; plan differs on {len(plan_diff)}, keys differ on {len(key_diff)}")
    for x in plan_diff[:8]:
        print("   axes %s  2^%d %+d ulp: device plan %s, oracle plan %s" % x)
    assert not plan_diff, "device plan != oracle plan"
    assert not key_diff, f"device keys != oracle keys on {key_diff[:8]}"


# ---- stage E ------------------------------------------------------------------------------------------------------
NAN_SCENE = np.full(32, 0xFF, np.uint8)            # the scene-extent output before every call: NaN bytes, so a missing reset shows


def _padded(pkg, v0, v1, v2):
    t = np.zeros(len(v0), dtype=pkg.meshgen.TRIANGLE)
    t["v1"], t["v2"], t["v3"] = v0, v1, v2
    return t


def _extents_ex(pkg, ctx, inp, n):
    L = pkg.lib()
    with _freed(ctx.upload(np.full(n * 24, SENTINEL, np.uint8)), ctx.upload(NAN_SCENE)) as (d_box, d_scene):
        assert L.bvh_stage_extents_ex(ctx.handle, C.byref(inp), n, d_box.ptr, d_scene.ptr) == 0
        return d_box.download(pkg.AABB, n), d_scene.download(pkg.AABB, 1)


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 4099])
def test_indexed_out_of_range_indices_read_vertex_0(pkg, orc, ctx, n):
    """bvh_build_input: indices >= n_vertices are read as vertex 0, never out of bounds"""
    rng = np.random.default_rng(n)
    nv = max(4, n // 2)
    verts = (rng.random((nv, 3), dtype=np.float32) * np.float32(4.0) - np.float32(1.5)).astype(np.float32)
    verts[0] = (-7.0, 9.0, 0.125)                  # vertex 0 lies outside the others' box: a substitution shows in the boxes and the scene
    idx = rng.integers(1, nv, (n, 3), dtype=np.uint32)
    bad = np.array([nv, nv + 1, 0xFFFFFFFF, 0x80000000, 2 * nv], np.uint32)
    sel = rng.random((n, 3)) < 0.3
    sel[0, 1] = True                               # at least one
    idx[sel] = bad[rng.integers(0, len(bad), int(sel.sum()))]
    with _freed(ctx.upload(verts), ctx.upload(idx)) as (d_v, d_i):
        boxes, scene = _extents_ex(pkg, ctx, pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, nv, 0), n)
    safe = np.where(idx < nv, idx, 0)
    rb, rs = orc.prim_bounds(_padded(pkg, verts[safe[:, 0]], verts[safe[:, 1]], verts[safe[:, 2]]))
    tri = verts[safe]                               # (n, 3 vertices, 3 coords): the plain min / max agrees with the oracle
    assert np.array_equal(rb["min"], tri.min(axis=1)) and np.array_equal(rb["max"], tri.max(axis=1))
    assert boxes.tobytes() == rb.tobytes(), f"{np.count_nonzero(boxes != rb)} boxes differ"
    assert scene.tobytes() == rs.tobytes()


@pytest.mark.parametrize("n", [4, 5, 6, 7, 255, 256, 257, 513])
def test_packed36_staging_tile_edges(pkg, orc, ctx, n):
    """BVH_TRI_PACKED36 at n mod 4 = 0..3 (the 16-byte staging loads and their word tail) and around EM_BLOCK = 256 triangles (one staging tile)"""
    tris = pkg.meshgen.uniform(n, 500 + n)
    pk = np.ascontiguousarray(np.concatenate([tris["v1"], tris["v2"], tris["v3"]], axis=1).astype(np.float32))
    with _freed(ctx.upload(pk)) as (d_pk,):
        boxes, scene = _extents_ex(pkg, ctx, pkg.BuildInput(pkg.TRI_PACKED36, 30, d_pk.ptr, None, None, 0, 0), n)
    rb, rs = orc.prim_bounds(tris)
    assert boxes.tobytes() == rb.tobytes(), f"{np.count_nonzero(boxes != rb)} boxes differ"
    assert scene.tobytes() == rs.tobytes()
