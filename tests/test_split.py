"""CPU: bvh_split_refs / bvh_remap_leaves in the C ABI, the library and the Python binding, and the numpy restatement of the split rule (include/bvh_mi355x.h,
refs(box, depth)) that the GPU tests (tests/test_gpu_split.py) compare against — itself checked byte for byte against goldens written by the reference's
Utility::doEarlySplitClipping (tests/golden/split_*.primref; the generator asserted depth <= 16 and min < c < max at every split, so neither of this library's
two extra emit rules fired) and against the oracle's identity PrimRefs.  Also here: the test meshes, ray / point sets and "split-well-conditioned" masks the GPU
tests use, computed once per process."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_query import accepted, brute_force, ray_ok, tri_formula, tri_vertices
from test_point_query import point_brute_force

E_INVALID = -10001
F32 = np.float32
FLT_MAX = F32(3.4028234663852886e38)
WELL_GROW = 2.0 ** -17           # "in some reference box of its triangle grown by 2^-17 * m_R"
MAX_DEPTH = 16
HEAVY_MIN = 64                   # csrc/split.hip SPLIT_HEAVY_MIN: more references than this and a wave fills the triangle
GOLDEN_MESHES = ("cornell32", "cornell82", "cornell382")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------------

def root_boxes(tris):
    """stage E's box per triangle, its expression: fminf(FLT_MAX, fminf(fminf(a, b), c)) / fmaxf(-FLT_MAX, ...) per axis (fmin / fmax skip NaN)"""
    a, b, c = (np.ascontiguousarray(tris[f], dtype=F32) for f in ("v1", "v2", "v3"))
    with np.errstate(invalid="ignore"):
        lo = np.fmin(FLT_MAX, np.fmin(np.fmin(a, b), c)).astype(F32)
        hi = np.fmax(-FLT_MAX, np.fmax(np.fmax(a, b), c)).astype(F32)
    return lo, hi


def split_refs_np(tris, sa_max, max_depth=MAX_DEPTH):
    """refs(box, depth) of the header in float32, level by level over all triangles at once; canonical order (triangle index, then depth-first, left first:
    a triangle's leaves are a prefix-free set of paths, so ordering the left-aligned paths is the depth-first order).
    Returns (offsets u32[n + 1], boxes AABB[total], prims u32[total], depths u32[total])."""
    from bvh_pkg import load
    pkg = load()
    n = len(tris)
    lo, hi = root_boxes(tris)
    sa = F32(sa_max)
    prim = np.arange(n, dtype=np.int64); path = np.zeros(n, dtype=np.int64)
    out_prim, out_key, out_depth, out_lo, out_hi = [], [], [], [], []
    depth = 0
    with np.errstate(all="ignore"):
        while len(prim):
            ext = (hi - lo).astype(F32)
            ex, ey, ez = ext[:, 0], ext[:, 1], ext[:, 2]
            area = F32(2) * ((ex * ey + ex * ez) + ey * ez)
            dim = np.where((ex > ey) & (ex > ez), 0, np.where(ey > ez, 1, 2))
            rows = np.arange(len(prim))
            l, h = lo[rows, dim], hi[rows, dim]
            c = ((h + l) * F32(0.5)).astype(F32)
            emit = ~(area > sa) | (depth == max_depth) | ~((l < c) & (c < h))
            out_prim.append(prim[emit]); out_key.append(path[emit] << (MAX_DEPTH - depth)); out_depth.append(np.full(int(emit.sum()), depth))
            out_lo.append(lo[emit]); out_hi.append(hi[emit])
            k = ~emit
            lo_k, hi_k, c_k, dim_k, rk = lo[k], hi[k], c[k], dim[k], np.arange(int(k.sum()))
            l_hi = hi_k.copy(); l_hi[rk, dim_k] = c_k
            r_lo = lo_k.copy(); r_lo[rk, dim_k] = c_k
            prim = np.concatenate([prim[k], prim[k]]); path = np.concatenate([path[k] << 1, (path[k] << 1) | 1])
            lo = np.concatenate([lo_k, r_lo]); hi = np.concatenate([l_hi, hi_k])
            depth += 1
    p = np.concatenate(out_prim); key = np.concatenate(out_key)
    order = np.lexsort((key, p))
    boxes = np.zeros(len(p), dtype=pkg.AABB)
    boxes["min"] = np.concatenate(out_lo)[order]; boxes["max"] = np.concatenate(out_hi)[order]
    prims = p[order].astype(np.uint32)
    offsets = np.zeros(n + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(np.bincount(prims, minlength=n))
    return offsets, boxes, prims, np.concatenate(out_depth)[order].astype(np.uint32)


def as_primrefs(pkg, boxes, prims):
    r = np.zeros(len(prims), dtype=pkg.PRIMREF)
    r["prim"] = prims; r["min"] = boxes["min"]; r["max"] = boxes["max"]
    return r


def sort_refs(r):
    """the goldens' order: (prim, min, max) by value, bit patterns last"""
    vals = np.concatenate([r["min"], r["max"]], axis=1)
    bits = np.ascontiguousarray(vals).view(np.uint32)
    keys = [bits[:, k] for k in range(5, -1, -1)] + [vals[:, k] for k in range(5, -1, -1)] + [r["prim"]]
    return r[np.lexsort(keys)]


def largest_root_area(tris):
    lo, hi = root_boxes(tris)
    ext = (hi - lo).astype(F32)
    with np.errstate(all="ignore"):
        a = F32(2) * ((ext[:, 0] * ext[:, 1] + ext[:, 0] * ext[:, 2]) + ext[:, 1] * ext[:, 2])
    return F32(np.nanmax(a))


def golden_cases():
    return json.load(open(os.path.join(GOLDEN, "split_cases.json")))["cases"]


def golden_mesh(pkg, name):
    return pkg.meshgen.load_tri(os.path.join(GOLDEN, name + ".tri"))


# ---- the GPU tests' special meshes ------------------------------------------------------------------------------------------------------------------------

def _tri(pkg, rows):
    t = np.zeros(len(rows), dtype=pkg.meshgen.TRIANGLE)
    a = np.asarray(rows, dtype=F32).reshape(-1, 3, 3)
    t["v1"], t["v2"], t["v3"] = a[:, 0], a[:, 1], a[:, 2]
    return t


def mesh70(pkg):
    """70 triangles (two waves): 68 small ones and, at indices 3 and 68, two large ones; with SA70 the large ones take several hundred references each"""
    t = pkg.meshgen.uniform(70, 9).copy()
    big = _tri(pkg, [[(0.0, 0.0, 0.0), (2.0, 0.1, 1.0), (0.3, 2.0, 0.2)], [(1.0, 1.0, 1.0), (-0.5, 1.2, 0.2), (0.5, -0.6, 1.8)]])
    t[3] = big[0]; t[68] = big[1]
    return t


SA70 = F32(0.5)


def ulp_grid_triangle(pkg):
    """one triangle at 2^24, where a float's spacing is 2: its box is 7 x 7 x 3 spacings, a cut can only fall on the grid, and a piece one spacing long cannot be
    cut (the no-progress rule emits it).  With sa_max = 0 the split tree has 147 leaves at depths 5 .. 8: heavy, with leaves above depth 6"""
    b = 16777216.0
    return _tri(pkg, [[(b, b, b), (b + 14, b, b + 6), (b, b + 14, b)]])


def sliver_triangle(pkg):
    """a long thin sliver: 100 x 1e-3 x 0 (axis-aligned, zero extent in z)"""
    return _tri(pkg, [[(0.0, 0.0, 0.5), (100.0, 0.0, 0.5), (100.0, 1e-3, 0.5)]])


def special_cases(pkg):
    """name -> (tris, sa_max, max_depth): the cases of the GPU byte-for-byte test besides the goldens"""
    nan = float("nan")
    two = _tri(pkg, [[(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(2, 2, 2), (2.5, 2, 2), (2, 2.5, 2.25)]])
    odd = _tri(pkg, [[(nan, 0, 0), (nan, 1, 0), (nan, 0, 3)],               # an all-NaN axis: stage E keeps +-FLT_MAX there, the area is not > sa_max: one reference
                     [(nan, nan, nan), (4, 0, 0), (0, 4, 1)],                 # one NaN vertex: fminf / fmaxf skip it, the box of the other two is split as usual
                     [(0, 0, 1), (3, 0, 1), (0, 3, 1)],                       # axis-aligned, zero extent in z
                     [(1, 1, 1), (1, 1, 1), (1, 1, 1)],                       # a point: zero area
                     [(0, 0, 0), (5, 0, 0), (2, 0, 0)],                       # a segment: zero area
                     [(-3e38, 0, 0), (3e38, 1, 0), (0, 0, 1)]])               # ext.x overflows to +inf
    return {
        "n1": (two[:1], F32(0.01), MAX_DEPTH),
        "n2_unsplit": (two, F32(100.0), MAX_DEPTH),
        "mesh70": (mesh70(pkg), SA70, MAX_DEPTH),
        "ulp_grid": (ulp_grid_triangle(pkg), F32(0.0), MAX_DEPTH),
        "sliver": (sliver_triangle(pkg), F32(1e-5), MAX_DEPTH),
        "depth3": (np.concatenate([mesh70(pkg)[:9], odd]), F32(0.0), 3),
        "odd": (odd, F32(0.5), MAX_DEPTH),
        "odd_deep": (odd[1:], F32(0.0), MAX_DEPTH),
    }


# ---- queries through split trees: meshes, ray / point sets, split-well-conditioned masks ----------------------------------------------------------------
QUERY_CASES = {"sponza_4096": 16, "cornell382": 64}          # mesh -> sa_max = the largest root-box area / this
_QUERY = {}


def query_mesh(pkg, name):
    from test_gpu_query import mesh
    return mesh(pkg, name)


def ray_split_well(rays, tris, offsets, boxes, chunk_elems=1 << 22):
    """per ray: every accepted hit's point (f64) lies in SOME reference box of its triangle grown by WELL_GROW * that box's largest |coordinate|"""
    v0, v1, v2 = tri_vertices(tris)
    lo = boxes["min"].astype(np.float64); hi = boxes["max"].astype(np.float64)
    g = WELL_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True)
    glo, ghi = lo - g, hi + g
    off = offsets.astype(np.int64)
    m, n = len(rays), len(tris)
    well = np.ones(m, dtype=bool)
    ok = ray_ok(rays)
    step = max(1, chunk_elems // max(n, 1))
    for s in range(0, m, step):
        r = rays[s:s + step]
        o = np.ascontiguousarray(r["origin"], dtype=F32)[:, None, :]; d = np.ascontiguousarray(r["direction"], dtype=F32)[:, None, :]
        it, iu, iv, iw = tri_formula(o, d, v0[None], v1[None], v2[None])
        acc = accepted(it, iu, iv, iw, r["tmin"][:, None], r["tmax"][:, None]) & ok[s:s + step, None]
        ri, pi = np.nonzero(acc)
        if not ri.size:
            continue
        p = r["origin"][ri].astype(np.float64) + it[ri, pi].astype(np.float64)[:, None] * r["direction"][ri].astype(np.float64)
        cnt = off[pi + 1] - off[pi]
        pair = np.repeat(np.arange(len(ri)), cnt)
        ref = np.repeat(off[pi], cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        inside = ((p[pair] >= glo[ref]) & (p[pair] <= ghi[ref])).all(axis=1)
        some = np.zeros(len(ri), dtype=bool); np.logical_or.at(some, pair, inside)
        bad = np.zeros(len(r), dtype=bool); np.logical_or.at(bad, ri, ~some)
        well[s:s + step] &= ~bad
    return well


def point_split_well(points, bf, offsets, boxes):
    """per query: the f64 squared distance from the point to SOME reference box of the winner, grown by WELL_GROW * that box's largest |coordinate|, is <= the
    winner's dist2 (misses are well-conditioned, as in the brute force)"""
    lo = boxes["min"].astype(np.float64); hi = boxes["max"].astype(np.float64)
    g = WELL_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True)
    glo, ghi = lo - g, hi + g
    off = offsets.astype(np.int64)
    well = np.ones(len(points), dtype=bool)
    idx = np.nonzero(bf["hit"])[0]
    w = bf["closest"]["prim"][idx].astype(np.int64)
    cnt = off[w + 1] - off[w]
    pair = np.repeat(np.arange(len(idx)), cnt)
    ref = np.repeat(off[w], cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    pp = points["point"][idx].astype(np.float64)[pair]
    dd = np.maximum(np.maximum(glo[ref] - pp, pp - ghi[ref]), 0.0)
    close = (dd * dd).sum(axis=1) <= bf["closest"]["dist2"][idx].astype(np.float64)[pair]
    some = np.zeros(len(idx), dtype=bool); np.logical_or.at(some, pair, close)
    well[idx] = some
    return well


def query_reference(pkg, name):
    """per mesh, computed once: tris, sa_max, the restated references, rays + brute force + split-well mask, points + brute force + split-well mask"""
    if name not in _QUERY:
        from test_gpu_query import make_rays
        from test_gpu_point_query import make_points
        tris = query_mesh(pkg, name)
        sa = F32(largest_root_area(tris) * F32(1.0 / QUERY_CASES[name]))
        offsets, boxes, prims, _ = split_refs_np(tris, sa)
        rays = make_rays(pkg, tris, 1024, 23 + len(tris))
        bf = brute_force(rays, tris)
        pts = make_points(pkg, tris, 1024, 29 + len(tris))
        pbf = point_brute_force(pkg, pts, tris)
        _QUERY[name] = {"tris": tris, "sa_max": sa, "offsets": offsets, "boxes": boxes, "prims": prims, "rays": rays, "bf": bf,
                        "ray_well": ray_split_well(rays, tris, offsets, boxes), "points": pts, "pbf": pbf,
                        "point_well": point_split_well(pts, pbf, offsets, boxes)}
    return _QUERY[name]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------------------

def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)


def test_header_declares_the_entry_points(pkg):
    text = header_text()
    assert re.search(r"#define\s+BVH_SPLIT_MAX_DEPTH\s+16\b", text) and pkg.SPLIT_MAX_DEPTH == MAX_DEPTH == 16
    assert re.search(r"\bint\s+bvh_split_refs\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*float\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*"
                     r"uint32_t\s*\*\s*\w+\s*,\s*bvh_aabb\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"\bint\s+bvh_remap_leaves\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*bvh_result\s*\*\s*\w+\s*,\s*const uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text


def test_library_exports_and_python_table_are_in_sync(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("bvh_split_refs", "bvh_remap_leaves"):
        assert hasattr(L, name) and name in pkg.EXPORTS
    lib = pkg.lib()
    assert lib.bvh_split_refs.argtypes[3] is C.c_float and len(lib.bvh_split_refs.argtypes) == 10 and len(lib.bvh_remap_leaves.argtypes) == 4
    assert lib.bvh_abi_version() == 4
    assert callable(pkg.Context.split_refs)
    for cls in pkg.BUILDERS.values():
        assert callable(cls.build_split) and callable(cls.remap_leaves) and callable(cls.split_arrays)
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().remap_leaves(np.zeros(4, dtype=np.uint32))          # no tree yet
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().split_arrays()


def test_errors_without_a_device(pkg):
    lib = pkg.lib()
    inp = pkg.BuildInput(pkg.TRI_PADDED64, 30, 4096, None, None, 0, 0)
    total = C.c_uint64(77)
    assert lib.bvh_split_refs(None, C.byref(inp), 4, 1.0, 16, 8192, None, None, 0, C.byref(total)) == E_INVALID and total.value == 77
    assert lib.bvh_split_refs(None, None, 0, float("nan"), 99, None, None, None, 0, None) == E_INVALID
    r = pkg.Result(); r.n_leaves = 4; r.layout = 0; r.d_nodes = 64
    assert lib.bvh_remap_leaves(None, C.byref(r), 4096, 4) == E_INVALID
    assert lib.bvh_remap_leaves(None, None, None, 0) == E_INVALID


# ---- the restatement against the reference ----------------------------------------------------------------------------------------------------------------

def test_goldens_are_small_and_complete():
    cases = golden_cases()
    assert sorted((c["mesh"], c["k"]) for c in cases) == sorted((m, k) for m in GOLDEN_MESHES for k in (8, 64))
    for c in cases:
        size = os.path.getsize(os.path.join(GOLDEN, c["file"]))
        assert size == 28 * c["count"] and size < 100_000
        assert c["max_depth_seen"] <= MAX_DEPTH


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: f"{c['mesh']}_{c['k']}")
def test_restatement_reproduces_the_reference_goldens(pkg, case):
    tris = golden_mesh(pkg, case["mesh"])
    sa = np.array([case["sa_max_bits"]], dtype=np.uint32).view(F32)[0]
    assert sa == F32(largest_root_area(tris) * F32(1.0 / case["k"]))   # 1/8 and 1/64 of the mesh's largest triangle-box area
    offsets, boxes, prims, depths = split_refs_np(tris, sa)
    assert offsets[-1] == len(prims) == case["count"] and depths.max() == case["max_depth_seen"]
    gold = np.fromfile(os.path.join(GOLDEN, case["file"]), dtype=pkg.PRIMREF)
    assert sort_refs(as_primrefs(pkg, boxes, prims)).tobytes() == gold.tobytes()
    assert depths.max() < MAX_DEPTH                                     # the cap never fired: the goldens are valid for this library's rule


def test_canonical_order_is_depth_first_left_first(pkg):
    """unsorted, the restatement's order is the recursion's: checked against a plain recursive evaluation of refs(box, depth)"""
    tris = golden_mesh(pkg, "cornell32")
    sa = F32(largest_root_area(tris) * F32(1.0 / 64))
    offsets, boxes, prims, depths = split_refs_np(tris, sa)
    lo0, hi0 = root_boxes(tris)

    def refs(lo, hi, depth, out):
        ext = hi - lo
        area = F32(2) * ((ext[0] * ext[1] + ext[0] * ext[2]) + ext[1] * ext[2])
        dim = 0 if (ext[0] > ext[1] and ext[0] > ext[2]) else (1 if ext[1] > ext[2] else 2)
        c = F32((hi[dim] + lo[dim]) * F32(0.5))
        if not (area > sa) or depth == MAX_DEPTH or not (lo[dim] < c < hi[dim]):
            out.append((lo.copy(), hi.copy(), depth)); return
        lh = hi.copy(); lh[dim] = c
        rl = lo.copy(); rl[dim] = c
        refs(lo, lh, depth + 1, out); refs(rl, hi, depth + 1, out)
    for p in range(len(tris)):
        out = []
        refs(lo0[p], hi0[p], 0, out)
        s = slice(int(offsets[p]), int(offsets[p + 1]))
        assert len(out) == s.stop - s.start and (prims[s] == p).all()
        assert np.array_equal(boxes["min"][s], np.array([o[0] for o in out])) and np.array_equal(boxes["max"][s], np.array([o[1] for o in out]))
        assert list(depths[s]) == [o[2] for o in out]
    assert (np.diff(prims.astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("name", GOLDEN_MESHES)
def test_identity_cases_equal_the_reference_primrefs(pkg, orc, name):
    """max_depth = 0 and sa_max = FLT_MAX: one reference per triangle, the oracle's PrimRefs (= Utility::doEarlySplitClipping with its default saMax, pinned by
    tests/test_oracle_golden.py) record for record"""
    tris = golden_mesh(pkg, name)
    expect = orc.primrefs(tris).tobytes()
    for sa, md in ((F32(0.0), 0), (FLT_MAX, MAX_DEPTH)):
        offsets, boxes, prims, depths = split_refs_np(tris, sa, md)
        assert list(offsets) == list(range(len(tris) + 1)) and not depths.any()
        assert as_primrefs(pkg, boxes, prims).tobytes() == expect


def test_special_cases_are_what_the_gpu_test_needs(pkg):
    sc = special_cases(pkg)
    off, _, _, _ = split_refs_np(*sc["mesh70"])
    cnt = np.diff(off.astype(np.int64))
    assert len(cnt) == 70 and 200 < cnt[3] < 2000 and 200 < cnt[68] < 2000          # heavy: several hundred references each, across a wave boundary
    assert (np.delete(cnt, [3, 68]) <= HEAVY_MIN).all() and (np.delete(cnt, [3, 68]) > 1).any()
    off, _, _, depths = split_refs_np(*sc["ulp_grid"])
    assert off[1] == 147 > HEAVY_MIN and depths.min() < 6 and depths.max() < MAX_DEPTH     # heavy, with a leaf above depth 6: lanes idle
    off, _, _, depths = split_refs_np(*sc["sliver"])
    assert off[1] > HEAVY_MIN
    tris, sa, md = sc["depth3"]
    off, boxes, _, depths = split_refs_np(tris, sa, md)
    cnt = np.diff(off.astype(np.int64))
    assert (cnt[:9] == 8).all() and depths.max() == 3                               # cut by max_depth: 8 references per non-degenerate triangle
    off, boxes, _, _ = split_refs_np(*sc["odd"])
    cnt = np.diff(off.astype(np.int64))
    assert cnt[0] == 1 and boxes["min"][0][0] == FLT_MAX and boxes["max"][0][0] == -FLT_MAX      # an all-NaN axis: one reference, stage E's clamped box
    assert cnt[3] == 1 and cnt[4] == 1                                              # zero-area boxes emit at once
    assert cnt[2] > 1                                                               # a zero-extent axis alone does not stop the split
    off, _, _, _ = split_refs_np(*sc["n2_unsplit"])
    assert list(off) == [0, 1, 2]


def test_references_tile_their_root_box(pkg):
    """sponza_like(4096): per triangle the references' boxes union to the root box, their volumes sum to the root's within f32 rounding, none is deeper than
    max_depth, and siblings share their cut plane (closed halves: no gap)"""
    tris = pkg.meshgen.sponza_like(4096, 3)
    sa = F32(largest_root_area(tris) * F32(1.0 / 64))
    for md in (MAX_DEPTH, 2):
        offsets, boxes, prims, depths = split_refs_np(tris, sa, md)
        assert depths.max() <= md and (md != 2 or depths.max() == 2)
        lo, hi = root_boxes(tris)
        start = offsets[:-1].astype(np.int64)
        assert (np.diff(offsets.astype(np.int64)) >= 1).all()
        assert np.array_equal(np.minimum.reduceat(boxes["min"], start, axis=0), lo) and np.array_equal(np.maximum.reduceat(boxes["max"], start, axis=0), hi)
        ext = boxes["max"].astype(np.float64) - boxes["min"].astype(np.float64)
        vol = np.add.reduceat(ext.prod(axis=1), start)
        root_ext = hi.astype(np.float64) - lo.astype(np.float64)
        root_vol = root_ext.prod(axis=1)
        # every cut plane is one f32 rounding of a midpoint: relative error <= depth * 2^-23 per axis extent, three axes
        assert (np.abs(vol - root_vol) <= 3 * MAX_DEPTH * 2.0 ** -23 * root_vol + 1e-300).all()
        assert (ext >= 0).all()


@pytest.mark.parametrize("name", list(QUERY_CASES))
def test_query_sets_are_split_well_conditioned(pkg, name):
    """the committed seeds: at least 99 % of the GPU tests' rays and points are split-well-conditioned, and that implies well-conditioned (§8b / §8e)"""
    q = query_reference(pkg, name)
    cnt = np.diff(q["offsets"].astype(np.int64))
    assert cnt.max() > 8 and q["offsets"][-1] > len(q["tris"])          # the mesh really is split
    assert q["ray_well"].mean() >= 0.99 and q["point_well"].mean() >= 0.99
    assert not (q["ray_well"] & ~q["bf"]["well"]).any() and not (q["point_well"] & ~q["pbf"]["well"]).any()
    assert q["bf"]["hit"].mean() > 0.25 and q["pbf"]["hit"].any()
