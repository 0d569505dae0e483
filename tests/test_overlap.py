"""CPU: bvh_overlap in the C ABI, the library, the Python binding and the C++ mirror; the numpy brute force and query mix that the GPU overlap tests
(tests/test_gpu_overlap.py) compare against; and the premise that makes the answer exact — on the CPU oracle's trees every internal box is the bitwise
fminf / fmaxf union of its children's, so a walk that prunes with the overlap test returns exactly the brute force's sets."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_query import mesh

E_INVALID = -10001
E_TOO_LARGE = -10002
F32 = np.float32
AABB = np.dtype([("min", "<f4", 3), ("max", "<f4", 3)])
PREMISE_MESHES = ["uniform_2", "uniform_3", "uniform_65", "uniform_1000", "uniform_20000", "sponza_1000", "sponza_20000", "cornell32", "cornell382"]


# ---- the brute force --------------------------------------------------------------------------------------------------------------------------------------

def as_boxes(a):
    """an AABB record array from AABB records or an (m, 6) float array (min xyz, max xyz)"""
    a = np.asarray(a)
    if a.dtype == AABB:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a, dtype=F32).reshape(-1, 6).view(AABB).reshape(-1)


def overlap_pairs(q, b, chunk_elems=1 << 23):
    """(query index, box index) of every overlapping pair, exactly the header's test in f32: per axis q.min <= b.max && b.min <= q.max && q.min <= q.max &&
    b.min <= b.max — comparisons only, so NaN fails, -0 == +0, touching boxes pass and inverted boxes overlap nothing"""
    q, b = as_boxes(q), as_boxes(b)
    qlo, qhi, blo, bhi = q["min"].astype(F32), q["max"].astype(F32), b["min"].astype(F32), b["max"].astype(F32)
    with np.errstate(invalid="ignore"):
        qok = (qlo <= qhi).all(axis=1); bok = (blo <= bhi).all(axis=1)
    bx_lo, bx_hi = np.ascontiguousarray(blo[:, 0]), np.ascontiguousarray(bhi[:, 0])
    step = max(1, chunk_elems // max(len(b), 1))
    qi_all, bj_all = [], []
    for s in range(0, len(q), step):
        with np.errstate(invalid="ignore"):
            m = (qlo[s:s + step, 0, None] <= bx_hi[None]) & (bx_lo[None] <= qhi[s:s + step, 0, None])
            qi, bj = np.nonzero(m)
            qi += s
            keep = qok[qi] & bok[bj]
            for k in (1, 2):
                keep &= (qlo[qi, k] <= bhi[bj, k]) & (blo[bj, k] <= qhi[qi, k])
        qi_all.append(qi[keep]); bj_all.append(bj[keep])
    if not qi_all:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(qi_all), np.concatenate(bj_all)


def overlap_brute_force(boxes, leaf_boxes, self_pairs=False):
    """one sorted uint32 index array per query: the primitives (indices into leaf_boxes) whose box overlaps the query's; self_pairs: only indices above the
    query's own (len(boxes) must equal len(leaf_boxes))"""
    boxes, leaf_boxes = as_boxes(boxes), as_boxes(leaf_boxes)
    if self_pairs:
        assert len(boxes) == len(leaf_boxes)
    qi, bj = overlap_pairs(boxes, leaf_boxes)
    if self_pairs:
        keep = bj > qi
        qi, bj = qi[keep], bj[keep]
    order = np.lexsort((bj, qi))
    qi, bj = qi[order], bj[order]
    cuts = np.searchsorted(qi, np.arange(len(boxes) + 1))
    return [bj[cuts[i]:cuts[i + 1]].astype(np.uint32) for i in range(len(boxes))]


def csr_of(sets):
    """(offsets u32[m + 1], prims u32[total]) of a list of index arrays"""
    counts = np.array([len(s) for s in sets], dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    prims = np.concatenate(sets).astype(np.uint32) if len(sets) and offsets[-1] else np.zeros(0, dtype=np.uint32)
    return offsets, prims


def sorted_slices(offsets, prims):
    """prims with every slice sorted: the canonical form of an answer (the order inside a slice is unspecified)"""
    out = prims.copy()
    for i in range(len(offsets) - 1):
        out[offsets[i]:offsets[i + 1]].sort()
    return out


def leaf_boxes_of(nodes, leaves, n, layout):
    """the primitives' boxes as the tree holds them, indexed by primitive: layout 0 node n-1+j, layout 1 leaves[j]"""
    out = np.zeros(n, dtype=AABB)
    if layout == 0:
        rec = nodes[n - 1: 2 * n - 1]
        out["min"][rec["left"]] = rec["min"]; out["max"][rec["left"]] = rec["max"]
    else:
        out["min"][leaves["prim"]] = leaves["min"]; out["max"][leaves["prim"]] = leaves["max"]
    return out


# ---- the query mix ------------------------------------------------------------------------------------------------------------------------------------------

def make_boxes(leaf_boxes, seed, m=1536, points=None):
    """m random boxes — centres uniform in the scene box enlarged by half its extent, half-widths a random fraction of 2 % / 10 % / 50 % of the extent per axis,
    a third each — then 32 boxes equal to a primitive's own box, 32 that share exactly one plane with a primitive's box (max = that box's min on one axis), 32
    point boxes (on ``points``: vertices; default the primitive boxes' corners), the whole scene, a box far outside, ten inverted boxes (nine random boxes with
    min and max swapped on one axis, and the reset box) and eight boxes with one NaN coordinate.  Returns (boxes, kind): kind[i] = 0 / 1 / 2 for the three
    random sizes, 3 for everything else."""
    lb = as_boxes(leaf_boxes)
    rng = np.random.default_rng(seed)
    with np.errstate(invalid="ignore"):
        good = np.isfinite(lb["min"]).all(axis=1) & np.isfinite(lb["max"]).all(axis=1)
    lo = lb["min"][good].astype(np.float64).min(axis=0); hi = lb["max"][good].astype(np.float64).max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    frac = np.repeat(np.array([0.02, 0.10, 0.50]), (m + 2) // 3)[:m]
    kind = np.repeat(np.array([0, 1, 2]), (m + 2) // 3)[:m]
    c = lo - 0.5 * ext + rng.random((m, 3)) * 2.0 * ext
    h = rng.random((m, 3)) * frac[:, None] * ext
    rnd = np.concatenate([c - h, c + h], axis=1).astype(F32)
    n = len(lb)
    own = lb[rng.integers(0, n, size=32)]
    own = np.concatenate([own["min"], own["max"]], axis=1)
    src = lb[rng.integers(0, n, size=32)]
    plane = np.concatenate([src["min"], src["max"]], axis=1).astype(F32)
    ax = rng.integers(0, 3, size=32)
    rows = np.arange(32)
    plane[rows, 3 + ax] = src["min"][rows, ax]                                      # max = the box's min on that axis: they share exactly that plane
    plane[rows, ax] = (src["min"][rows, ax].astype(np.float64) - (0.01 + rng.random(32)) * ext[ax]).astype(F32)
    if points is None:
        points = np.concatenate([lb["min"], lb["max"]])
    p = np.asarray(points, dtype=F32).reshape(-1, 3)
    p = p[rng.integers(0, len(p), size=32)]
    pts = np.concatenate([p, p], axis=1)
    scene = np.concatenate([lo, hi])[None].astype(np.float64)
    scene[0, :3] = np.nextafter(scene[0, :3].astype(F32), F32(-np.inf)); scene[0, 3:] = np.nextafter(scene[0, 3:].astype(F32), F32(np.inf))
    far = np.concatenate([hi + 10.0 * ext, hi + 11.0 * ext])[None]
    inv = rnd[rng.integers(0, m, size=10)].copy()
    iax = rng.integers(0, 3, size=10)
    r10 = np.arange(10)
    inv[r10, iax], inv[r10, 3 + iax] = inv[r10, 3 + iax].copy(), inv[r10, iax].copy()
    flat = inv[r10, iax] == inv[r10, 3 + iax]
    inv[r10[flat], iax[flat]] = np.nextafter(inv[r10[flat], iax[flat]], F32(np.inf))   # (strictly inverted)
    fmax = np.finfo(F32).max
    inv[9] = (fmax, fmax, fmax, -fmax, -fmax, -fmax)                                 # Aabb::reset
    nan = rnd[rng.integers(0, m, size=8)].copy()
    nan[np.arange(8), rng.integers(0, 6, size=8)] = np.nan
    allb = np.concatenate([rnd, own, plane, pts, scene, far, inv, nan]).astype(F32)
    kinds = np.concatenate([kind, np.full(len(allb) - m, 3)])
    return as_boxes(allb), kinds


# ---- a numpy walk with the kernels' pruning -------------------------------------------------------------------------------------------------------------------

def tree_walk(boxes, nodes, leaves, root, n, layout):
    """per query the sorted primitives a walk reports that enters a child iff its box passes the overlap test (the root's own box is not tested, as in the
    kernels); all queries advance together, one tree level per round"""
    boxes = as_boxes(boxes)
    ni = n - 1
    if layout == 0:
        rec_lo, rec_hi, left, right = nodes["min"], nodes["max"], nodes["left"], nodes["right"]
        leaf_prim = nodes["left"][ni:]
    else:
        rec_lo = np.concatenate([nodes["min"][:ni], leaves["min"]]); rec_hi = np.concatenate([nodes["max"][:ni], leaves["max"]])
        left, right = nodes["left"], nodes["right"]
        leaf_prim = leaves["prim"]
    qlo, qhi = boxes["min"], boxes["max"]
    with np.errstate(invalid="ignore"):
        live = np.nonzero((qlo <= qhi).all(axis=1))[0]
    fq, fn = live, np.full(len(live), root, dtype=np.int64)
    out_q, out_p = [], []
    rounds = 0
    while len(fq):
        rounds += 1
        assert rounds <= 2 * n, "not a tree"
        cq = np.concatenate([fq, fq]); cn = np.concatenate([left[fn], right[fn]]).astype(np.int64)
        with np.errstate(invalid="ignore"):
            ok = ((qlo[cq] <= rec_hi[cn]) & (rec_lo[cn] <= qhi[cq]) & (rec_lo[cn] <= rec_hi[cn])).all(axis=1)
        cq, cn = cq[ok], cn[ok]
        leaf = cn >= ni
        out_q.append(cq[leaf]); out_p.append(leaf_prim[cn[leaf] - ni])
        fq, fn = cq[~leaf], cn[~leaf]
    qi = np.concatenate(out_q) if out_q else np.zeros(0, dtype=np.int64)
    pj = np.concatenate(out_p).astype(np.int64) if out_p else np.zeros(0, dtype=np.int64)
    order = np.lexsort((pj, qi))
    qi, pj = qi[order], pj[order]
    cuts = np.searchsorted(qi, np.arange(len(boxes) + 1))
    return [pj[cuts[i]:cuts[i + 1]].astype(np.uint32) for i in range(len(boxes))]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_overlap_and_its_enum(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    assert re.search(r"typedef enum\s*\{\s*BVH_OVERLAP_BOXES\s*=\s*0\s*,\s*BVH_OVERLAP_SELF\s*=\s*1\s*\}\s*bvh_overlap_mode\s*;", text)
    assert re.search(r"\bint\s+bvh_overlap\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*const bvh_result\s*\*\s*\w+\s*,\s*const bvh_aabb\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*"
                     r"int\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text


def test_library_exports_overlap(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_overlap") and "bvh_overlap" in pkg.EXPORTS
    assert (pkg.OVERLAP_BOXES, pkg.OVERLAP_SELF) == (0, 1)
    f = pkg.lib().bvh_overlap
    assert len(f.argtypes) == 9 and f.argtypes[7] is C.c_uint64 and f.restype is C.c_int
    assert pkg.lib().bvh_abi_version() == 4 and pkg.ABI_VERSION == 4
    assert pkg.AABB == AABB


def test_overlap_errors_without_a_device(pkg):
    lib = pkg.lib()
    total = C.c_uint64(77)
    assert lib.bvh_overlap(None, None, None, 0, 0, None, None, 0, None) == E_INVALID
    r = pkg.Result(); r.n_leaves = 4; r.layout = 0; r.d_nodes = 64
    assert lib.bvh_overlap(None, C.byref(r), 256, 4, 0, 4096, 8192, 16, C.byref(total)) == E_INVALID          # NULL ctx
    assert lib.bvh_overlap(None, None, 256, 4, 0, 4096, 8192, 16, C.byref(total)) == E_INVALID                # NULL ctx and tree
    assert total.value == 77


def test_builder_classes_have_overlap(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "overlap"))
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().overlap(np.zeros(4, dtype=pkg.AABB))         # no tree yet


def test_cpp_mirror_overlap_compiles(tmp_path):
    src = tmp_path / "overlap_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> uint64_t ask(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_aabb* q, uint32_t n, uint32_t* off, uint32_t* prims,
                                   uint64_t cap) {
    B bvh; bvh.build(ctx, a);
    bvh.overlapAsync(ctx, q, n, BVH_OVERLAP_BOXES, off, nullptr, 0);
    return bvh.overlap(ctx, q, n, BVH_OVERLAP_BOXES, off, prims, cap) + bvh.overlap(ctx, q, n, BVH_OVERLAP_SELF, off, prims, cap);
}
uint64_t all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_aabb* q, uint32_t n, uint32_t* off, uint32_t* prims, uint64_t cap) {
    return ask<BvhConstruction::TwoPassLbvh>(ctx, a, q, n, off, prims, cap) + ask<BvhConstruction::SinglePassLbvh>(ctx, a, q, n, off, prims, cap) +
           ask<BvhConstruction::PLOCNew>(ctx, a, q, n, off, prims, cap) + ask<BvhConstruction::HPLOC>(ctx, a, q, n, off, prims, cap);
}
static_assert(BVH_OVERLAP_BOXES == 0 && BVH_OVERLAP_SELF == 1 && sizeof(bvh_aabb) == 24, "enum / sizes");
""")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the brute force on hand-made cases -----------------------------------------------------------------------------------------------------------------------

UNIT = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)


def one(q, b):
    return len(overlap_brute_force(np.array([q], dtype=F32), np.array([b], dtype=F32))[0]) == 1


def test_touching_faces_edges_and_corners_overlap():
    assert one((1.0, 0.25, 0.25, 2.0, 0.75, 0.75), UNIT)             # a shared face plane
    assert one((1.0, 1.0, 0.25, 2.0, 2.0, 0.75), UNIT)               # an edge
    assert one((1.0, 1.0, 1.0, 2.0, 2.0, 2.0), UNIT)                 # a corner
    assert one((-1.0, -1.0, -1.0, 0.0, 0.0, 0.0), UNIT)              # the opposite corner
    assert one(UNIT, UNIT)
    assert not one((1.5, 0.0, 0.0, 2.0, 1.0, 1.0), UNIT)


def test_a_gap_of_one_ulp_does_not_overlap():
    up = float(np.nextafter(F32(1.0), F32(2.0))); down = float(np.nextafter(F32(0.0), F32(-1.0)))
    for k in range(3):
        q = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
        q[k], q[3 + k] = up, 2.0
        assert not one(q, UNIT)                                       # just above the max plane
        q[k], q[3 + k] = 1.0, 2.0
        assert one(q, UNIT)
        q[k], q[3 + k] = -1.0, down
        assert not one(q, UNIT)                                       # just below the min plane (a denormal away from 0)
        q[k], q[3 + k] = -1.0, 0.0
        assert one(q, UNIT)


def test_nan_in_either_box_fails():
    for k in range(6):
        q = list((0.25, 0.25, 0.25, 0.75, 0.75, 0.75)); q[k] = np.nan
        assert not one(q, UNIT) and not one(UNIT, q)


def test_inverted_boxes_overlap_nothing():
    fmax = float(np.finfo(F32).max)
    reset = (fmax, fmax, fmax, -fmax, -fmax, -fmax)
    big = (-fmax, -fmax, -fmax, fmax, fmax, fmax)
    everything = (-np.inf, -np.inf, -np.inf, np.inf, np.inf, np.inf)
    for other in (UNIT, big, everything, reset):
        assert not one(reset, other) and not one(other, reset)
    for k in range(3):                                                # mildly inverted on one axis, inside the other box
        q = [0.25, 0.25, 0.25, 0.75, 0.75, 0.75]
        q[k], q[3 + k] = q[3 + k], q[k]
        assert not one(q, UNIT) and not one(UNIT, q) and not one(q, q)
    assert one(big, UNIT) and one(everything, big)


def test_negative_zero_equals_positive_zero():
    assert one((-1.0, -1.0, -1.0, -0.0, -0.0, -0.0), (0.0, 0.0, 0.0, 1.0, 1.0, 1.0))
    assert one((-1.0, -1.0, -1.0, 0.0, 0.0, 0.0), (-0.0, -0.0, -0.0, 1.0, 1.0, 1.0))
    assert one((0.0, 0.0, 0.0, -0.0, -0.0, -0.0), (-0.0, -0.0, -0.0, 0.0, 0.0, 0.0))       # min +0 above max -0 only as bit patterns: not inverted


def test_a_point_box_inside_another():
    p = (0.5, 0.5, 0.5, 0.5, 0.5, 0.5)
    assert one(p, UNIT) and one(UNIT, p) and one(p, p)
    assert one((1.0, 1.0, 1.0, 1.0, 1.0, 1.0), UNIT)                  # on the corner
    assert not one((1.5, 0.5, 0.5, 1.5, 0.5, 0.5), UNIT)


def test_brute_force_sets_self_pairs_and_csr():
    leaf = np.array([(0, 0, 0, 1, 1, 1), (0.5, 0.5, 0.5, 2, 2, 2), (3, 3, 3, 4, 4, 4), (1, 1, 1, 3, 3, 3)], dtype=F32)
    sets = overlap_brute_force(np.array([(0, 0, 0, 4, 4, 4), (2.5, 2.5, 2.5, 2.75, 2.75, 2.75), (9, 9, 9, 10, 10, 10)], dtype=F32), leaf)
    assert [s.tolist() for s in sets] == [[0, 1, 2, 3], [3], []]
    assert all(s.dtype == np.uint32 for s in sets)
    off, prims = csr_of(sets)
    assert off.tolist() == [0, 4, 5, 5] and prims.tolist() == [0, 1, 2, 3, 3]
    pairs = overlap_brute_force(leaf, leaf, self_pairs=True)
    assert [s.tolist() for s in pairs] == [[1, 3], [3], [3], []]      # {0,1}, {0,3} (a corner), {1,3}, {2,3} (a corner): each once, nothing with itself
    assert sorted_slices(np.array([0, 3, 5], dtype=np.uint32), np.array([9, 2, 4, 8, 1], dtype=np.uint32)).tolist() == [2, 4, 9, 1, 8]


def test_query_mix_has_every_kind(pkg):
    tris = mesh(pkg, "sponza_1000")
    lo = np.minimum(np.minimum(tris["v1"], tris["v2"]), tris["v3"]); hi = np.maximum(np.maximum(tris["v1"], tris["v2"]), tris["v3"])
    leaf = as_boxes(np.concatenate([lo, hi], axis=1))
    boxes, kind = make_boxes(leaf, 5, points=np.concatenate([tris["v1"], tris["v2"], tris["v3"]]))
    assert len(boxes) == 1536 + 32 * 3 + 2 + 10 + 8 and (np.bincount(kind) == [512, 512, 512, 116]).all()
    sets = overlap_brute_force(boxes, leaf)
    counts = np.array([len(s) for s in sets])
    assert (counts[:1536] == 0).any() and (counts[:1536] > 0).any()
    assert (counts[1536:1536 + 96] >= 1).all()                        # own boxes, plane-sharing boxes and vertex points all touch their source
    assert counts[1536 + 96] == len(tris) and counts[1536 + 97] == 0  # the whole scene, the far box
    assert (counts[-18:] == 0).all()                                  # inverted and NaN boxes
    again, _ = make_boxes(leaf, 5, points=np.concatenate([tris["v1"], tris["v2"], tris["v3"]]))
    assert again.tobytes() == boxes.tobytes()


# ---- the premise, on the CPU oracle ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PREMISE_MESHES)
def test_internal_boxes_are_the_bitwise_union_of_their_children(pkg, orc, name):
    tris = mesh(pkg, name); n = len(tris)
    for algo in (0, 1, 2, 3):
        t = orc.build_tree(algo, tris)
        nodes, leaves, layout = t["nodes"], t["leaves"], t["layout"]
        ni = n - 1
        if layout == 0:
            lo, hi = nodes["min"], nodes["max"]
        else:
            lo = np.concatenate([nodes["min"][:ni], leaves["min"]]); hi = np.concatenate([nodes["max"][:ni], leaves["max"]])
        l, r = nodes["left"][:ni].astype(np.int64), nodes["right"][:ni].astype(np.int64)
        assert l.max() < 2 * n - 1 and r.max() < 2 * n - 1
        ulo = np.minimum(lo[l], lo[r]); uhi = np.maximum(hi[l], hi[r])
        assert ulo.tobytes() == np.ascontiguousarray(lo[:ni]).tobytes() and uhi.tobytes() == np.ascontiguousarray(hi[:ni]).tobytes(), f"{name} algo {algo}"
        # and the leaf records hold the primitives' own boxes
        prim_boxes, _ = orc.prim_bounds(tris)
        assert leaf_boxes_of(nodes, leaves, n, layout).tobytes() == prim_boxes.tobytes()


@pytest.mark.parametrize("name", PREMISE_MESHES)
def test_pruned_walk_equals_brute_force_on_every_builder(pkg, orc, name):
    tris = mesh(pkg, name); n = len(tris)
    ref = None
    for algo in (0, 1, 2, 3):
        t = orc.build_tree(algo, tris)
        leaf = leaf_boxes_of(t["nodes"], t["leaves"], n, t["layout"])
        if ref is None:
            boxes, _ = make_boxes(leaf, 31 + n, points=np.concatenate([tris["v1"], tris["v2"], tris["v3"]]))
            ref = overlap_brute_force(boxes, leaf)
            if n >= 3:
                counts = np.array([len(s) for s in ref[:1536]])
                assert (counts == 0).any() and (counts > 0).any()
        got = tree_walk(boxes, t["nodes"], t["leaves"], t["root"], n, t["layout"])
        assert len(got) == len(ref)
        bad = [i for i in range(len(ref)) if got[i].tobytes() != ref[i].tobytes()]
        assert not bad, f"{name} algo {algo}: {len(bad)} queries differ (first {bad[:6]})"
