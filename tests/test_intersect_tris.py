"""CPU: bvh_intersect_tris in the C ABI, the library, the Python binding and the C++ mirror; the predicate of include/bvh_mi355x.h restated twice — crosses64
in numpy f64, operation for operation what the kernels evaluate, and crosses_exact in fractions.Fraction — with the rule cases checked in both; the brute force
(box test, then crosses64) that the GPU tests (tests/test_gpu_intersect_tris.py) compare against; and the premise that lets those tests compare whole sets:
crosses64 agrees with exact arithmetic on EVERY box-overlapping pair of this project's meshes and of two sets built to lie within f32 rounding of touching.
The determinants alone (determinants64) would report an edge of a zero-area triangle, or the clean edge of a triangle with a NaN elsewhere, that passes
through another triangle; the header's proper() keeps those out, and both counter-examples are kept here."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_gpu_refit import no_negzero
from test_overlap import as_boxes, csr_of, overlap_pairs

E_INVALID = -10001
F32 = np.float32
F64 = np.float64
FLT_MAX = F32(3.4028234663852886e38)
SHIFT = (0.37, 0.11, -0.23)             # the shifted copy: this fraction of the mesh's extent per axis
# (crossing pairs, box pairs) of every input, computed by tris_brute_force / overlap_pairs on the CPU (self: unordered pairs, j > i)
TOTALS = {
    ("uniform_1000", None): (548, 3245),
    ("cornell382", None): (15, 2222),
    ("cornell82", None): (14, 488),
    ("bunny_1280", None): (0, 7757),
    ("bunny_1280_shifted", "bunny_1280"): (197, 862),
}


# ---- meshes -------------------------------------------------------------------------------------------------------------------------------------------------

_MESHES = {}


def xyz(tris):
    """(n, 3, 3) f32: vertex, coordinate — from TRIANGLE records or any array of 9 floats per triangle"""
    if getattr(tris, "dtype", None) is not None and tris.dtype.names:
        return np.ascontiguousarray(np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1), dtype=F32)
    return np.ascontiguousarray(np.asarray(tris, dtype=F32).reshape(-1, 3, 3))


def as_triangles(pkg, v):
    """TRIANGLE records of an (n, 3, 3) array"""
    v = np.asarray(v, dtype=F32).reshape(-1, 3, 3)
    t = np.zeros(len(v), dtype=pkg.meshgen.TRIANGLE)
    t["v1"], t["v2"], t["v3"] = v[:, 0], v[:, 1], v[:, 2]
    return t


def shifted(pkg, tris):
    """the mesh moved by SHIFT times its extent, the sum rounded to f32"""
    v = xyz(tris)
    flat = v.reshape(-1, 3).astype(F64)
    d = (np.array(SHIFT) * (flat.max(axis=0) - flat.min(axis=0))).astype(F32)
    return no_negzero(as_triangles(pkg, (v + d[None, None, :]).astype(F32)))


def tt_mesh(pkg, name):
    """uniform_N: meshgen.uniform(N, seed 1); bunny_N: meshgen.bunny_like(N, seed 2); cornellN: the golden .tri file; NAME_shifted: shifted(NAME)"""
    if name not in _MESHES:
        if name.endswith("_shifted"):
            t = shifted(pkg, tt_mesh(pkg, name[: -len("_shifted")]))
        elif name.startswith("cornell"):
            t = pkg.meshgen.load_tri(os.path.join(GOLDEN, name + ".tri"))
        else:
            kind, n = name.split("_")
            t = pkg.meshgen.bunny_like(int(n), 2) if kind == "bunny" else pkg.meshgen.uniform(int(n), 1)
        _MESHES[name] = no_negzero(t)
    return _MESHES[name]


# ---- the predicate, twice -------------------------------------------------------------------------------------------------------------------------------------

def orient64(a, b, c, d):
    """orient(a, b, c, d) on (m, 3) f64 arrays, in the header's association: rows a - d, b - d, c - d, expansion along the first row, terms summed left to right"""
    ad, bd, cd = a - d, b - d, c - d
    return (ad[:, 0] * (bd[:, 1] * cd[:, 2] - bd[:, 2] * cd[:, 1]) + ad[:, 1] * (bd[:, 2] * cd[:, 0] - bd[:, 0] * cd[:, 2])) + ad[:, 2] * (bd[:, 0] * cd[:, 1] - bd[:, 1] * cd[:, 0])


def _edges64(x, y):
    """one of x's three edges crosses y: x, y (m, 3, 3) f64"""
    s = [orient64(y[:, 0], y[:, 1], y[:, 2], x[:, k]) for k in range(3)]           # each plane side once per vertex
    out = np.zeros(len(x), dtype=bool)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        p, q = x[:, i], x[:, j]
        straddle = ((s[i] > 0) & (s[j] < 0)) | ((s[i] < 0) & (s[j] > 0))
        o1, o2, o3 = orient64(p, q, y[:, 0], y[:, 1]), orient64(p, q, y[:, 1], y[:, 2]), orient64(p, q, y[:, 2], y[:, 0])
        out |= straddle & (((o1 > 0) & (o2 > 0) & (o3 > 0)) | ((o1 < 0) & (o2 < 0) & (o3 < 0)))
    return out


def proper64(t):
    """proper(T): no NaN coordinate, and a component of (v2 - v1) x (v3 - v1) that is > 0 or < 0.  t (m, 3, 3) f64"""
    u, w = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    n = (u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0])
    return ~np.isnan(t).any(axis=(1, 2)) & ((n[0] > 0) | (n[0] < 0) | (n[1] > 0) | (n[1] < 0) | (n[2] > 0) | (n[2] < 0))


def determinants64(x, y):
    """the determinant part of crosses64 alone, without proper(): what the header says is NOT enough"""
    x, y = xyz(x).astype(F64), xyz(y).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        return _edges64(x, y) | _edges64(y, x)


def crosses64(x, y):
    """crosses(X_k, Y_k) for k < m, the header's predicate in numpy: f32 coordinates widened exactly, IEEE f64 without contraction or reassociation (numpy
    evaluates every elementwise operation on its own), strict comparisons.  x, y: (m, 3, 3) arrays or TRIANGLE records"""
    x, y = xyz(x).astype(F64), xyz(y).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        return proper64(x) & proper64(y) & (_edges64(x, y) | _edges64(y, x))


SCALE = 2 ** 149                        # every finite f32 is an integer multiple of 2^-149: scaled coordinates are integers, and a sign does not see the scale


def exact_coords(t):
    """(3, 3) nested lists of Fractions of one triangle ((3, 3) f32), scaled by 2^149; None if a coordinate is not finite"""
    if not np.isfinite(t).all():
        return None
    return [[Fraction(float(v)) * SCALE for v in row] for row in t]


def orient_exact(a, b, c, d):
    ad = [a[k] - d[k] for k in range(3)]; bd = [b[k] - d[k] for k in range(3)]; cd = [c[k] - d[k] for k in range(3)]
    return ad[0] * (bd[1] * cd[2] - bd[2] * cd[1]) + ad[1] * (bd[2] * cd[0] - bd[0] * cd[2]) + ad[2] * (bd[0] * cd[1] - bd[1] * cd[0])


def _edges_exact(x, y):
    s = [orient_exact(y[0], y[1], y[2], x[k]) for k in range(3)]
    for i, j in ((0, 1), (1, 2), (2, 0)):
        if (s[i] > 0 and s[j] < 0) or (s[i] < 0 and s[j] > 0):
            o = (orient_exact(x[i], x[j], y[0], y[1]), orient_exact(x[i], x[j], y[1], y[2]), orient_exact(x[i], x[j], y[2], y[0]))
            if all(v > 0 for v in o) or all(v < 0 for v in o):
                return True
    return False


def proper_exact(t):
    u = [t[1][k] - t[0][k] for k in range(3)]; w = [t[2][k] - t[0][k] for k in range(3)]
    return any(v != 0 for v in (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]))


def crosses_exact(x, y):
    """the same predicate in exact rational arithmetic (fractions.Fraction), pair by pair: -> bool[m].  A triangle with a NaN or an infinity crosses nothing
    here (the header promises that for NaN; with infinities only crosses64 is the contract)"""
    x, y = xyz(x), xyz(y)
    out = np.zeros(len(x), dtype=bool)
    cache = {}

    def coords(arr, k):
        key = arr[k].tobytes()
        if key not in cache:
            cache[key] = exact_coords(arr[k])
        return cache[key]
    for k in range(len(x)):
        a, b = coords(x, k), coords(y, k)
        out[k] = a is not None and b is not None and proper_exact(a) and proper_exact(b) and (_edges_exact(a, b) or _edges_exact(b, a))
    return out


# ---- the brute force --------------------------------------------------------------------------------------------------------------------------------------------

def stage_e_boxes(tris):
    """stage E's boxes restated: fminf / fmaxf of the three vertices (a NaN operand is dropped), then clamped against the reset box, so an axis whose three
    coordinates are all NaN — or all +inf for the min, all -inf for the max — keeps +-FLT_MAX"""
    v = xyz(tris)
    lo = np.fmin(FLT_MAX, np.fmin(np.fmin(v[:, 0], v[:, 1]), v[:, 2]))
    hi = np.fmax(-FLT_MAX, np.fmax(np.fmax(v[:, 0], v[:, 1]), v[:, 2]))
    return as_boxes(np.concatenate([lo, hi], axis=1).astype(F32))


def box_pairs(a, b, self_pairs=False):
    """(i, j) of every pair whose stage-E boxes overlap (bvh_overlap's test); self_pairs: j > i only"""
    qi, bj = overlap_pairs(stage_e_boxes(a), stage_e_boxes(b))
    if self_pairs:
        keep = bj > qi
        qi, bj = qi[keep], bj[keep]
    return qi, bj


def tris_brute_force(a, b, self_pairs=False):
    """one sorted uint32 index array per triangle of ``a``: the triangles of ``b`` whose box overlaps its box and which it crosses (crosses64);
    self_pairs: a and b are the same mesh and only indices above the query's own are kept"""
    va, vb = xyz(a), xyz(b)
    if self_pairs:
        assert len(va) == len(vb)
    qi, bj = box_pairs(va, vb, self_pairs)
    keep = crosses64(va[qi], vb[bj]) if len(qi) else np.zeros(0, dtype=bool)
    qi, bj = qi[keep], bj[keep]
    order = np.lexsort((bj, qi))
    qi, bj = qi[order], bj[order]
    cuts = np.searchsorted(qi, np.arange(len(va) + 1))
    return [bj[cuts[i]:cuts[i + 1]].astype(np.uint32) for i in range(len(va))]


# ---- triangles within f32 rounding of touching ---------------------------------------------------------------------------------------------------------------

def near_degenerate(seed=20, m=1500):
    """(B, A_vertex, A_edge), each (m, 3, 3) f32.  B: random triangles in [-1, 1]^3.  A_vertex[k]: one vertex a point of B[k]'s interior rounded to f32 and then
    moved by -2 .. 2 ulps on one coordinate (within 2 ulps of the plane), the other two vertices on one side of the plane.  A_edge[k]: the edge (v1, v2) runs
    through a point of one of B[k]'s edges rounded to f32 — both end points rounded too, so the line passes that edge within f32 rounding — across the plane."""
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1.0, 1.0, (m, 3, 3)).astype(F32)
    b64 = b.astype(F64)
    nrm = np.cross(b64[:, 1] - b64[:, 0], b64[:, 2] - b64[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    # (a) a vertex on the plane, inside
    w = rng.uniform(0.15, 1.0, (m, 3)); w /= w.sum(axis=1, keepdims=True)
    p = np.einsum("mk,mkc->mc", w, b64).astype(F32)
    ax = rng.integers(0, 3, m); ulps = rng.integers(-2, 3, m)
    rows = np.arange(m)
    for step in (1, 2):
        move = np.abs(ulps) >= step
        p[rows[move], ax[move]] = np.nextafter(p[rows[move], ax[move]], np.where(ulps[move] > 0, F32(np.inf), F32(-np.inf)).astype(F32))
    side = np.where(rng.random(m) < 0.5, 1.0, -1.0)[:, None]
    a_vertex = np.empty((m, 3, 3), dtype=F32)
    a_vertex[:, 0] = p
    for k in (1, 2):
        a_vertex[:, k] = (p.astype(F64) + side * nrm * rng.uniform(0.05, 0.5, (m, 1)) + rng.uniform(-0.3, 0.3, (m, 3))).astype(F32)
    # (b) an edge through a point of one of B's edges
    e = rng.integers(0, 3, m)
    t = rng.uniform(0.1, 0.9, (m, 1))
    e0, e1 = b64[rows, e], b64[rows, (e + 1) % 3]
    on = (e0 + t * (e1 - e0)).astype(F32).astype(F64)
    d = nrm * rng.uniform(0.5, 1.0, (m, 1)) + rng.uniform(-0.4, 0.4, (m, 3))
    a_edge = np.empty((m, 3, 3), dtype=F32)
    a_edge[:, 0] = (on - d * rng.uniform(0.1, 0.6, (m, 1))).astype(F32)
    a_edge[:, 1] = (on + d * rng.uniform(0.1, 0.6, (m, 1))).astype(F32)
    a_edge[:, 2] = (on + rng.uniform(-0.5, 0.5, (m, 3)) + nrm * rng.uniform(-0.5, 0.5, (m, 1))).astype(F32)
    return b, a_vertex, a_edge


def crosses32(x, y):
    """the predicate evaluated in f32 instead — what the device does NOT do; only for the record below"""
    x, y = xyz(x), xyz(y)
    with np.errstate(invalid="ignore", over="ignore"):
        return proper64(x) & proper64(y) & (_edges64(x, y) | _edges64(y, x))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_intersect_tris_and_its_enum(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    assert re.search(r"typedef enum\s*\{\s*BVH_TRIS_QUERY\s*=\s*0\s*,\s*BVH_TRIS_SELF\s*=\s*1\s*\}\s*bvh_tris_mode\s*;", text)
    assert re.search(r"\bint\s+bvh_intersect_tris\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*const bvh_result\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,\s*"
                     r"const bvh_build_input\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*int\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*,\s*"
                     r"uint64_t\s*\*\s*\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text


def test_library_exports_intersect_tris(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_intersect_tris") and "bvh_intersect_tris" in pkg.EXPORTS
    assert (pkg.TRIS_QUERY, pkg.TRIS_SELF) == (0, 1)
    f = pkg.lib().bvh_intersect_tris
    assert len(f.argtypes) == 10 and f.argtypes[8] is C.c_uint64 and f.restype is C.c_int


def test_intersect_tris_errors_without_a_device(pkg):
    lib = pkg.lib()
    total = C.c_uint64(77)
    assert lib.bvh_intersect_tris(None, None, None, None, 0, 0, None, None, 0, None) == E_INVALID
    r = pkg.Result(); r.n_leaves = 4; r.layout = 0; r.d_nodes = 64; r.d_tris = 1 << 20
    q = pkg.BuildInput(pkg.TRI_PADDED64, 30, 1 << 21, None, None, 0, 0)
    assert lib.bvh_intersect_tris(None, C.byref(r), None, C.byref(q), 4, 0, 4096, 8192, 16, C.byref(total)) == E_INVALID        # NULL ctx
    assert lib.bvh_intersect_tris(None, None, None, C.byref(q), 4, 0, 4096, 8192, 16, C.byref(total)) == E_INVALID             # NULL ctx and tree
    assert lib.bvh_intersect_tris(None, C.byref(r), None, None, 4, 1, 4096, 8192, 16, C.byref(total)) == E_INVALID             # self mode, NULL ctx
    assert total.value == 77


def test_builder_classes_have_intersect_tris(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "intersect_tris"))
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().intersect_tris(np.zeros(4, dtype=pkg.meshgen.TRIANGLE))         # no tree yet


def test_self_pairs_is_refused_on_a_split_tree(pkg):
    """BVH_TRIS_SELF fetches triangle i for every i < n_leaves; a build_split tree has more leaves (references) than triangles, so the binding must refuse
    before any call is made — here without a device: the context is never touched"""
    b = pkg.HPLOC()
    b._ctx = object()                                                 # (anything but None: "a tree was built")
    b.result.n_leaves = 12
    b._split = {"tris": 1 << 20, "n_tris": 8}
    try:
        with pytest.raises(pkg.BvhError, match="build_split"):
            b.intersect_tris(self_pairs=True)
    finally:
        b._ctx = None; b._split = None
    text = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    assert "tris must hold n_leaves triangles" in text and "NOT usable on a tree with more leaves than" in text


def test_cpp_mirror_intersect_tris_compiles(tmp_path):
    src = tmp_path / "intersect_tris_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> uint64_t ask(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_build_input* q, uint32_t n, uint32_t* off,
                                   uint32_t* prims, uint64_t cap) {
    B bvh; bvh.build(ctx, a);
    bvh.intersectTrisAsync(ctx, q, n, BVH_TRIS_QUERY, off, nullptr, 0);
    return bvh.intersectTris(ctx, q, n, BVH_TRIS_QUERY, off, prims, cap) + bvh.intersectTris(ctx, nullptr, (uint32_t)a.size(), BVH_TRIS_SELF, off, prims, cap);
}
uint64_t all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_build_input* q, uint32_t n, uint32_t* off, uint32_t* prims, uint64_t cap) {
    return ask<BvhConstruction::TwoPassLbvh>(ctx, a, q, n, off, prims, cap) + ask<BvhConstruction::SinglePassLbvh>(ctx, a, q, n, off, prims, cap) +
           ask<BvhConstruction::PLOCNew>(ctx, a, q, n, off, prims, cap) + ask<BvhConstruction::HPLOC>(ctx, a, q, n, off, prims, cap);
}
static_assert(BVH_TRIS_QUERY == 0 && BVH_TRIS_SELF == 1, "enum");
""")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the rules, in both restatements ----------------------------------------------------------------------------------------------------------------------------

def both(x, y):
    """crosses(x, y) of one pair of (3, 3) triangles, checked to be the same in f64 and exactly, and symmetric in both"""
    x, y = np.asarray(x, dtype=F32).reshape(1, 3, 3), np.asarray(y, dtype=F32).reshape(1, 3, 3)
    r64, rex = bool(crosses64(x, y)[0]), bool(crosses_exact(x, y)[0])
    assert r64 == rex, (x, y, r64, rex)
    assert bool(crosses64(y, x)[0]) == r64 and bool(crosses_exact(y, x)[0]) == rex
    return r64


FLOOR = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]                             # in the plane z = 0


NAN = float("nan")
WING = [(0, 0, 0), (4, 0, 0), (1, 3, 0)]                              # hinged on FLOOR's edge (0,0,0)-(4,0,0) and folded flat onto it
# (label, X, Y, crosses(X, Y)): the rules as single pairs; the GPU test runs them as tiny meshes
RULE_CASES = [
    ("an edge through the interior", FLOOR, [(1, 1, -1), (1, 1, 1), (3, 3, 1)], True),
    ("above", FLOOR, [(1, 1, 1), (1, 2, 1), (2, 1, 2)], False),
    ("through the plane, outside", FLOOR, [(5, 5, -1), (5, 5, 1), (6, 5, 1)], False),
    ("a vertex in the plane, inside", FLOOR, [(1, 1, 0), (1, 1, 1), (2, 1, 1)], False),
    ("a vertex on the boundary", FLOOR, [(2, 0, 0), (2, 0, 1), (3, -1, 1)], False),
    ("an edge through a boundary edge", FLOOR, [(2, 0, -1), (2, 0, 1), (2, -3, 0)], False),
    ("an edge in the plane, inside", FLOOR, [(1, 1, 0), (2, 1, 0), (1, 1, 1)], False),
    ("coplanar, overlapping", FLOOR, [(1, 1, 0), (3, 1, 0), (1, 3, 0)], False),
    ("coplanar, edges crossing", FLOOR, [(-1, 1, 0), (5, 1, 0), (1, -2, 0)], False),
    ("identical", FLOOR, FLOOR, False),
    ("identical, rotated", FLOOR, [FLOOR[1], FLOOR[2], FLOOR[0]], False),
    ("zero area: a segment through the interior", FLOOR, [(1, 1, -1), (1, 1, 1), (1, 1, 1)], False),
    ("zero area: collinear through the interior", FLOOR, [(1, 1, -1), (1, 1, 0), (1, 1, 1)], False),
    ("zero area: a point", FLOOR, [(1, 1, 0), (1, 1, 0), (1, 1, 0)], False),
    ("a shared vertex, no penetration", FLOOR, [(0, 0, 0), (1, 1, 1), (2, 1, 1)], False),
    ("a shared vertex, the opposite edge outside", FLOOR, [(0, 0, 0), (-1, -1, 1), (-1, -2, -1)], False),
    ("a shared vertex, the opposite edge through the interior", FLOOR, [(0, 0, 0), (1, 1, 1), (1, 1, -1)], True),
    ("a shared edge, folded flat", FLOOR, WING, False),
    ("a shared edge, 90 degrees", FLOOR, [(0, 0, 0), (4, 0, 0), (1, 0, 3)], False),
    ("a shared edge, 30 degrees", FLOOR, [(4, 0, 0), (0, 0, 0), (1, 2.5, 1.5)], False),
    ("a shared edge, opened flat", FLOOR, [(0, 0, 0), (4, 0, 0), (1, -3, 0)], False),
    ("a NaN in the crossing vertex", FLOOR, [(1, NAN, -1), (1, 1, 1), (3, 3, 1)], False),
    ("a NaN in the other vertex", FLOOR, [(1, 1, -1), (1, 1, 1), (NAN, 3, 1)], False),
    ("a NaN in the crossed triangle", [(0, 0, 0), (4, 0, NAN), (0, 4, 0)], [(1, 1, -1), (1, 1, 1), (3, 3, 1)], False),
]


@pytest.mark.parametrize("label,x,y,expected", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_rule_case(label, x, y, expected):
    assert both(x, y) == expected


def test_a_proper_crossing_is_reported():
    assert both(FLOOR, [(1, 1, -1), (1, 1, 1), (3, 3, 1)])            # one edge through the interior
    assert both(FLOOR, [(1, 1, -1), (1.5, 1, 1), (1, 1.5, 1)])        # two edges through the interior
    assert not both(FLOOR, [(1, 1, 1), (1, 2, 1), (2, 1, 2)])         # above
    assert not both(FLOOR, [(5, 5, -1), (5, 5, 1), (6, 5, 1)])        # through the plane, outside the triangle


def test_a_vertex_exactly_in_an_axis_aligned_plane_is_not_a_crossing():
    assert not both(FLOOR, [(1, 1, 0), (1, 1, 1), (2, 1, 1)])         # touches the interior from above
    assert both(FLOOR, [(1, 1, 0), (0.5, 1, 1), (2.5, 1, -1)])        # ... with the other two on opposite sides the far edge passes through the interior,
    assert both(FLOOR, [(1, 1, 0), (1, 1, 1), (9, 1, -1)])            # ... or outside, at (5, 1, 0): then FLOOR's edge (4,0,0)-(0,4,0) passes through the other at (3, 1, 0)
    assert not both(FLOOR, [(1, 1, 0), (1, 1, -1), (2, 1, -2)])       # from below
    assert not both(FLOOR, [(1, 1, 0), (2, 1, 0), (1, 1, 1)])         # a whole edge in the plane, inside
    assert not both(FLOOR, [(2, 0, 0), (2, 0, 1), (3, -1, 1)])        # a vertex on the boundary
    assert not both(FLOOR, [(2, 0, -1), (2, 0, 1), (2, -3, 0)])       # an edge through the boundary edge


def test_coplanar_overlap_is_not_a_crossing():
    assert not both(FLOOR, [(1, 1, 0), (3, 1, 0), (1, 3, 0)])
    assert not both(FLOOR, [(-1, 1, 0), (5, 1, 0), (1, -2, 0)])       # edges cross edges, all in one plane
    tilted = [(0, 0, 0), (4, 0, 4), (0, 4, 4)]
    assert not both(tilted, [(1, 1, 2), (2, 1, 3), (1, 2, 3)])        # coplanar in the plane z = x + y


def test_identical_and_zero_area_triangles_are_not_a_crossing():
    assert not both(FLOOR, FLOOR)
    assert not both(FLOOR, [FLOOR[1], FLOOR[2], FLOOR[0]])
    assert not both(FLOOR, [(1, 1, -1), (1, 1, 1), (1, 1, 1)])        # a segment through the interior, as a zero-area triangle
    assert not both(FLOOR, [(1, 1, -1), (1, 1, 0), (1, 1, 1)])        # three collinear points through the interior
    assert not both(FLOOR, [(1, 1, 0), (1, 1, 0), (1, 1, 0)])
    # the determinants alone report the first two: the edge (1,1,-1)-(1,1,1) is a segment through FLOOR's interior whatever the third vertex is
    for seg in ([(1, 1, -1), (1, 1, 1), (1, 1, 1)], [(1, 1, -1), (1, 1, 0), (1, 1, 1)]):
        assert determinants64(np.array([FLOOR], dtype=F32), np.array([seg], dtype=F32))[0]


def test_a_shared_vertex():
    apex = (0, 0, 0)
    assert not both(FLOOR, [apex, (1, 1, 1), (2, 1, 1)])              # shared vertex, the rest above
    assert not both(FLOOR, [apex, (-1, -1, 1), (-1, -2, -1)])         # shared vertex, the opposite edge crosses the plane outside
    assert both(FLOOR, [apex, (1, 1, 1), (1, 1, -1)])                 # the edge opposite the shared vertex passes through the interior: reported
    assert both(FLOOR, [apex, (2, 1, 1), (1, 2, -1)])


def test_a_shared_edge_is_never_reported():
    for deg in (0, 1e-3, 30, 90, 150, 179.999, 180, 181, 270, 359.9):
        a = np.deg2rad(deg)
        wing = [FLOOR[0], FLOOR[1], (1.0, 3.0 * np.cos(a), 3.0 * np.sin(a))]         # hinged on the edge (0,0,0)-(4,0,0); 0 degrees: folded flat onto FLOOR
        assert not both(FLOOR, wing), deg
        assert not both(FLOOR, [wing[1], wing[0], wing[2]]), deg
    rng = np.random.default_rng(3)
    for _ in range(200):                                               # random hinges in general position
        p = rng.uniform(-1, 1, (4, 3)).astype(F32)
        assert not both(p[[0, 1, 2]], p[[1, 0, 3]]) and not both(p[[0, 1, 2]], p[[3, 0, 1]])


def test_nan_in_either_triangle_is_not_a_crossing():
    y = np.array([(1, 1, -1), (1, 1, 1), (3, 3, 1)], dtype=F32)
    assert both(FLOOR, y)
    for v in range(3):
        for k in range(3):
            bad = y.copy(); bad[v, k] = np.nan
            assert not both(FLOOR, bad) and not both(bad, FLOOR)
            bad = np.array(FLOOR, dtype=F32); bad[v, k] = np.nan
            assert not both(bad, y)
    bad = y.copy(); bad[2, 0] = np.nan                                 # the determinants alone report this one: the edge (v1, v2) holds no NaN
    assert determinants64(np.array([FLOOR], dtype=F32), bad[None])[0] and not both(FLOOR, bad)


def test_symmetry_on_random_pairs():
    rng = np.random.default_rng(8)
    x = rng.uniform(-1, 1, (4000, 3, 3)).astype(F32); y = rng.uniform(-1, 1, (4000, 3, 3)).astype(F32)
    r = crosses64(x, y)
    assert 0.05 < r.mean() < 0.6 and (crosses64(y, x) == r).all()
    assert (crosses64(x[:, [1, 2, 0]], y) == r).all() and (crosses64(x, y[:, [2, 0, 1]]) == r).all()
    assert (crosses_exact(x[:300], y[:300]) == r[:300]).all() and (crosses_exact(y[:300], x[:300]) == r[:300]).all()


def test_brute_force_sets_and_self_pairs(pkg):
    a = np.array([FLOOR, [(1, 1, -1), (1, 1, 1), (3, 3, 1)], [(10, 10, 10), (11, 10, 10), (10, 11, 10)], [(0.5, 0.5, -2), (0.5, 0.5, 2), (0.6, 3, 2)]], dtype=F32)
    sets = tris_brute_force(a, a)
    assert [s.tolist() for s in sets] == [[1, 3], [0], [], [0]] and all(s.dtype == np.uint32 for s in sets)
    assert [s.tolist() for s in tris_brute_force(a, a, self_pairs=True)] == [[1, 3], [], [], []]
    assert [s.tolist() for s in tris_brute_force(as_triangles(pkg, a), a[:1])] == [[], [0], [], [0]]
    off, prims = csr_of(sets)
    assert off.tolist() == [0, 2, 3, 3, 4] and prims.tolist() == [1, 3, 0, 0]
    nan = a.copy(); nan[1, 0, 0] = np.nan; nan[3] = np.inf
    assert [s.tolist() for s in tris_brute_force(nan, a)] == [[1, 3], [], [], []]
    bx = stage_e_boxes(nan)
    assert bx["min"][1].tolist() == [1, 1, -1] and bx["min"][3].tolist() == [FLT_MAX] * 3 and bx["max"][3].tolist() == [np.inf] * 3


# ---- the premise: f64 agrees with exact arithmetic on every box-overlapping pair ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,tree", list(TOTALS))
def test_f64_agrees_with_exact_arithmetic_on_every_box_pair(pkg, name, tree):
    a = tt_mesh(pkg, name)
    b = a if tree is None else tt_mesh(pkg, tree)
    va, vb = xyz(a), xyz(b)
    qi, bj = box_pairs(va, vb, self_pairs=tree is None)
    r64 = crosses64(va[qi], vb[bj])
    shared = (va[qi][:, :, None, :] == vb[bj][:, None, :, :]).all(axis=3).any(axis=(1, 2))
    print(f"{name}: {int(r64.sum())} crossing pairs of {len(qi)} box pairs; {int(shared.sum())} pairs share a vertex, {int((r64 & shared).sum())} of them cross")
    assert (int(r64.sum()), len(qi)) == TOTALS[(name, tree)]
    rex = crosses_exact(va[qi], vb[bj])
    assert int((r64 != rex).sum()) == 0
    assert sum(len(s) for s in tris_brute_force(a, b, self_pairs=tree is None)) == TOTALS[(name, tree)][0]


def test_f64_agrees_with_exact_arithmetic_within_rounding_of_touching():
    b, a_vertex, a_edge = near_degenerate()
    again = near_degenerate()
    assert all(u.tobytes() == v.tobytes() for u, v in zip((b, a_vertex, a_edge), again))
    for label, a in (("vertex", a_vertex), ("edge", a_edge)):
        rex = crosses_exact(a, b)
        r64, r32 = crosses64(a, b), crosses32(a, b)
        print(f"near-degenerate {label}: {int(rex.sum())} of {len(b)} cross exactly; f64 agrees on {int((r64 == rex).sum())}, f32 would get {int((r32 != rex).sum())} wrong")
        assert 0.2 < rex.mean() < 0.8                                 # the sets sit ON the decision: both answers occur
        assert int((r64 == rex).sum()) == len(b)
        assert (r32 != rex).any()                                     # and f32 is not enough for them
