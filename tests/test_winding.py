"""CPU: bvh_winding_prepare / bvh_winding_number in the C ABI, the library and the Python binding, and the numpy restatements that the GPU tests
(tests/test_gpu_winding.py) compare against: the f64 brute force (winding_brute_force), the per-node moments operation for operation in f32 (moments_host) and
the hierarchical walk with its opening decision in f32 and its terms and sum in a chosen precision (walk_host) — each checked here on the CPU oracle's trees."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_point_query import E_INVALID, tri_arrays

F32 = np.float32
FOURPI32 = F32(4.0 * np.pi)
THIRD32 = F32(1.0) / F32(3.0)
WIND_NAN_BITS = 0x7FC00000


def _comps(x, dtype):
    x = np.asarray(x).astype(dtype)
    return [x[..., k] for k in range(3)]


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _cross(x, y):
    return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]


def leaf_terms(q, v1, v2, v3, dtype):
    """the Van Oosterom–Strackee solid angle over 4 pi, in ``dtype``, in the header's operation order; arguments broadcast over a trailing axis of 3"""
    with np.errstate(all="ignore"):
        Q, A, B, Cc = (_comps(x, dtype) for x in (q, v1, v2, v3))
        a = [A[k] - Q[k] for k in range(3)]; b = [B[k] - Q[k] for k in range(3)]; c = [Cc[k] - Q[k] for k in range(3)]
        num = _dot(a, _cross(b, c))
        la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
        den = (((la * lb) * lc + _dot(a, b) * lc) + _dot(b, c) * la) + _dot(c, a) * lb
        fourpi = FOURPI32 if dtype == F32 else dtype(4.0 * np.pi)
        return ((dtype(2.0) * np.arctan2(num, den)) / fourpi).astype(dtype)


def leaf_sum(pts, v1, v2, v3, dtype, chunk_elems=1 << 21):
    """per point, the sum of leaf_terms over all the given triangles, terms and sum in ``dtype``"""
    pts = np.asarray(pts, dtype=F32)
    m, n = len(pts), len(v1)
    out = np.zeros(m, dtype=dtype)
    step = max(1, chunk_elems // max(n, 1))
    for s in range(0, m, step):
        out[s:s + step] = leaf_terms(pts[s:s + step, None, :], v1[None], v2[None], v3[None], dtype).sum(axis=1, dtype=dtype)
    return out


def winding_brute_force(tris, pts):
    """the generalized winding number of every point: the f64 sum of the triangles' solid angles over 4 pi (NaN for a point with a NaN coordinate)"""
    v1, v2, v3 = tri_arrays(tris)
    return leaf_sum(pts, v1, v2, v3, np.float64)


def tree_arrays(nodes, leaves, layout):
    """(n, ni, leaf_prims u32[n]) of a tree in either layout: internal nodes [0, ni), leaf j at ni + j"""
    if layout == 0:
        n = (len(nodes) + 1) // 2
        return n, n - 1, nodes["left"][n - 1:].astype(np.int64)
    n = len(leaves)
    return n, n - 1, leaves["prim"].astype(np.int64)


def moments_host(pkg, nodes, leaves, layout, root, tris):
    """bvh_winding_prepare's records in f32, operation for operation: leaf values from the triangles, internal sums left + right bottom-up, then p and r"""
    n, ni, prims = tree_arrays(nodes, leaves, layout)
    total = 2 * n - 1
    v1, v2, v3 = tri_arrays(tris)
    S = np.zeros((total, 7), dtype=F32)
    with np.errstate(all="ignore"):
        ok = prims < len(tris)
        pr = np.where(ok, prims, 0)
        a, b, c = _comps(v1[pr], F32), _comps(v2[pr], F32), _comps(v3[pr], F32)
        x = _cross([b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)])
        A = [F32(0.5) * x[k] for k in range(3)]
        area = np.sqrt((A[0] * A[0] + A[1] * A[1]) + A[2] * A[2])
        cen = [((a[k] + b[k]) + c[k]) * THIRD32 for k in range(3)]
        leaf = np.stack(A + [area] + [area * cen[k] for k in range(3)], axis=1).astype(F32)
        S[ni:] = np.where(ok[:, None], leaf, F32(0.0))
        left, right = nodes["left"][:ni].astype(np.int64), nodes["right"][:ni].astype(np.int64)
        order, stack = [], [int(root)]
        while stack:                                                # pre-order over the internal nodes; reversed: children before parents
            v = stack.pop()
            order.append(v)
            for ch in (int(left[v]), int(right[v])):
                if ch < ni:
                    stack.append(ch)
        for v in reversed(order):
            S[v] = S[left[v]] + S[right[v]]
        lo, hi = nodes["min"][:ni].astype(F32), nodes["max"][:ni].astype(F32)
        area = S[:ni, 3]
        good = (area != 0) & np.isfinite(area)
        p = np.where(good[:, None], S[:ni, 4:7] / area[:, None], (lo + hi) * F32(0.5)).astype(F32)
        e = np.fmax(np.abs(lo - p), np.abs(hi - p))
        r = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    out = np.zeros(ni, dtype=pkg.WINDING_MOMENT)
    out["a"] = S[:ni, 0:3]; out["area"] = S[:ni, 3]; out["p"] = p; out["r"] = r
    return out


_INF_MEMO = {}


def walk_host(nodes, leaves, layout, root, tris, moments, pts, beta, dtype, stats=None):
    """bvh_winding_number restated: left child first, the opening decision always in f32 (d = p - q, d2, t = beta * r, approximated iff d2 > t * t), the terms and
    the sum in ``dtype``.  All (point, node) pairs of one tree level are expanded together.  beta = +inf opens every node (the comparison is never true), so the
    answer is the plain sum over the tree's leaves: that case is summed directly, in primitive order, and memoised per (points, triangles, leaf set, dtype).
    stats (a dict): 'terms' = the mean number of terms per live point."""
    n, ni, prims = tree_arrays(nodes, leaves, layout)
    total = 2 * n - 1
    v1, v2, v3 = tri_arrays(tris)
    pts = np.ascontiguousarray(pts, dtype=F32)
    m = len(pts)
    live = ~np.isnan(pts).any(axis=1)
    acc = np.zeros(m, dtype=dtype)
    beta = F32(beta)
    if np.isinf(beta):
        use = np.sort(prims[prims < len(tris)])
        key = hashlib.sha1(pts.tobytes() + v1.tobytes() + v2.tobytes() + v3.tobytes() + use.tobytes() + np.dtype(dtype).str.encode()).hexdigest()
        if key not in _INF_MEMO:
            _INF_MEMO[key] = leaf_sum(pts, v1[use], v2[use], v3[use], dtype)
        acc = _INF_MEMO[key].copy()
        if stats is not None:
            stats["terms"] = float(len(use))
    else:
        left, right = nodes["left"][:ni].astype(np.int64), nodes["right"][:ni].astype(np.int64)
        A, P, R = moments["a"].astype(F32), moments["p"].astype(F32), moments["r"].astype(F32)
        fourpi = FOURPI32 if dtype == F32 else dtype(4.0 * np.pi)
        pi = np.nonzero(live)[0]; nd = np.full(len(pi), int(root), dtype=np.int64)
        n_terms = 0
        with np.errstate(all="ignore"):
            while len(pi):
                nxt_p, nxt_n = [], []
                for side in (left, right):
                    ch = side[nd]
                    lf = (ch >= ni) & (ch < total)
                    pr = prims[ch[lf] - ni]
                    inr = pr < len(tris)
                    if inr.any():
                        sel = pi[lf][inr]; pr = pr[inr]
                        np.add.at(acc, sel, leaf_terms(pts[sel], v1[pr], v2[pr], v3[pr], dtype)); n_terms += len(sel)
                    it = ch < ni
                    c, qi = ch[it], pi[it]
                    d = P[c] - pts[qi]                                # f32: the decision
                    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                    t = beta * R[c]
                    far = d2 > t * t
                    if far.any():
                        cf, qf = c[far], qi[far]
                        dd = _comps(P[cf].astype(dtype) - pts[qf].astype(dtype), dtype)
                        dd2 = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]
                        term = _dot(_comps(A[cf], dtype), dd) / ((fourpi * dd2) * np.sqrt(dd2))
                        np.add.at(acc, qf, term.astype(dtype)); n_terms += len(qf)
                    nxt_p.append(qi[~far]); nxt_n.append(c[~far])
                pi, nd = np.concatenate(nxt_p), np.concatenate(nxt_n)
        if stats is not None:
            stats["terms"] = n_terms / max(int(live.sum()), 1)
    acc[~live] = np.nan
    return acc


def stack_depth_all_open(nodes, root, ni):
    """the deepest short stack of k_winding when every internal child is opened (beta = +inf): at a node with two internal children the left is entered and the
    right pushed, so the depth at a node is the number of such ancestors whose LEFT subtree holds it"""
    best, work = 0, [(int(root), 0)]
    while work:
        v, d = work.pop()
        best = max(best, d)
        l, r = int(nodes["left"][v]), int(nodes["right"][v])
        if l < ni and r < ni:
            work.append((l, d + 1)); work.append((r, d))
        else:
            for ch in (l, r):
                if ch < ni:
                    work.append((ch, d))
    return best


def off_surface_points(tris, m, seed):
    """m points in and around the mesh's box (a quarter of them centroids jittered by 1e-2 of the extent)"""
    rng = np.random.default_rng(seed)
    v1, v2, v3 = tri_arrays(tris)
    v = np.concatenate([v1, v2, v3]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    p = lo - 0.25 * ext + rng.random((m, 3)) * 1.5 * ext
    k = m // 4
    t = rng.integers(0, len(tris), size=k)
    p[:k] = ((v1[t].astype(np.float64) + v2[t]) + v3[t]) / 3.0 + rng.normal(0, 1e-2, (k, 3)) * ext
    return p.astype(F32)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_winding_record_and_entry_points(pkg):
    types = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh", "types.h")).read(), flags=re.S)
    assert re.search(r"typedef struct\s*\{\s*float ax, ay, az, area;\s*float px, py, pz, r;\s*\}\s*bvh_winding_moment;", types)
    assert re.search(r"static_assert\(sizeof\(bvh_winding_moment\) == 32", types)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+bvh_winding_prepare\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*const bvh_result\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,\s*"
                     r"bvh_winding_moment\s*\*\s*\w+\s*\)", text)
    assert re.search(r"\bint\s+bvh_winding_number\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*const bvh_result\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,\s*"
                     r"const bvh_winding_moment\s*\*\s*\w+\s*,\s*const bvh_point_query\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*float\s+\w+\s*,\s*float\s*\*\s*\w+\s*\)", text)
    assert "#define BVH_ABI_VERSION 4" in text


def test_library_exports_winding_and_record_layout(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("bvh_winding_prepare", "bvh_winding_number"):
        assert hasattr(L, name) and name in pkg.EXPORTS
    dt = pkg.WINDING_MOMENT
    assert dt.itemsize == 32 and [dt.fields[k][1] for k in dt.names] == [0, 12, 16, 28]
    assert pkg.lib().bvh_abi_version() == 4


def test_winding_errors_without_a_device(pkg):
    lib = pkg.lib()
    assert lib.bvh_winding_prepare(None, None, None, None) == E_INVALID
    assert lib.bvh_winding_number(None, None, None, None, None, 0, 2.0, None) == E_INVALID
    r = pkg.Result(); r.n_leaves = 4; r.layout = 0; r.d_nodes = 64; r.d_tris = 64
    assert lib.bvh_winding_prepare(None, C.byref(r), None, 4096) == E_INVALID
    assert lib.bvh_winding_number(None, C.byref(r), None, 4096, 256, 4, 2.0, 8192) == E_INVALID


def test_builder_classes_have_the_winding_methods(pkg):
    for cls in pkg.BUILDERS.values():
        for name in ("winding_prepare", "winding_number", "signed_distance"):
            assert callable(getattr(cls, name))
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().winding_number(np.zeros((4, 3), dtype=F32))     # no tree yet
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().winding_prepare()


def test_cpp_mirror_winding_compiles(tmp_path):
    import subprocess
    src = tmp_path / "winding_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> void ask(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, bvh_winding_moment* m, const bvh_point_query* q, uint32_t n, float* w) {
    B bvh; bvh.build(ctx, a); bvh.windingPrepare(ctx, m); bvh.windingNumber(ctx, m, q, n, 2.0f, w);
}
void all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, bvh_winding_moment* m, const bvh_point_query* q, uint32_t n, float* w) {
    ask<BvhConstruction::TwoPassLbvh>(ctx, a, m, q, n, w); ask<BvhConstruction::SinglePassLbvh>(ctx, a, m, q, n, w);
    ask<BvhConstruction::PLOCNew>(ctx, a, m, q, n, w); ask<BvhConstruction::HPLOC>(ctx, a, m, q, n, w);
}
static_assert(sizeof(bvh_winding_moment) == 32, "size");
""")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the solid angle and the brute force -------------------------------------------------------------------------------------------------------------

def test_solid_angle_of_an_octant_face_and_its_sign(pkg):
    # the triangle (1,0,0), (0,1,0), (0,0,1) seen from the origin covers one octant: 1/8 of the sphere; its normal points away from the origin: positive
    t = [np.array(x, dtype=F32) for x in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    for dtype, tol in ((np.float64, 1e-15), (F32, 1e-7)):
        assert abs(float(leaf_terms(np.zeros(3), *t, dtype)) - 0.125) <= tol
        assert abs(float(leaf_terms(np.zeros(3), t[0], t[2], t[1], dtype)) + 0.125) <= tol
    assert leaf_terms(np.zeros(3), *t, F32).dtype == F32
    assert np.isnan(leaf_terms(np.array((np.nan, 0, 0)), *t, np.float64))
    assert float(leaf_terms(t[0], *t, F32)) == 0.0                 # on a vertex: atan2(0, 0) = 0


@pytest.mark.parametrize("n", [320, 1280])
def test_bunny_like_is_closed_and_outward_at_20_times_4_to_the_k(pkg, n):
    tris = pkg.meshgen.bunny_like(n)
    assert len(tris) == n
    pts = off_surface_points(tris, 2000, n)
    w = winding_brute_force(tris, pts)
    assert np.isfinite(w).all()
    assert (np.minimum(np.abs(w), np.abs(w - 1.0)) <= 1e-6).all()
    inside = w > 0.5
    assert 0.05 < inside.mean() < 0.95                              # both answers occur


def test_brute_force_on_an_open_mesh_and_nan_points(pkg):
    tris = pkg.meshgen.bunny_like(320)[:160]                        # half a blob: between 0 and 1 inside its hull
    pts = np.array([(0.0, 0.9, 0.0), (50.0, 0.9, 0.0), (np.nan, 0.0, 0.0)], dtype=F32)
    w = winding_brute_force(tris, pts)
    assert 0.05 < w[0] < 0.95 and abs(w[1]) < 1e-3 and np.isnan(w[2])


# ---- moments and walk on the CPU oracle's trees ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bunny_trees(pkg, orc):
    tris = pkg.meshgen.bunny_like(1280)
    out = {}
    for algo in (1, 3):                                             # a layout-0 and a layout-1 tree
        t = orc.build_tree(algo, tris)
        out[algo] = (t["nodes"], t["leaves"], t["layout"], t["root"])
    return tris, out


def test_moments_host_root_and_children(pkg, bunny_trees):
    tris, trees = bunny_trees
    v1, v2, v3 = (x.astype(np.float64) for x in tri_arrays(tris))
    A = 0.5 * np.cross(v2 - v1, v3 - v1)
    area = np.linalg.norm(A, axis=1)
    cen = (v1 + v2 + v3) / 3.0
    for algo, (nodes, leaves, layout, root) in trees.items():
        mom = moments_host(pkg, nodes, leaves, layout, root, tris)
        assert mom.dtype == pkg.WINDING_MOMENT and len(mom) == len(tris) - 1
        # the root holds the whole mesh: closed, so the area vectors cancel; the centre is the area-weighted centroid
        assert np.abs(mom["a"][root]).max() <= 1e-5 * area.sum()
        assert abs(mom["area"][root] - area.sum()) <= 1e-5 * area.sum()
        assert np.abs(mom["p"][root] - (area[:, None] * cen).sum(axis=0) / area.sum()).max() <= 1e-5
        # r reaches the farthest corner of the node's box, so every vertex of the subtree (inside the box) is within r of p
        lo, hi = nodes["min"][root].astype(np.float64), nodes["max"][root].astype(np.float64)
        far = np.maximum(np.abs(lo - mom["p"][root]), np.abs(hi - mom["p"][root]))
        assert abs(mom["r"][root] - np.linalg.norm(far)) <= 1e-6 * np.linalg.norm(far)
        assert np.linalg.norm(np.concatenate([v1, v2, v3]) - mom["p"][root], axis=1).max() <= mom["r"][root] * (1 + 1e-6)
        assert np.isfinite(mom.view(F32)).all() and (mom["r"] > 0).all() and (mom["area"] > 0).all()
    # the sums follow the tree: the same bytes on a second evaluation
    nodes, leaves, layout, root = trees[3]
    assert moments_host(pkg, nodes, leaves, layout, root, tris).tobytes() == moments_host(pkg, nodes, leaves, layout, root, tris).tobytes()


def test_moments_host_degenerate_node_takes_the_box_centre(pkg):
    # two zero-area triangles under one root: area 0 -> p is the centre of the root's box
    tris = np.zeros(2, dtype=pkg.meshgen.TRIANGLE)
    tris["v1"] = tris["v2"] = tris["v3"] = [(0, 0, 0), (2, 4, 6)]
    nodes = np.zeros(3, dtype=pkg.BVH2_NODE)
    nodes["left"] = (1, 0, 1); nodes["right"] = (2, pkg.INVALID, pkg.INVALID)
    nodes["min"] = [(0, 0, 0), (0, 0, 0), (2, 4, 6)]; nodes["max"] = [(2, 4, 6), (0, 0, 0), (2, 4, 6)]
    mom = moments_host(pkg, nodes, None, 0, 0, tris)
    assert mom["area"][0] == 0 and tuple(mom["p"][0]) == (1.0, 2.0, 3.0) and mom["r"][0] == F32(np.sqrt(F32(14.0)))


@pytest.mark.parametrize("algo", [1, 3])
def test_walk_host_against_the_brute_force(pkg, bunny_trees, algo):
    tris, trees = bunny_trees
    nodes, leaves, layout, root = trees[algo]
    mom = moments_host(pkg, nodes, leaves, layout, root, tris)
    pts = off_surface_points(tris, 600, 5)
    pts[-2:, 1] = np.nan
    bf = winding_brute_force(tris, pts)
    live = ~np.isnan(bf)
    assert live.sum() == len(pts) - 2
    # beta = +inf is the exact sum; the direct sum and the level-by-level expansion with a huge finite beta agree
    w_inf = walk_host(nodes, leaves, layout, root, tris, mom, pts, np.inf, np.float64)
    assert np.isnan(w_inf[~live]).all() and np.abs(w_inf[live] - bf[live]).max() <= 1e-12
    w_big = walk_host(nodes, leaves, layout, root, tris, mom, pts, 1e18, np.float64)
    assert np.abs(w_big[live] - bf[live]).max() <= 1e-12
    # finite beta: few terms, small error, the error falls as beta grows, the classification stands (the issue's table: 0.026 at 1 280, beta 2)
    prev = None
    for beta in (2.0, 3.0, 4.0):
        st = {}
        w = walk_host(nodes, leaves, layout, root, tris, mom, pts, beta, np.float64, st)
        err = np.abs(w[live] - bf[live]).max()
        assert st["terms"] < 0.5 * len(tris)
        assert err <= 0.1 and ((w > 0.5) == (bf > 0.5))[live].all()
        assert prev is None or err <= prev
        prev = err
    # f32 terms stay close to f64 terms: what the GPU tolerance is made from
    w32 = walk_host(nodes, leaves, layout, root, tris, mom, pts, 2.0, F32)
    w64 = walk_host(nodes, leaves, layout, root, tris, mom, pts, 2.0, np.float64)
    assert w32.dtype == F32 and np.abs(w32[live] - w64[live]).max() <= 1e-4


def test_stack_depth_all_open_on_a_left_chain(pkg):
    # root 0 = (1, 2), 1 = (3, 4) ... : a comb whose left child is always the deeper one
    ni = 5
    nodes = np.zeros(2 * ni + 1, dtype=pkg.BVH2_NODE)
    nodes["left"][:ni] = (1, 3, ni, ni + 2, ni + 4); nodes["right"][:ni] = (2, 4, ni + 1, ni + 3, ni + 5)
    assert stack_depth_all_open(nodes, 0, ni) == 2                  # pushes at node 0 (1 | 2) and node 1 (3 | 4)
