"""CPU: bvh_optimize (treelet restructuring) in the C ABI, the library and the C++ mirror, and the numpy restatement of its contract that the GPU
tests (tests/test_gpu_optimize.py) compare against byte for byte — itself checked against the oracle's trees and against exhaustive enumeration."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")

TREELET = 7                       # leaves of a treelet (and gamma of round 0)
FULL = (1 << TREELET) - 1
_F2 = np.float32(2)


def _area(lo, hi):
    """common.hpp box_area in f32, operation for operation: 2 * ((ex*ey + ex*ez) + ey*ez), no contraction"""
    with np.errstate(over="ignore", invalid="ignore"):              # (leaf and empty boxes: inf / NaN areas, as on the device)
        e = hi - lo
        ex, ey, ez = e[..., 0], e[..., 1], e[..., 2]
        return _F2 * (ex * ey + ex * ez + ey * ez)


# the proper subsets P of S that hold S's lowest set bit, in increasing mask order (the DP's candidate partitions {P, S \ P})
_PARTS = {}
for _s in range(1, FULL + 1):
    if _s & (_s - 1):
        _low = _s & -_s
        _PARTS[_s] = np.array([p for p in range(_low, _s) if (p & _s) == p and (p & _low)], dtype=np.int64)


def _first_min(vals):
    """per row: the index of the first strict minimum of a scan that starts with column 0 and moves on only for a value < the best so far (NaN never wins
    a comparison, a NaN in column 0 stays) — np.argmin's answer whenever a row holds no NaN"""
    best = np.argmin(vals, axis=1)
    bad = np.isnan(vals).any(axis=1)
    for k in np.nonzero(bad)[0]:
        b = 0
        for i in range(1, vals.shape[1]):
            if vals[k, i] < vals[k, b]:
                b = i
        best[k] = b
    return best


def reference_optimize(nodes, leaves, root, n, layout, rounds):
    """numpy restatement of bvh_optimize (include/bvh_mi355x.h).  nodes / leaves as bvh_download returns them (BVH2_NODE / PRIMREF, layout
    0 or 1; leaves only read).  Returns the new node array (leaf records, root and the treelet roots' boxes are untouched).

    Nodes are processed by height in the tree at the start of the round: two nodes of one height are disjoint subtrees, and a node's children keep their
    indices until the node itself is processed, so this is one of the bottom-up orders the contract allows (all give the same result)."""
    ni = n - 1
    nodes = nodes.copy()
    if layout == 0:
        lo = nodes["min"].copy(); hi = nodes["max"].copy()
    else:
        lo = np.concatenate([nodes["min"][:ni], leaves["min"]]); hi = np.concatenate([nodes["max"][:ni], leaves["max"]])
    left = nodes["left"][:ni].astype(np.int64); right = nodes["right"][:ni].astype(np.int64)
    total = 2 * n - 1
    for r in range(rounds):
        gamma = TREELET << r
        levels, frontier = [], np.array([root], dtype=np.int64)
        while frontier.size:
            levels.append(frontier)
            ch = np.concatenate([left[frontier], right[frontier]])
            frontier = ch[ch < ni]
        assert sum(len(lv) for lv in levels) == ni, "not a tree over n - 1 internal nodes"
        cnt = np.ones(total, dtype=np.int64); height = np.zeros(total, dtype=np.int64)
        for lv in reversed(levels):
            cnt[lv] = cnt[left[lv]] + cnt[right[lv]]
            height[lv] = 1 + np.maximum(height[left[lv]], height[right[lv]])
        internal = np.arange(ni)
        roots = internal[cnt[:ni] >= gamma]
        for h in np.unique(height[roots]):
            _restructure(roots[height[roots] == h], left, right, lo, hi, ni)
    nodes["left"][:ni] = left; nodes["right"][:ni] = right
    nodes["min"][:ni] = lo[:ni]; nodes["max"][:ni] = hi[:ni]
    return nodes


def _restructure(Ns, left, right, lo, hi, ni):
    """one batch of disjoint treelet roots: formation, current cost, DP, decision, rebuild (left / right / lo / hi updated in place)"""
    K = len(Ns)
    rows = np.arange(K)
    T = np.empty((K, TREELET), dtype=np.int64); T[:, 0] = left[Ns]; T[:, 1] = right[Ns]
    E = np.empty((K, TREELET - 2), dtype=np.int64)
    for size in range(2, TREELET):                                # formation: the collapse's rule (largest area, earliest position on ties)
        best = np.full(K, -1, dtype=np.int64); best_a = np.zeros(K, dtype=np.float32)
        for pos in range(size):
            idx = T[:, pos]
            a = _area(lo[idx], hi[idx])
            take = (idx < ni) & ((best < 0) | (a > best_a))
            best = np.where(take, pos, best); best_a = np.where(take, a, best_a)
        assert (best >= 0).all(), "a treelet root with >= 7 leaves always has an internal entry to expand"
        picked = T[rows, best]
        E[:, size - 2] = picked
        T[rows, best] = left[picked]; T[:, size] = right[picked]
    # current cost, deepest expansion first: c_cur(x) = area(x) + (c_cur(left x) + c_cur(right x)), 0 for the entries of T
    X = np.concatenate([Ns[:, None], E], axis=1)                  # the treelet's internal nodes: N, E0 .. E4
    cc = np.zeros((K, TREELET - 1), dtype=np.float32)
    for k in range(TREELET - 2, -1, -1):
        x = X[:, k]
        cl = np.zeros(K, dtype=np.float32); cr = np.zeros(K, dtype=np.float32)
        for k2 in range(k + 1, TREELET - 1):
            cl = np.where(X[:, k2] == left[x], cc[:, k2], cl); cr = np.where(X[:, k2] == right[x], cc[:, k2], cr)
        cc[:, k] = _area(lo[x], hi[x]) + (cl + cr)
    # subset boxes: the union of the entries' boxes in increasing bit order (B(S) = B(S without its highest bit) u box(highest bit))
    blo = np.empty((K, FULL + 1, 3), dtype=np.float32); bhi = np.empty((K, FULL + 1, 3), dtype=np.float32)
    for s in range(1, FULL + 1):
        top = s.bit_length() - 1
        rest = s ^ (1 << top)
        if rest == 0:
            blo[:, s] = lo[T[:, top]]; bhi[:, s] = hi[T[:, top]]
        else:
            blo[:, s] = np.fmin(blo[:, rest], lo[T[:, top]]); bhi[:, s] = np.fmax(bhi[:, rest], hi[T[:, top]])
    sa = _area(blo, bhi)
    c = np.zeros((K, FULL + 1), dtype=np.float32)
    part = np.zeros((K, FULL + 1), dtype=np.int64)
    for s, P in _PARTS.items():                                   # increasing mask order: every proper subset is done before s
        vals = c[:, P] + c[:, s ^ P]
        b = _first_min(vals)
        c[:, s] = sa[:, s] + vals[rows, b]
        part[:, s] = P[b]
    do = c[:, FULL] < cc[:, 0]
    for k in np.nonzero(do)[0]:                                   # rebuild: preorder, P before Q, E's indices handed out in ascending order
        free = iter(np.sort(E[k]).tolist())
        stack = [(FULL, int(Ns[k]))]
        while stack:
            s, idx = stack.pop()
            p = int(part[k, s]); q = s ^ p
            kids = []
            for sub in (p, q):
                kids.append(int(T[k, sub.bit_length() - 1]) if (sub & (sub - 1)) == 0 else next(free))
            left[idx], right[idx] = kids
            if idx != Ns[k]:                                      # (a treelet root keeps its box: its leaf set does not change)
                lo[idx] = blo[k, s]; hi[idx] = bhi[k, s]
            for sub, kid in ((q, kids[1]), (p, kids[0])):         # (popped P first)
                if sub & (sub - 1):
                    stack.append((sub, kid))


def internal_area_sum(nodes, leaves, root, n, layout):
    """f64 sum of the internal nodes' f32 areas (what restructuring lowers; the SAH's other terms are fixed)"""
    return float(_area(nodes["min"][:n - 1], nodes["max"][:n - 1]).astype(np.float64).sum())


def header_text():
    return open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()


# ---- the C ABI, the Python builders, the C++ mirror -------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_optimize(pkg):
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert re.search(r"\bint\s+bvh_optimize\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*bvh_result\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*bvh_timings\s*\*", text)
    assert re.search(r"#define\s+BVH_ABI_VERSION\s+4\b", header_text())
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_optimize")
    assert "bvh_optimize" in pkg.EXPORTS
    assert pkg.lib().bvh_optimize(None, None, 3, None) == -10001


def test_builder_classes_have_optimize(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "optimize"))
    with pytest.raises(pkg.BvhError):
        pkg.BUILDERS[1]().optimize()                        # no tree yet


def test_cpp_mirror_optimize_compiles(tmp_path):
    src = tmp_path / "optimize_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> void better(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a) {
    B bvh; bvh.build(ctx, a); bvh.optimize(ctx); bvh.optimize(ctx, 1); (void)bvh.m_cost;
}
void all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a) {
    better<BvhConstruction::TwoPassLbvh>(ctx, a); better<BvhConstruction::SinglePassLbvh>(ctx, a);
    better<BvhConstruction::PLOCNew>(ctx, a); better<BvhConstruction::HPLOC>(ctx, a);
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the restatement on the oracle's trees -------------------------------------------------------------------------------------------------------
_TREES = {}


def oracle_tree(pkg, orc, name, algo):
    if (name, algo) not in _TREES:
        tris = pkg.meshgen.load_tri(os.path.join(GOLDEN, name + ".tri"))
        _TREES[(name, algo)] = (len(tris), orc.build_tree(algo, tris))
    return _TREES[(name, algo)]


# SAH of the single-pass LBVH trees of the golden meshes: before, after 1 round, after 3 rounds
LBVH_SAH = {"cornell32": (22.0688, 18.1798, 18.0567), "cornell82": (26.7136, 20.7518, 20.1438), "cornell382": (28.7050, 21.8139, 21.2061)}


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
@pytest.mark.parametrize("rounds", [1, 3])
def test_reference_optimize_on_oracle_trees(pkg, orc, algo, rounds):
    for name in LBVH_SAH:
        n, t = oracle_tree(pkg, orc, name, algo)
        nodes, leaves, root, layout = t["nodes"], t["leaves"], t["root"], t["layout"]
        got = reference_optimize(nodes, leaves, root, n, layout, rounds)
        assert orc.validate_bvh2(got, leaves, root, n, layout) == 0, name
        if layout == 0:
            assert got[n - 1:].tobytes() == nodes[n - 1:].tobytes(), f"{name}: leaf records changed"
        assert got[root].tobytes()[8:] == nodes[root].tobytes()[8:], f"{name}: the root's box changed"
        before = orc.sah_bvh2(nodes, leaves, root, n, layout)[0]
        after = orc.sah_bvh2(got, leaves, root, n, layout)[0]
        assert after <= before, name
        if algo in (0, 1):
            assert after < before, name
        if algo == 1:
            want = LBVH_SAH[name]
            assert round(before, 4) == want[0], name
            assert round(after, 4) == want[1 if rounds == 1 else 2], (name, rounds, after)


def test_reference_optimize_leaves_small_trees_alone(pkg, orc):
    for n in (2, 3, 6):
        tris = pkg.meshgen.uniform(n, 3 + n)
        for algo in (1, 3):
            t = orc.build_tree(algo, tris)
            got = reference_optimize(t["nodes"], t["leaves"], t["root"], n, t["layout"], 3)
            assert got.tobytes() == t["nodes"].tobytes()


def _topologies(items):
    """every rooted binary tree over the leaf set `items`, as nested pairs"""
    if len(items) == 1:
        yield items[0]
        return
    first, rest = items[0], items[1:]
    for k in range(len(rest)):                        # the part holding `first`: first + a proper subset of the rest
        for sub in itertools.combinations(rest, k):
            other = [x for x in rest if x not in sub]
            for a in _topologies([first, *sub]):
                for b in _topologies(other):
                    yield (a, b)


def _min_internal_area(boxes):
    best, count = np.inf, 0

    def cost(t):
        if not isinstance(t, tuple):
            return boxes[t][0], boxes[t][1], 0.0
        l0, h0, c0 = cost(t[0]); l1, h1, c1 = cost(t[1])
        lo, hi = np.fmin(l0, l1), np.fmax(h0, h1)
        return lo, hi, c0 + c1 + float(_area(lo, hi))

    for t in _topologies(list(range(TREELET))):
        count += 1
        best = min(best, cost(t)[2])
    return best, count


def test_one_round_is_optimal_on_seven_leaves(orc):
    """a 7-leaf tree is one treelet: one round gives the minimum sum of internal areas over all 10 395 topologies"""
    from oracle import BVH2_NODE
    rng = np.random.default_rng(7)
    n = TREELET
    for trial in range(12):
        c = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
        e = rng.uniform(0.01, 2 + 3 * (trial % 3), (n, 3)).astype(np.float32)
        lo, hi = c - e, c + e
        # a random initial topology: leaves joined in a random order, internal nodes numbered 0 .. n-2 with the root at 0
        nodes = np.zeros(2 * n - 1, dtype=BVH2_NODE)
        nodes["min"][n - 1:] = lo; nodes["max"][n - 1:] = hi; nodes["left"][n - 1:] = np.arange(n); nodes["right"][n - 1:] = 0xFFFFFFFF
        pool = [(n - 1 + j, lo[j], hi[j]) for j in range(n)]
        nxt = n - 2
        while len(pool) > 1:
            i, j = sorted(rng.choice(len(pool), 2, replace=False))
            a, b = pool[i], pool[j]
            nodes["left"][nxt], nodes["right"][nxt] = a[0], b[0]
            blo, bhi = np.fmin(a[1], b[1]), np.fmax(a[2], b[2])
            nodes["min"][nxt], nodes["max"][nxt] = blo, bhi
            pool = [p for k, p in enumerate(pool) if k not in (i, j)] + [(nxt, blo, bhi)]
            nxt -= 1
        assert orc.validate_bvh2(nodes, None, 0, n, 0) == 0
        got = reference_optimize(nodes, None, 0, n, 0, 1)
        assert orc.validate_bvh2(got, None, 0, n, 0) == 0
        best, count = _min_internal_area([(lo[j], hi[j]) for j in range(n)])
        assert count == 10395
        have = internal_area_sum(got, None, 0, n, 0)
        assert have <= best * (1 + 1e-6), (trial, have, best)
