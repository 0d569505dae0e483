"""CPU: the inputs of tests/test_gpu_tree_passes_extremes.py — meshes whose built trees hold equal, zero, denormal, infinite and NaN box areas — the premises
that keep that file from being vacuous (ties in the optimiser's DP, rows tied at +inf, rows with a NaN, NaN-area internal nodes, trees that must not change),
and the checkers both files share.  bvh_optimize, bvh_collapse4, bvh_sah_cost, bvh_bvh4_cost and bvh_to_lbvh_layout read a built tree's box areas and decide by
comparing them; their contract on such trees consists of tie rules and IEEE rules (collapse.hip).  The counters are taken by wrapping
test_optimize._first_min while reference_optimize runs on the oracle's trees.  Run with -s for the table of counts."""
import contextlib

import numpy as np
import pytest

import test_optimize
from test_optimize import _area, reference_optimize
from test_query_extremes import mesh as special_mesh

F32 = np.float32
ALGOS = [0, 1, 2, 3]
ROUNDS = 3
TINY = np.finfo(F32).tiny

SPECIALS = ["inf_vertex", "neg_inf_vertex", "huge_triangle", "huge_offset", "nan_coordinate", "nan_vertex", "neg_nan_coordinate", "ff_filled_triangle", "denormals"]
SMALL = [f"quant8_{n}" for n in (2, 3, 6, 7, 8, 9, 63, 64, 65)]      # a treelet (7 leaves) and a wide node (4 children) first or last full
TABLE = ["base", "quant8", "quant4", "point_cloud_dups", "nonfinite40", "planar_inf64", "planar_inf8", "identical", "line", "staircase", "denormal_areas"]
MESH_NAMES = TABLE + SPECIALS + SMALL
NO_CHANGE = ["identical", "line", "staircase", "denormals"]          # every internal area is equal or zero: no treelet is strictly cheaper
ZERO_AREA = ["line", "staircase", "denormals"]                       # every internal area == 0: nothing expands, every wide node has two children
PLANAR = ["planar_inf64", "planar_inf8"]
CONSUMER_MESHES = ["inf_vertex", "huge_triangle", "planar_inf8"]

_MESHES, _TREES, _PREMISES = {}, {}, {}


def _nonfinite40(t):
    """test_gpu_refit.test_refit_with_nan_and_inf_coordinates' recipe (rng 15): 40 triangles each get NaN, +inf, -inf"""
    n = len(t)
    rng = np.random.default_rng(15)
    for val in (np.nan, np.inf, -np.inf):
        idx = rng.choice(n, 40, replace=False)
        for k, i in enumerate(idx):
            f = ("v1", "v2", "v3")[k % 3]
            v = t[f][i].copy()
            if k % 4 == 0:
                v[:] = val
            else:
                v[k % 3] = val
            t[f][i] = v
            if k % 10 == 0:
                for g in ("v1", "v2", "v3"):
                    w = t[g][i].copy(); w[1] = val; t[g][i] = w
    return t


def _planar_inf(t, count):
    """every z = 0.25 (extent 0 in z); `count` triangles get one infinite coordinate: the boxes above them have the area inf * 0 = NaN"""
    for v in ("v1", "v2", "v3"):
        t[v][:, 2] = 0.25
    idx = np.random.default_rng(3).choice(len(t), count, replace=False)
    t["v2"][idx[:count // 2], 0] = np.inf
    t["v1"][idx[count // 2:], 1] = -np.inf
    return t


def mesh(pkg, name):
    if name not in _MESHES:
        mg = pkg.meshgen
        if name in SPECIALS:
            t = special_mesh(pkg, name)
        elif name == "base":
            t = mg.uniform(4000, 77)
        elif name.startswith("quant"):
            kind, _, cut = name.partition("_")
            q = F32(int(kind[5:]))
            t = mg.uniform(4000, 5)
            for v in ("v1", "v2", "v3"):
                t[v] = np.round(t[v] * q) / q + F32(0)                 # (+ 0: no -0 coordinate)
            if cut:
                t = t[:int(cut)]
        elif name == "point_cloud_dups":
            t = np.tile(mg.uniform(64, 7), 50)
        elif name == "nonfinite40":
            t = _nonfinite40(mg.uniform(4000, 77))
        elif name in PLANAR:
            t = _planar_inf(mg.uniform(4000, 77), int(name[10:]))
        elif name == "identical":
            t = np.repeat(mg.uniform(1, 3), 3000)
        elif name == "line":
            t = mg.uniform(3000, 6)
            for v in ("v1", "v2", "v3"):
                t[v][:, 1] = 0.5; t[v][:, 2] = -2.0
        elif name == "staircase":
            t = mg.uniform(6000, 9)
            x = (F32(2.0) ** (-(np.arange(6000) % 120).astype(F32) / 4)) + (np.arange(6000) // 120).astype(F32) * F32(1e-6)
            for v in ("v1", "v2", "v3"):
                t[v][:, 0] = x; t[v][:, 1] = 0.0; t[v][:, 2] = 0.0
        elif name == "denormal_areas":
            t = mg.uniform(4000, 10)
            for v in ("v1", "v2", "v3"):
                t[v] *= F32(2.0 ** -66)
        else:
            raise KeyError(name)
        _MESHES[name] = np.ascontiguousarray(t)
    return _MESHES[name]


def oracle_tree(pkg, orc, name, algo):
    if (name, algo) not in _TREES:
        _TREES[(name, algo)] = orc.build_tree(algo, mesh(pkg, name))
    return _TREES[(name, algo)]


# ---- the counters -------------------------------------------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def counting_first_min():
    """counts the DP rows (one subset S of one treelet and its candidate partitions) that pass through test_optimize._first_min"""
    c = {"rows": 0, "tied": 0, "tied_inf": 0, "nan": 0}
    inner = test_optimize._first_min

    def counted(vals):
        nan = np.isnan(vals).any(axis=1)
        with np.errstate(invalid="ignore"):
            low = np.nanmin(np.where(np.isnan(vals), np.inf, vals), axis=1)
            tied = ((vals == low[:, None]).sum(axis=1) > 1) & ~nan
        c["rows"] += len(vals); c["nan"] += int(nan.sum()); c["tied"] += int(tied.sum()); c["tied_inf"] += int((tied & (low == np.inf)).sum())
        return inner(vals)
    test_optimize._first_min = counted
    try:
        yield c
    finally:
        test_optimize._first_min = inner


def internal_areas(nodes, n):
    return _area(nodes["min"][:n - 1], nodes["max"][:n - 1])


def changed_nodes(before, after, n):
    return int(np.count_nonzero(before[:n - 1] != after[:n - 1]))


def premises(pkg, orc, name, algo):
    """the oracle's tree, the restatement's tree after ROUNDS rounds, and the counters of the table in the module's docstring"""
    if (name, algo) not in _PREMISES:
        t = oracle_tree(pkg, orc, name, algo)
        n = len(mesh(pkg, name))
        with counting_first_min() as c:
            after = reference_optimize(t["nodes"], t["leaves"], t["root"], n, t["layout"], ROUNDS)
        a = internal_areas(t["nodes"], n)
        c.update(changed=changed_nodes(t["nodes"], after, n), zero=int((a == 0).sum()), inf=int(np.isinf(a).sum()), nan_area=int(np.isnan(a).sum()),
                 denormal=int(((a != 0) & (np.abs(a) < TINY)).sum()), internal=n - 1)
        _PREMISES[(name, algo)] = (t, after, c)
    return _PREMISES[(name, algo)]


# ---- the shared checkers --------------------------------------------------------------------------------------------------------------------------------------------

def levels_of(left, right, root, ni):
    levels, frontier = [], np.array([root], dtype=np.int64)
    while frontier.size:
        levels.append(frontier)
        ch = np.concatenate([left[frontier], right[frontier]])
        frontier = ch[ch < ni]
    return levels


def collapse_map(nodes, leaves, root, n, layout, wide, prims, total):
    """which BVH2 node every wide node stands for and which BVH2 nodes the collapse expanded, found WITHOUT the collapse's rule: every node of either tree is
    identified by the set of primitives below it (a sum of one random 64-bit word per primitive).  Returns (t, expanded): t[g] = the BVH2 node of wide node g,
    expanded = the BVH2 internal nodes strictly between some t[g] and g's children.  Asserts that the wide tree is a collapse of this BVH2 at all."""
    ni = n - 1
    word = np.random.default_rng(99).integers(1, 2 ** 63, size=n, dtype=np.uint64)
    left = nodes["left"][:ni].astype(np.int64); right = nodes["right"][:ni].astype(np.int64)
    leaf_prim = (nodes["left"][ni:2 * ni + 1] if layout == 0 else leaves["prim"]).astype(np.int64)
    assert np.array_equal(prims["prim"], leaf_prim.astype(np.uint32)), "PrimNode[j].prim is not leaf j's primitive"
    sig2 = np.zeros(2 * n - 1, dtype=np.uint64); sig2[ni:] = word[leaf_prim]
    parent2 = np.full(2 * n - 1, -1, dtype=np.int64)
    parent2[left] = np.arange(ni); parent2[right] = np.arange(ni)
    for lv in reversed(levels_of(left, right, root, ni)):
        sig2[lv] = sig2[left[lv]] + sig2[right[lv]]
    assert len(np.unique(sig2)) == 2 * n - 1
    child = wide["child"][:total].astype(np.int64); count = wide["count"][:total].astype(np.int64)
    used = np.arange(4)[None] < count[:, None]
    assert ((child == 0xFFFFFFFF) == ~used).all(), "a child slot at or beyond count is not INVALID (or one below it is)"
    internal = used & (child < ni)
    assert (child[internal] < total).all() and (child[used & ~internal] < 2 * n - 1).all()
    wlevels, frontier = [], np.array([0], dtype=np.int64)
    while frontier.size:
        wlevels.append(frontier)
        frontier = child[frontier][internal[frontier]]
    assert sum(len(lv) for lv in wlevels) == total
    sig4 = np.zeros(total, dtype=np.uint64)
    for lv in reversed(wlevels):
        c = child[lv]
        s = np.where(internal[lv], sig4[np.where(internal[lv], c, 0)], 0).astype(np.uint64) + np.where(used[lv] & ~internal[lv], sig2[np.where(used[lv] & ~internal[lv], c, ni)], 0).astype(np.uint64)
        sig4[lv] = s.sum(axis=1, dtype=np.uint64)
    order = np.argsort(sig2[:ni]); sorted_sig = sig2[:ni][order]
    at = np.searchsorted(sorted_sig, sig4)
    assert (at < ni).all() and (sorted_sig[at] == sig4).all(), "a wide node's primitives are no BVH2 node's"
    t = order[at]
    assert t[0] == root
    expanded = []
    for g in range(total):
        for k in range(count[g]):
            c = t[child[g, k]] if internal[g, k] else child[g, k]
            p = parent2[c]
            while p != t[g]:
                assert p >= 0, "a wide node's child is not below its BVH2 node"
                expanded.append(p); p = parent2[p]
    expanded = np.unique(np.array(expanded, dtype=np.int64))
    assert len(expanded) + total == ni, "tasks and expanded nodes together are not the internal nodes"
    return t, expanded


def check_collapse(orc, nodes, leaves, root, n, layout, wide, prims, total, what, zero_area=False):
    """the wide tree against the BVH2 it was made from: structure, the permutation, the stored boxes, and the reference's rule read off the BVH2 — an expanded
    node has an area > 0 (never 0, never NaN: `a > best` from best = 0)"""
    ni = n - 1
    assert orc.topology_hash4(wide, prims, total, n) != 0, what
    assert np.array_equal(np.sort(prims["prim"]), np.arange(n, dtype=np.uint32)), f"{what}: prims is not a permutation"
    t, expanded = collapse_map(nodes, leaves, root, n, layout, wide, prims, total)
    a = internal_areas(nodes, n)
    assert (a[expanded] > 0).all(), f"{what}: {int((~(a[expanded] > 0)).sum())} expanded nodes have a zero or NaN area ({int(np.isnan(a[expanded]).sum())} NaN)"
    child = wide["child"][:total].astype(np.int64)
    internal = child < ni
    box = t[np.where(internal, child, 0)]
    for f in ("min", "max"):
        assert wide["aabb"][f][:total][internal].tobytes() == nodes[f][box][internal].tobytes(), f"{what}: an internal child's box is not its BVH2 node's"
        reset = np.full(3, np.finfo(F32).max if f == "min" else -np.finfo(F32).max, dtype=F32)
        assert (wide["aabb"][f][:total][~internal] == reset).all(), f"{what}: a leaf slot does not hold the reset box"
    if zero_area:
        assert (wide["count"][:total] == 2).all(), f"{what}: a zero-area internal node was expanded"
    return expanded


def cost_class(x):
    return "nan" if np.isnan(x) else "+inf" if x == np.inf else "-inf" if x == -np.inf else "finite"


def bvh4_cost_restated(wide, prims, prim_boxes, total, n):
    """k_bvh4_cost's sum, term for term: every term is the f32 product area * (1 / root area) — infinite or NaN when the root area is a denormal (1 / area
    overflows), zero or infinite — accumulated in f64 (the order of an f64 sum of these terms cannot change its class)"""
    ni = n - 1
    with np.errstate(all="ignore"):
        lo = np.full(3, np.finfo(F32).max, dtype=F32); hi = -lo
        for k in range(4):
            if wide["child"][0, k] != 0xFFFFFFFF:
                lo = np.fmin(lo, wide["aabb"]["min"][0, k]); hi = np.fmax(hi, wide["aabb"]["max"][0, k])
        inv = F32(1.0) / _area(lo, hi)
        internal = wide["child"][:total] < ni
        terms = _area(wide["aabb"]["min"][:total], wide["aabb"]["max"][:total])[internal] * inv
        leaf = _area(prim_boxes["min"][prims["prim"]], prim_boxes["max"][prims["prim"]]) * inv
        return float(1.0 + terms.astype(np.float64).sum() + leaf.astype(np.float64).sum())


def sah_cost_restated(nodes, leaves, root, n, layout):
    """k_sah's sum, term for term: (double) area / (double) root area over both children of every internal node and over every leaf, in f64"""
    ni = n - 1
    with np.errstate(all="ignore"):
        if layout == 0:
            a = _area(nodes["min"], nodes["max"]).astype(np.float64)
        else:
            a = np.concatenate([_area(nodes["min"], nodes["max"]), _area(leaves["min"], leaves["max"])]).astype(np.float64)
        kids = np.concatenate([nodes["left"][:ni], nodes["right"][:ni]]).astype(np.int64)
        return float(1.0 + (a[kids] / a[root]).sum() + (a[ni:] / a[root]).sum())


def lbvh_layout_restated(nodes, leaves, n):
    """bvh_to_lbvh_layout in numpy: internal nodes verbatim, leaf j as {prim, INVALID, box}"""
    out = np.zeros(2 * n - 1, dtype=nodes.dtype)
    out[:n - 1] = nodes[:n - 1]
    out["left"][n - 1:] = leaves["prim"]; out["right"][n - 1:] = 0xFFFFFFFF
    out["min"][n - 1:] = leaves["min"]; out["max"][n - 1:] = leaves["max"]
    return out


_PLANAR_QUERIES = []


def planar_queries(pkg):
    """planar_inf8 is not one of test_query_extremes' meshes: its own rays (from off the plane z = 0.25 towards points of it) and points (around the plane, the
    radius infinite or 0.2 in turn) with their brute forces, computed once: (rays, ray brute force, points, point brute force)"""
    if not _PLANAR_QUERIES:
        from test_point_query import point_brute_force
        from test_query import brute_force
        tris = mesh(pkg, "planar_inf8")
        base = pkg.meshgen.uniform(4000, 77)
        v = np.concatenate([base["v1"], base["v2"], base["v3"]]).astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        rng = np.random.default_rng(808)
        m = 192
        target = lo + rng.random((m, 3)) * (hi - lo); target[:, 2] = 0.25
        o = target + rng.normal(0, 0.3, (m, 3)); o[:, 2] = 0.25 + np.where(np.arange(m) % 2 == 0, 1.0, -1.0) * (0.1 + rng.random(m))
        d = target - o
        rays = np.zeros(m, dtype=pkg.RAY)
        rays["origin"] = o; rays["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True); rays["tmax"] = F32(3.0e38)
        pts = np.zeros(m, dtype=pkg.POINT_QUERY)
        p = lo + rng.random((m, 3)) * (hi - lo); p[:, 2] = 0.25 + rng.normal(0, 0.05, m)
        pts["point"] = p; pts["radius"] = np.where(np.arange(m) % 2 == 0, np.inf, 0.2)
        _PLANAR_QUERIES.append((rays, brute_force(rays, tris), pts, point_brute_force(pkg, pts, tris)))
    return _PLANAR_QUERIES[0]


# ---- the premises ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_planar_queries_are_well_conditioned_and_answered(pkg):
    rays, bf, pts, pbf = planar_queries(pkg)
    print(f"planar_inf8: rays well {bf['well'].mean():.3f} hit {bf['hit'].mean():.3f}; points well {pbf['well'].mean():.3f} hit {pbf['hit'].mean():.3f}")
    assert bf["well"].mean() >= 0.99 and pbf["well"].mean() >= 0.99
    assert bf["hit"].mean() >= 0.25 and pbf["hit"].mean() >= 0.5


@pytest.mark.parametrize("name", MESH_NAMES)
def test_premises_and_oracle_side_checks(pkg, orc, name):
    """per mesh and builder: the counters (printed; the conditions are fixed, the counts are DESIGN.md's), and on the oracle's tree before and after the
    restatement's three rounds: a valid BVH2, a collapse that is a collapse of it, the reference's expansion rule read off the BVH2.  (identical, line, staircase
    and denormals take 30 to 150 s each: their PLOC++ and HPLOC trees are thousands of levels deep, and the restatement works through a tree level by level.)"""
    n = len(mesh(pkg, name))
    assert n <= 6000
    for algo in ALGOS:
        t, after, c = premises(pkg, orc, name, algo)
        print(f"{name:22s} algo {algo}: rows {c['rows']:7d} tied {c['tied']:7d} tied at +inf {c['tied_inf']:6d} NaN rows {c['nan']:6d} changed {c['changed']:5d} of "
              f"{c['internal']:5d}  internal areas: zero {c['zero']:5d} denormal {c['denormal']:5d} inf {c['inf']:4d} NaN {c['nan_area']:4d}")
        what = f"{name} algo {algo}"
        if name in ("quant8", "point_cloud_dups"):
            assert c["tied"] > 0 and c["changed"] > 0, what
        if name == "nonfinite40":
            assert c["tied_inf"] > 0, what
        if name == "planar_inf64":
            assert c["nan"] > 0 and c["nan_area"] > 0 and c["changed"] > 0, what
        if name in ZERO_AREA:
            assert c["zero"] == c["internal"], what
        if name == "denormal_areas":
            assert c["denormal"] == c["internal"], what
        if name in NO_CHANGE:
            assert c["changed"] == 0 and after.tobytes() == t["nodes"].tobytes(), what
        if n < 7:
            assert c["rows"] == 0 and after.tobytes() == t["nodes"].tobytes(), what
        for tag, nodes in (("as built", t["nodes"]), ("optimised", after)):
            assert orc.validate_bvh2(nodes, t["leaves"], t["root"], n, t["layout"]) == 0, f"{what} {tag}"
            wide, prims, total = orc.collapse4(nodes, t["leaves"], t["root"], n, t["layout"])
            expanded = check_collapse(orc, nodes, t["leaves"], t["root"], n, t["layout"], wide, prims, total, f"{what} {tag}", zero_area=name in ZERO_AREA)
            if name in PLANAR:                                        # the oracle itself is pinned to the reference's rule before the device is compared with it
                a = internal_areas(nodes, n)
                assert np.isnan(a).sum() > 0 and not np.isnan(a[expanded]).any(), f"{what} {tag}"


def test_cost_restatements_agree_with_the_oracle_where_both_are_finite(pkg, orc):
    """the numpy sums the GPU file falls back on for the class of a cost (NaN, +inf, finite) are the oracle's sums on an ordinary tree"""
    for name in ("base", "quant8_65"):
        tris = mesh(pkg, name); n = len(tris)
        boxes, _ = orc.prim_bounds(tris)
        for algo in ALGOS:
            t, after, _ = premises(pkg, orc, name, algo)
            for nodes in (t["nodes"], after):
                c = orc.sah_bvh2(nodes, t["leaves"], t["root"], n, t["layout"])[0]
                assert abs(sah_cost_restated(nodes, t["leaves"], t["root"], n, t["layout"]) - c) <= 1e-12 * c
                wide, prims, total = orc.collapse4(nodes, t["leaves"], t["root"], n, t["layout"])
                c4 = orc.sah_bvh4(wide, prims, boxes, total, n)[0]
                assert abs(bvh4_cost_restated(wide, prims, boxes, total, n) - c4) <= 1e-6 * c4      # (f32 products against f64 quotients)


def test_cost_classes_on_the_extreme_trees(pkg, orc):
    """which answers the GPU file expects of the two cost entry points: NaN and +inf are answers here.  bvh_sah_cost's class is the oracle's on every tree (the
    same f64 quotients in another order); bvh_bvh4_cost's is not on `denormal_areas`, where 1 / root area overflows in f32 and the oracle divides in f64"""
    seen = {}
    for name in MESH_NAMES:
        tris = mesh(pkg, name); n = len(tris)
        boxes, _ = orc.prim_bounds(tris)
        t = oracle_tree(pkg, orc, name, 1)
        c = orc.sah_bvh2(t["nodes"], None, t["root"], n, 0)[0]
        assert cost_class(sah_cost_restated(t["nodes"], None, t["root"], n, 0)) == cost_class(c), name
        wide, prims, total = orc.collapse4(t["nodes"], None, t["root"], n, 0)
        c4 = orc.sah_bvh4(wide, prims, boxes, total, n)[0]; r4 = bvh4_cost_restated(wide, prims, boxes, total, n)
        seen[name] = (cost_class(c), cost_class(c4), cost_class(r4))
        print(f"{name:22s} SAH {c!r:24} BVH4 cost: oracle f64 {c4!r:24} kernel's terms {r4!r}")
    assert {"nan", "+inf", "finite"} <= {v[0] for v in seen.values()}
    differ = sorted(k for k, v in seen.items() if v[1] != v[2])
    print("BVH4 cost class differs between the oracle's f64 quotients and the kernel's f32 products on:", differ)
    assert "denormal_areas" in differ


def test_small_sizes_cross_the_treelet_and_wide_node_limits(pkg, orc):
    t = mesh(pkg, "quant8")
    for name in SMALL:
        n = int(name.split("_")[1])
        assert mesh(pkg, name).tobytes() == t[:n].tobytes()
    v = np.concatenate([t["v1"], t["v2"], t["v3"]])
    assert (v * 8 == np.round(v * 8)).all() and not np.signbit(v[v == 0]).any()


def test_counting_leaves_the_restatement_alone(pkg, orc):
    """the wrapped _first_min returns what the plain one does, and is put back afterwards"""
    plain = test_optimize._first_min
    n = len(mesh(pkg, "planar_inf8"))
    t = oracle_tree(pkg, orc, "planar_inf8", 1)
    want = reference_optimize(t["nodes"], None, t["root"], n, 0, 2)
    with counting_first_min() as c:
        got = reference_optimize(t["nodes"], None, t["root"], n, 0, 2)
    assert test_optimize._first_min is plain and got.tobytes() == want.tobytes() and c["rows"] > 0
