"""CPU: bvh_cull's reference and premises.  The numpy restatement of the plane-box test (pkg.cull_brute_force, the single reference of these tests and of
tests/test_gpu_cull.py), its monotonicity under box containment in rounded f32 (what makes the hierarchical answer exact), its exact boundaries, the host
restatements of the lane walk (with and without plane masking) and of the group walk's schedule on the CPU oracle's trees, the volume families the GPU tests
use with the properties they must have, and frustum_planes."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_query import mesh
from test_overlap import AABB, as_boxes, leaf_boxes_of

F32 = np.float32
GROUP_BLOCK = 256                                                   # threads of the group walk's workgroup (cull.hip)
PADDING = (0.0, 0.0, 0.0, 1.0)
WALK_MESHES = ["cornell32", "cornell82", "cornell382", "uniform_1000"]
PLANE_COUNTS = (1, 6, 8)
N_VOLUMES = 257
N_SPECIAL = 10                                                      # volumes in front of the random ones (make_volumes)


# ---- cameras ------------------------------------------------------------------------------------------------------------------------------------------------

def perspective(fovy, aspect, near, far, zero_to_one=True):
    """row-major clip matrix, column-vector convention, camera looking down -z"""
    f = 1.0 / np.tan(0.5 * fovy)
    m = np.zeros((4, 4))
    m[0, 0] = f / aspect; m[1, 1] = f; m[3, 2] = -1.0
    if zero_to_one:
        m[2, 2] = far / (near - far); m[2, 3] = near * far / (near - far)
    else:
        m[2, 2] = (far + near) / (near - far); m[2, 3] = 2.0 * far * near / (near - far)
    return m


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = target - eye; f /= np.linalg.norm(f)
    s = np.cross(f, up)
    if np.linalg.norm(s) < 1e-6:
        s = np.cross(f, (1.0, 0.0, 0.0))
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[:3, 3] = -m[:3, :3] @ eye
    return m


# ---- the volume families ------------------------------------------------------------------------------------------------------------------------------------

def box_planes(lo, hi):
    """the six inside-positive planes of the axis-aligned box [lo, hi]"""
    return [(1.0, 0.0, 0.0, -lo[0]), (-1.0, 0.0, 0.0, hi[0]), (0.0, 1.0, 0.0, -lo[1]), (0.0, -1.0, 0.0, hi[1]), (0.0, 0.0, 1.0, -lo[2]), (0.0, 0.0, -1.0, hi[2])]


def make_volumes(pkg, leaf_boxes, points, seed, per, count=N_VOLUMES):
    """``count`` volumes of ``per`` planes (1, 6 or 8; 8 is 6 padded with (0, 0, 0, 1)) around the scene of ``leaf_boxes``, f32 (count, per, 4).  First the
    N_SPECIAL special ones — 0 contains everything (every mask 0), 1 a half-space through the centroid, 2 misses everything, 3 a zero-thickness slab through a
    vertex coordinate (per 1: the half-space that ends there), 4 / 5 the exact-boundary planes n = (1, -0, 0) through a leaf box's max x (passes: s = 0) and
    one ulp beyond it (fails), 6 a plane holding a NaN, 7 a half-space through the centroid along another axis with a -0 component, 8 / 9 the all-containing
    and the all-missing volume scaled by 2^-6 and 2^3 (planes need not be normalised) —, then random ones: camera frusta from pkg.frustum_planes in both
    depth conventions (per 1: one random half-space through a random vertex).  All finite inputs have magnitudes <= 1e3."""
    lb = as_boxes(leaf_boxes)
    rng = np.random.default_rng(seed)
    lo = lb["min"].astype(np.float64).min(axis=0); hi = lb["max"].astype(np.float64).max(axis=0)
    ext = np.maximum(hi - lo, 1e-3); ctr = 0.5 * (lo + hi)
    pts = np.asarray(points, dtype=F32).reshape(-1, 3)
    vtx = pts[rng.integers(0, len(pts))].astype(np.float64)
    j = int(rng.integers(0, len(lb)))
    face = F32(lb["max"][j, 0]); beyond = np.nextafter(face, F32(np.inf))
    pad = [PADDING] * 8

    def vol(planes):
        return (list(planes) + pad)[:per] if per != 1 else [planes[0]]
    spec = [
        vol(box_planes(lo - ext, hi + ext)),
        vol([(1.0, 0.0, 0.0, -ctr[0])]),
        vol(box_planes(hi + 10.0 * ext, hi + 11.0 * ext)),
        vol([(1.0, 0.0, 0.0, -vtx[0]), (-1.0, 0.0, 0.0, vtx[0])]),
        vol([(1.0, -0.0, 0.0, -face)]),
        vol([(1.0, -0.0, 0.0, -beyond)]),
        vol([(0.0, 1.0, 0.0, np.nan)] + box_planes(lo - ext, hi + ext)[:5]),
        vol([(-0.0, 0.0, -1.0, ctr[2])]),
        vol([tuple(2.0 ** -6 * np.array(p)) for p in box_planes(lo - ext, hi + ext)]),
        vol([(0.0, 0.0, 0.0, -1.0)] if per == 1 else [tuple(2.0 ** 3 * np.array(p)) for p in box_planes(hi + 10.0 * ext, hi + 11.0 * ext)]),
    ]
    if per == 1:
        spec[0] = [PADDING]; spec[8] = [(0.0, 0.0, 0.0, 2.0 ** -6)]
        spec[2] = [(0.0, 0.0, 0.0, -1.0)]
    assert len(spec) == N_SPECIAL
    out = np.zeros((count, per, 4), dtype=F32)
    out[:, :, 3] = 1.0
    out[:N_SPECIAL] = np.array(spec, dtype=np.float64).astype(F32)[:count]
    diag = float(np.linalg.norm(ext))
    for i in range(N_SPECIAL, count):
        if per == 1:
            nrm = rng.normal(size=3); nrm /= np.linalg.norm(nrm)
            p = pts[rng.integers(0, len(pts))].astype(np.float64)
            out[i, 0] = (*nrm, -float(nrm @ p))
            continue
        eye = ctr + rng.normal(size=3) * ext * rng.choice([0.3, 1.5])
        target = lo + rng.random(3) * ext
        if np.linalg.norm(target - eye) < 1e-3 * diag:
            target = eye + (0.0, 0.0, -1.0)
        near = diag * rng.choice([0.01, 0.2]); far = near + diag * rng.choice([0.3, 3.0])
        zero_to_one = bool(i & 1)
        clip = perspective(np.radians(rng.uniform(10.0, 100.0)), rng.choice([1.0, 16.0 / 9.0]), near, far, zero_to_one) @ look_at(eye, target)
        out[i, :6] = pkg.frustum_planes(clip, depth_zero_to_one=zero_to_one)
    return out


def slices_of(offsets, hits):
    return [hits[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


def sorted_hits(offsets, hits):
    """hits with every slice in ascending prim order: the canonical form of an answer (the order inside a slice is unspecified)"""
    owner = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets.astype(np.int64)))
    return hits[np.lexsort((hits["prim"], owner))]


def check_premises(offsets, hits, n, what):
    """what every family must contain for the tests to mean something (asserted on the reference alone)"""
    counts = np.diff(offsets.astype(np.int64))
    assert (counts == 0).any(), f"{what}: no empty slice"
    assert (counts == n).any(), f"{what}: no slice holds every primitive"
    if n >= 3:
        assert ((counts > 0) & (counts < n)).any(), f"{what}: no partial slice"
    assert (hits["straddle"] == 0).any() and (hits["straddle"] != 0).any(), f"{what}: the straddle masks are all zero or all non-zero"
    assert (hits["straddle"][offsets[0]:offsets[1]] == 0).all() and counts[0] == n, f"{what}: volume 0 does not contain everything"
    assert counts[2] == 0 and counts[6] == 0, f"{what}: the missing volume or the NaN plane's volume is not empty"


# ---- trees as the walks read them ---------------------------------------------------------------------------------------------------------------------------

class Tree:
    """the combined index space of the kernels: internal [0, ni), leaf j at ni + j"""

    def __init__(self, nodes, leaves, root, n, layout):
        ni = n - 1
        self.n, self.ni, self.root = n, ni, int(root)
        self.left = nodes["left"][:ni].astype(np.int64); self.right = nodes["right"][:ni].astype(np.int64)
        if layout == 0:
            self.lo, self.hi = nodes["min"].astype(F32), nodes["max"].astype(F32)
            self.prim = nodes["left"][ni:].astype(np.int64)
        else:
            self.lo = np.concatenate([nodes["min"][:ni], leaves["min"]]).astype(F32); self.hi = np.concatenate([nodes["max"][:ni], leaves["max"]]).astype(F32)
            self.prim = leaves["prim"].astype(np.int64)
        self.leaf_boxes = leaf_boxes_of(nodes, leaves, n, layout)
        self.kids = list(zip(self.left.tolist(), self.right.tolist()))      # (plain lists: the lane walk indexes them node by node)
        self.prims = self.prim.tolist()


def node_tests(pkg, tree, volume):
    """per plane and node: (s(p) >= 0, s(n) >= 0) as bool arrays (planes, 2n - 1), and the nodes' validity"""
    s_p, s_n = pkg.cull_plane_values(volume[:, None, :], tree.lo[None], tree.hi[None])
    with np.errstate(invalid="ignore"):
        return s_p >= F32(0.0), s_n >= F32(0.0), (tree.lo <= tree.hi).all(axis=1)


def lane_walk(pkg, tree, volume, masking):
    """k_cull_walk restated: both children tested per internal node, a passing leaf child reported at once, of two passing internal children the left entered
    and the right pushed; the root's own box is not tested.  ``masking``: a plane whose n-vertex value is >= 0 at a node is dropped below it, and the mask
    travels with a pushed entry (the kernel itself restarts a popped node with all planes: masking off).  Returns (records sorted by prim, deepest stack)."""
    pass_p, inside_n, valid = node_tests(pkg, tree, volume)
    per = len(volume); ni = tree.ni
    pass_p, inside_n, valid = pass_p.T.tolist(), inside_n.T.tolist(), valid.tolist()      # [node][plane]
    out, stack, deepest = [], [], 0
    v, active = tree.root, tuple(range(per))
    while True:
        kids = []
        for c in tree.kids[v]:
            if valid[c] and all(pass_p[c][k] for k in active):
                if c >= ni:
                    out.append((tree.prims[c - ni], sum((0 if inside_n[c][k] else 1) << k for k in range(per))))
                else:
                    kids.append((c, tuple(k for k in active if not inside_n[c][k]) if masking else active))
        if len(kids) == 2:
            stack.append(kids[1]); deepest = max(deepest, len(stack))
        if kids:
            v, active = kids[0]
        elif stack:
            v, active = stack.pop()
        else:
            break
    rec = np.array(sorted(out), dtype=np.int64).reshape(-1, 2)
    hits = np.zeros(len(rec), dtype=pkg.CULL_HIT)
    hits["prim"], hits["straddle"] = rec[:, 0], rec[:, 1]
    return hits, deepest


def group_walk(pkg, tree, volume):
    """k_cull_group's schedule restated: each round takes the m = min(top, 256) entries at the top of the stack, thread t entry top - m + t; both children are
    tested; leaf survivors are emitted and internal survivors pushed, both in thread order, left child before right.  Returns (records in emission order,
    the largest occupancy of the stack after a round's pushes — what the kernel compares with BVH_CULL_GROUP_STACK)."""
    pass_p, inside_n, valid = node_tests(pkg, tree, volume)
    ok = valid & pass_p.all(axis=0)
    bits = (np.uint32(1) << np.arange(len(volume), dtype=np.uint32))[:, None]
    mask = np.where(inside_n, np.uint32(0), bits).sum(axis=0, dtype=np.uint32)
    ni = tree.ni
    stack = np.array([tree.root], dtype=np.int64)
    prims, masks, peak = [], [], 1
    while len(stack):
        m = min(len(stack), GROUP_BLOCK)
        ent, stack = stack[len(stack) - m:], stack[:len(stack) - m]
        kids = np.stack([tree.left[ent], tree.right[ent]], axis=1).reshape(-1)
        kids = kids[ok[kids]]
        leaf = kids[kids >= ni]
        prims.append(tree.prim[leaf - ni]); masks.append(mask[leaf])
        stack = np.concatenate([stack, kids[kids < ni]])
        peak = max(peak, len(stack))
    hits = np.zeros(sum(len(p) for p in prims), dtype=pkg.CULL_HIT)
    if len(hits):
        hits["prim"], hits["straddle"] = np.concatenate(prims), np.concatenate(masks)
    return hits, peak


def by_prim(hits):
    return hits[np.argsort(hits["prim"], kind="stable")]


def fat_caterpillar(pkg, levels, seed=0):
    """a layout-0 tree on which the group walk's stack grows by 256 entries per round: every level has 512 internal nodes, of which the 256 pushed LAST (the
    children of the round's threads 128 .. 255: the top of the stack) each have two internal children again, while the other 256 hold two leaves each and stay
    in the stack until the chain ends.  An all-containing volume therefore reaches an occupancy of about 256 * levels, on about 1024 * levels leaves.  Leaf
    boxes are random small boxes in [0, 100]^3; internal boxes the bitwise union of their children's.  Returns (leaf AABB[n], nodes, root, n)."""
    rng = np.random.default_rng(seed)
    kids, is_leaf_pair = {}, []
    next_id = [0]

    def new():
        next_id[0] += 1
        return next_id[0] - 1
    root = new()
    # the top: a complete tree down to 256 nodes (8 levels), in breadth-first order: each round pops a whole level
    level = [root]
    while len(level) < GROUP_BLOCK:
        nxt = []
        for v in level:
            a, b = new(), new(); kids[v] = (a, b); nxt += [a, b]
        level = nxt
    for _ in range(levels):
        nxt = []
        for v in level:
            a, b = new(), new(); kids[v] = (a, b); nxt += [a, b]
        for v in nxt[:GROUP_BLOCK]:                                  # pushed first: deeper in the stack, stay there
            kids[v] = None
        level = nxt[GROUP_BLOCK:]
    for v in level:
        kids[v] = None
    ni = next_id[0]; n = ni + 1
    nodes = np.zeros(2 * n - 1, dtype=pkg.BVH2_NODE)
    ctr = rng.random((n, 3)) * 100.0; half = rng.random((n, 3)) * 0.5
    nodes["min"][ni:] = (ctr - half).astype(F32); nodes["max"][ni:] = (ctr + half).astype(F32)
    nodes["left"][ni:] = np.arange(n); nodes["right"][ni:] = pkg.INVALID
    leaf = [ni]

    def take_leaf():
        leaf[0] += 1
        return leaf[0] - 1
    for v in range(ni - 1, -1, -1):                                  # ids grow with depth: children before parents
        a, b = kids[v] if kids[v] is not None else (take_leaf(), take_leaf())
        nodes["left"][v], nodes["right"][v] = a, b
        nodes["min"][v] = np.minimum(nodes["min"][a], nodes["min"][b]); nodes["max"][v] = np.maximum(nodes["max"][a], nodes["max"][b])
    assert leaf[0] == 2 * n - 1
    boxes = np.zeros(n, dtype=AABB)
    boxes["min"], boxes["max"] = nodes["min"][ni:], nodes["max"][ni:]
    return boxes, nodes, root, n


# ---- 1. monotonicity ----------------------------------------------------------------------------------------------------------------------------------------

def test_plane_test_is_monotone_under_containment(pkg):
    """200 000 random nested box pairs (magnitudes <= 1e3), each with a plane placed within a few ulps of tangent to the inner box's p-vertex or n-vertex: in
    rounded f32 the outer box's p-value is never below the inner's, its n-value never above, and no n-value is above its box's p-value — so every box above a
    passing leaf passes, and a plane dropped where the n-value is >= 0 stays satisfied below."""
    rng = np.random.default_rng(5)
    m = 200_000
    scale = 10.0 ** rng.uniform(-3, 3, size=(m, 1))
    c = rng.uniform(-1, 1, size=(m, 3)) * scale
    h_in = rng.random((m, 3)) * scale * 0.1
    grow_lo = rng.random((m, 3)) * scale * rng.choice([0.0, 1e-6, 0.5], size=(m, 3)); grow_hi = rng.random((m, 3)) * scale * rng.choice([0.0, 1e-6, 0.5], size=(m, 3))
    ilo, ihi = (c - h_in).astype(F32), (c + h_in).astype(F32)
    olo, ohi = np.minimum((c - h_in - grow_lo).astype(F32), ilo), np.maximum((c + h_in + grow_hi).astype(F32), ihi)
    lim = F32(1e3)
    ilo, ihi, olo, ohi = (np.clip(a, -lim, lim) for a in (ilo, ihi, olo, ohi))
    assert (olo <= ilo).all() and (ihi <= ohi).all() and (ilo <= ihi).all()
    nrm = rng.normal(size=(m, 3)).astype(F32)
    nrm[rng.random((m, 3)) < 0.1] = 0.0
    nrm[rng.random((m, 3)) < 0.02] = -0.0
    pl = np.zeros((m, 4), dtype=F32); pl[:, :3] = nrm
    s_p, s_n = pkg.cull_plane_values(pl, ilo, ihi)                   # with d = 0: the tangent offsets
    d = -np.where(rng.random(m) < 0.5, s_p, s_n)
    for _ in range(3):                                                # within three ulps either way
        step = rng.integers(-1, 2, size=m)
        d = np.where(step > 0, np.nextafter(d, F32(np.inf)), np.where(step < 0, np.nextafter(d, F32(-np.inf)), d)).astype(F32)
    pl[:, 3] = np.clip(d, -lim, lim)
    ip, in_ = pkg.cull_plane_values(pl, ilo, ihi)
    op, on = pkg.cull_plane_values(pl, olo, ohi)
    assert np.isfinite(ip).all() and np.isfinite(on).all()
    assert (np.abs(ip) < 1e-2 * np.maximum(np.abs(pl[:, 3]), 1e-3)).mean() > 0.3   # (near tangent: the values are a few ulps of the offsets)
    assert (op >= ip).all(), np.count_nonzero(op < ip)
    assert (on <= in_).all(), np.count_nonzero(on > in_)
    assert (in_ <= ip).all() and (on <= op).all()
    assert ((ip >= 0) & (op >= 0)).any() and (ip < 0).any() and ((in_ >= 0) != (ip >= 0)).any()


# ---- 2. exact boundaries ----------------------------------------------------------------------------------------------------------------------------------------

def test_exact_boundaries(pkg):
    box = np.array([[0.25, -3.0, 1.0, 0.7, 5.0, 2.0]], dtype=F32)
    hx = box[0, 3]
    off, hits = pkg.cull_brute_force([[(1.0, 0.0, 0.0, -hx)], [(1.0, 0.0, 0.0, -np.nextafter(hx, F32(np.inf)))], [(1.0, 0.0, 0.0, -box[0, 0])],
                                      [(1.0, 0.0, 0.0, -np.nextafter(box[0, 0], F32(np.inf)))]], box)
    assert off.tolist() == [0, 1, 1, 2, 3]                           # through the max face: s(p) = 0 passes; one ulp beyond: fails
    assert hits["straddle"].tolist() == [1, 0, 1]                    # through the min face: s(n) = 0, wholly inside; one ulp beyond: straddles
    # n.k = -0.0 selects hi for the p-vertex (-0.0 >= 0): with hi.x = +inf the product would be a NaN, but a +-0 coefficient contributes +0 whatever the
    # coordinate: s = d at both vertices, and the box passes wholly inside
    inf_box = np.array([[0.0, 0.0, 0.0, np.inf, 1.0, 1.0]], dtype=F32)
    s_p, s_n = pkg.cull_plane_values(np.array([-0.0, 0.0, 0.0, 1.0], dtype=F32), inf_box[0, :3], inf_box[0, 3:])
    assert s_p == 1.0 and s_n == 1.0
    s_p, s_n = pkg.cull_plane_values(np.array([0.0, 0.0, 0.0, 1.0], dtype=F32), inf_box[0, :3], inf_box[0, 3:])
    assert s_p == 1.0 and s_n == 1.0
    off, hits = pkg.cull_brute_force([[(-0.0, 0.0, 0.0, 1.0)]], inf_box)
    assert off.tolist() == [0, 1] and hits["straddle"].tolist() == [0]
    # a NaN in a plane, an inverted box and a box with a NaN pass nothing; the padding plane passes every finite box with its bit clear
    bad = np.array([[0, 0, 0, 1, 1, 1], [1, 0, 0, 0, 1, 1], [0, np.nan, 0, 1, 1, 1]], dtype=F32)
    off, hits = pkg.cull_brute_force([[PADDING], [(0.0, 0.0, np.nan, 1.0)], [(np.nan, 0.0, 0.0, 1.0)]], bad)
    assert off.tolist() == [0, 1, 1, 1] and hits["prim"].tolist() == [0] and hits["straddle"].tolist() == [0]
    # each product and each sum is rounded on its own: (a x + b y) + c z + d with a x + b y rounding away the low bits
    s_p, _ = pkg.cull_plane_values(np.array([1.0, 1.0, 1.0, -1.0], dtype=F32), np.array([1.0, 2.0 ** -24, 2.0 ** -24], dtype=F32), np.array([1.0, 2.0 ** -24, 2.0 ** -24], dtype=F32))
    assert s_p == 0.0                                                # (exactly: 2^-23; one rounding at the end: 2^-23 as well; rounded step by step: 0)


# ---- 3. the host walks on the oracle's trees ----------------------------------------------------------------------------------------------------------------

_FAMILY = {}


def family(pkg, name, per):
    """(volumes, (offsets, hits) of the brute force on the mesh's stage-E boxes) per mesh and plane count, computed once"""
    if (name, per) not in _FAMILY:
        tris = mesh(pkg, name)
        lo = np.minimum(np.minimum(tris["v1"], tris["v2"]), tris["v3"]); hi = np.maximum(np.maximum(tris["v1"], tris["v2"]), tris["v3"])
        leaf = as_boxes(np.concatenate([lo, hi], axis=1))
        vols = make_volumes(pkg, leaf, np.concatenate([tris["v1"], tris["v2"], tris["v3"]]), 17 + len(tris) + per, per)
        _FAMILY[(name, per)] = (vols, pkg.cull_brute_force(vols, leaf), leaf)
    return _FAMILY[(name, per)]


@pytest.mark.parametrize("name", WALK_MESHES + ["uniform_2", "uniform_3", "uniform_64", "uniform_65", "uniform_4096"])
def test_families_have_what_the_tests_need(pkg, name):
    n = len(mesh(pkg, name))
    for per in PLANE_COUNTS:
        vols, (off, hits), _ = family(pkg, name, per)
        assert vols.shape == (N_VOLUMES, per, 4) and off[-1] == len(hits)
        finite = vols[np.isfinite(vols)]
        assert np.abs(finite).max() <= 1e3 and np.isnan(vols).sum() == 1
        check_premises(off, hits, n, f"{name} x {per} planes")
        assert off[4] + 1 <= off[5] and off[6] - off[5] < off[5] - off[4], "the exact-boundary pair: the box on the plane passes, one ulp beyond it fails"


@pytest.mark.parametrize("name", WALK_MESHES)
def test_host_walks_equal_the_brute_force(pkg, orc, name):
    tris = mesh(pkg, name); n = len(tris)
    checked = 0
    for per in PLANE_COUNTS:
        vols, (off, hits), leaf = family(pkg, name, per)
        ref = slices_of(off, hits)
        pick = list(range(N_SPECIAL)) + list(range(N_SPECIAL, N_VOLUMES, 16 if n > 100 else 4))
        for algo in (0, 1, 2, 3):
            t = orc.build_tree(algo, tris)
            tree = Tree(t["nodes"], t["leaves"], t["root"], n, t["layout"])
            assert tree.leaf_boxes.tobytes() == leaf.tobytes()
            for i in pick:
                for masking in (False, True):
                    got, _ = lane_walk(pkg, tree, vols[i], masking)
                    assert got.tobytes() == ref[i].tobytes(), f"{name} algo {algo} volume {i} x {per}: lane walk, masking {masking}"
                got, peak = group_walk(pkg, tree, vols[i])
                assert by_prim(got).tobytes() == ref[i].tobytes(), f"{name} algo {algo} volume {i} x {per}: group walk"
                assert len(np.unique(got["prim"])) == len(got) and 1 <= peak <= max(n - 1, 1)
                checked += 1
    assert checked >= 4 * 3 * N_SPECIAL


def test_group_schedule_occupancy(pkg):
    """the schedule's occupancy on a tree made for it (fat_caterpillar: + 256 entries per round) passes BVH_CULL_GROUP_STACK at 32 levels (8448 entries) and does not at 31
    (8192: exactly full), and both answers equal the brute force — what tests/test_gpu_cull.py relies on for the group walk's hand-over to the stackless pass"""
    everything = np.array([PADDING], dtype=F32)
    for levels, over in ((32, True), (31, False)):
        leaf, nodes, root, n = fat_caterpillar(pkg, levels)
        tree = Tree(nodes, None, root, n, 0)
        got, peak = group_walk(pkg, tree, everything)
        assert (peak > pkg.CULL_GROUP_STACK) == over, (levels, peak)
        off, hits = pkg.cull_brute_force(everything, leaf)
        assert off[1] == n and by_prim(got).tobytes() == hits.tobytes()


# ---- 4. frustum_planes --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("zero_to_one", [True, False])
def test_frustum_planes_of_a_known_matrix(pkg, zero_to_one):
    """fovy 90 degrees, aspect 1, near 1, far 9, looking down -z: the frustum is |x| <= -z, |y| <= -z, 1 <= -z <= 9"""
    pl = pkg.frustum_planes(perspective(np.radians(90.0), 1.0, 1.0, 9.0, zero_to_one), depth_zero_to_one=zero_to_one)
    assert pl.shape == (6, 4) and pl.dtype == F32
    eps = 1e-3
    faces = {  # a point on each face (not on an edge) and the outward direction
        "left": ((-4.0, 0.5, -4.0), (-1.0, 0.0, 0.0)), "right": ((4.0, 0.5, -4.0), (1.0, 0.0, 0.0)), "bottom": ((0.5, -4.0, -4.0), (0.0, -1.0, 0.0)),
        "top": ((0.5, 4.0, -4.0), (0.0, 1.0, 0.0)), "near": ((0.25, 0.25, -1.0), (0.0, 0.0, 1.0)), "far": ((2.0, 2.0, -9.0), (0.0, 0.0, -1.0)),
    }
    for k, (name, (p, out)) in enumerate(faces.items()):
        p, out = np.array(p), np.array(out)
        s_in = pl[:, :3].astype(np.float64) @ (p - eps * out) + pl[:, 3]
        s_out = pl[:, :3].astype(np.float64) @ (p + eps * out) + pl[:, 3]
        assert (s_in > 0).all(), (name, s_in)
        assert s_out[k] < 0 and (np.delete(s_out, k) > 0).all(), (name, s_out)  # planes in the order left, right, bottom, top, near, far
    # the other convention's near plane on the same matrix is a different plane
    other = pkg.frustum_planes(perspective(np.radians(90.0), 1.0, 1.0, 9.0, zero_to_one), depth_zero_to_one=not zero_to_one)
    assert other[4].tobytes() != pl[4].tobytes() and np.delete(other, 4, axis=0).tobytes() == np.delete(pl, 4, axis=0).tobytes()
    # a view matrix moves the planes with the camera: the eye's own near-plane centre stays inside
    clip = perspective(np.radians(60.0), 1.5, 0.5, 50.0, zero_to_one) @ look_at((3.0, 4.0, 5.0), (0.0, 0.0, 0.0))
    pl = pkg.frustum_planes(clip, depth_zero_to_one=zero_to_one)
    fwd = -np.array([3.0, 4.0, 5.0]) / np.linalg.norm([3.0, 4.0, 5.0])
    for dist, inside in ((0.4, False), (0.6, True), (49.0, True), (51.0, False)):
        p = np.array([3.0, 4.0, 5.0]) + dist * fwd
        assert bool(((pl[:, :3].astype(np.float64) @ p + pl[:, 3]) >= 0).all()) == inside, dist


# ---- 5. the ABI ---------------------------------------------------------------------------------------------------------------------------------------------

def test_header_library_and_binding_agree(pkg):
    L = pkg.lib()
    assert hasattr(L, "bvh_cull") and "bvh_cull" in pkg.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    assert int(re.search(r"#define\s+BVH_CULL_MAX_PLANES\s+(\d+)", hdr).group(1)) == pkg.CULL_MAX_PLANES == 8
    assert int(re.search(r"#define\s+BVH_CULL_GROUP_STACK\s+(\d+)", hdr).group(1)) == pkg.CULL_GROUP_STACK
    assert re.search(r"BVH_CULL_AUTO = 0, BVH_CULL_LANE = 1, BVH_CULL_GROUP = 2", hdr) and (pkg.CULL_AUTO, pkg.CULL_LANE, pkg.CULL_GROUP) == (0, 1, 2)
    assert pkg.CULL_HIT.itemsize == 8 and pkg.CULL_HIT.names == ("prim", "straddle")
    # host-side argument checks come before any device work: no GPU is needed to be refused
    assert L.bvh_cull(None, None, None, 1, 6, 0, None, None, 0, None) == -10001
    with pytest.raises(pkg.BvhError):
        pkg.cull_brute_force(np.zeros((2, 9, 4), dtype=F32), np.zeros((1, 6), dtype=F32))
    off, hits = pkg.cull_brute_force(np.zeros((0, 6, 4), dtype=F32), np.zeros((1, 6), dtype=F32))
    assert off.tolist() == [0] and len(hits) == 0 and hits.dtype == pkg.CULL_HIT
