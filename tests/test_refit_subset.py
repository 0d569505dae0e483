"""CPU: bvh_refit_subset in the C ABI, the library, the Python binding and the C++ mirror, and the numpy restatement the GPU tests
(tests/test_gpu_refit_subset.py) compare against — itself checked against reference_refit on the oracle's trees."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_refit import reference_refit

GOLDEN = os.path.join(ROOT, "tests", "golden")


def reference_refit_subset(nodes, leaves, root, n, layout, prim_boxes_before, new_boxes, prims):
    """numpy restatement of bvh_refit_subset.  prims: the listed primitive indices (duplicates and indices >= n allowed).  For every distinct listed p < n:
    prim box p and the box of the leaf that holds p become new_boxes[p]; every internal node on a path from such a leaf to the root becomes the componentwise
    fmin / fmax of its two children's boxes, deepest level first — a child off the paths contributes the box it stores.  Every other record is copied through.
    nodes / leaves as bvh_download returns them.  Returns (nodes, leaves, prim_boxes, scene) — scene = the root's new box as (min, max)."""
    ni = n - 1
    nodes = nodes.copy()
    leaves = leaves.copy() if leaves is not None else None
    prim_boxes = prim_boxes_before.copy()
    prims = np.asarray(prims, dtype=np.uint32).ravel()
    listed = np.unique(prims[prims < n]).astype(np.int64)
    prim_boxes[listed] = new_boxes[listed]
    leaf_prim = (nodes["left"][ni:2 * ni + 1] if layout == 0 else leaves["prim"]).astype(np.int64)
    leaf_of_prim = np.full(n, -1, dtype=np.int64)
    ok = leaf_prim < n
    leaf_of_prim[leaf_prim[ok]] = np.nonzero(ok)[0]
    dirty_leaves = leaf_of_prim[listed]; held = dirty_leaves >= 0
    dirty_leaves, held_prims = dirty_leaves[held], listed[held]
    if layout == 0:
        nodes["min"][ni + dirty_leaves] = new_boxes["min"][held_prims]; nodes["max"][ni + dirty_leaves] = new_boxes["max"][held_prims]
        lo = nodes["min"].copy(); hi = nodes["max"].copy()
    else:
        leaves["min"][dirty_leaves] = new_boxes["min"][held_prims]; leaves["max"][dirty_leaves] = new_boxes["max"][held_prims]
        lo = np.concatenate([nodes["min"], leaves["min"]]); hi = np.concatenate([nodes["max"], leaves["max"]])
    left = nodes["left"][:ni].astype(np.int64); right = nodes["right"][:ni].astype(np.int64)
    parent = np.full(2 * n - 1, -1, dtype=np.int64)
    parent[left] = np.arange(ni); parent[right] = np.arange(ni)
    parent[root] = -1
    levels, frontier = [], np.array([root], dtype=np.int64)
    while frontier.size:
        levels.append(frontier)
        ch = np.concatenate([left[frontier], right[frontier]])
        frontier = ch[ch < ni]
    assert sum(len(lv) for lv in levels) == ni, "not a tree over n - 1 internal nodes"
    on_path = np.zeros(ni, dtype=bool)
    walk = np.unique(parent[ni + dirty_leaves])
    while walk.size:
        walk = walk[(walk >= 0) & ~on_path[np.maximum(walk, 0)]]      # (a node that is marked already: somebody walked on from there)
        on_path[walk] = True
        walk = np.unique(parent[walk])
    for lv in reversed(levels):
        lv = lv[on_path[lv]]
        lo[lv] = np.fmin(lo[left[lv]], lo[right[lv]]); hi[lv] = np.fmax(hi[left[lv]], hi[right[lv]])
    nodes["min"][:ni] = lo[:ni]; nodes["max"][:ni] = hi[:ni]
    return nodes, leaves, prim_boxes, (lo[root].copy(), hi[root].copy())


def dirty_path_mask(nodes, leaves, root, n, layout, prims):
    """(internal nodes on a dirty path bool[n-1], dirty leaves bool[n]) from the child links alone"""
    ni = n - 1
    prims = np.asarray(prims, dtype=np.uint32).ravel()
    listed = np.unique(prims[prims < n]).astype(np.int64)
    leaf_prim = (nodes["left"][ni:2 * ni + 1] if layout == 0 else leaves["prim"]).astype(np.int64)
    leaf_dirty = np.isin(leaf_prim, listed)
    left = nodes["left"][:ni].astype(np.int64); right = nodes["right"][:ni].astype(np.int64)
    parent = np.full(2 * n - 1, -1, dtype=np.int64)
    parent[left] = np.arange(ni); parent[right] = np.arange(ni); parent[root] = -1
    on_path = np.zeros(ni, dtype=bool)
    for j in np.nonzero(leaf_dirty)[0]:
        a = parent[ni + j]
        while a >= 0 and not on_path[a]:
            on_path[a] = True; a = parent[a]
    return on_path, leaf_dirty


def header_text():
    return open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()


def test_header_declares_and_library_exports_refit_subset(pkg):
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert re.search(r"\bint\s+bvh_refit_subset\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*bvh_result\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,"
                     r"\s*const uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*bvh_timings\s*\*\s*\w+\s*\)", text)
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_refit_subset")
    assert "bvh_refit_subset" in pkg.EXPORTS
    assert pkg.lib().bvh_refit_subset(None, None, None, None, 0, None) == -10001
    assert pkg.lib().bvh_refit_subset(None, None, None, None, 5, None) == -10001


def test_builder_classes_have_refit_subset(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "refit_subset"))
        with pytest.raises(pkg.BvhError):
            cls().refit_subset(np.array([0], dtype=np.uint32))        # no tree yet


def test_cpp_mirror_refit_subset_compiles(tmp_path):
    src = tmp_path / "refit_subset_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> void animate(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, std::vector<BvhConstruction::Triangle>& b,
                                   const std::vector<BvhConstruction::u32>& moved) {
    B bvh; bvh.build(ctx, a); bvh.refitSubset(ctx, b, moved); (void)bvh.m_cost;
}
void all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, std::vector<BvhConstruction::Triangle>& b, const std::vector<BvhConstruction::u32>& moved) {
    animate<BvhConstruction::TwoPassLbvh>(ctx, a, b, moved); animate<BvhConstruction::SinglePassLbvh>(ctx, a, b, moved);
    animate<BvhConstruction::PLOCNew>(ctx, a, b, moved); animate<BvhConstruction::HPLOC>(ctx, a, b, moved);
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _meshes(pkg):
    out = {name: pkg.meshgen.load_tri(os.path.join(GOLDEN, name + ".tri")) for name in ("cornell32", "cornell82", "cornell382")}
    out["uniform20000"] = pkg.meshgen.uniform(20_000, 5)
    return out


def _moved_boxes(boxes, seed):
    """other boxes for every primitive: the build's, shifted and grown by a random amount"""
    rng = np.random.default_rng(seed)
    out = boxes.copy()
    d = rng.normal(0.0, 0.05, out["min"].shape).astype(np.float32); g = np.abs(rng.normal(0.0, 0.02, out["min"].shape)).astype(np.float32)
    out["min"] = out["min"] + d - g; out["max"] = out["max"] + d + g
    return out


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_reference_refit_subset_agrees_with_reference_refit(pkg, orc, algo):
    """with the listed primitives' boxes replaced, a full reference refit of the oracle's tree and the subset restatement give the same bytes — and the subset
    restatement changes nothing off the dirty paths (checked on a tree whose off-path boxes are junk)"""
    for name, tris in _meshes(pkg).items():
        n = len(tris)
        t = orc.build_tree(algo, tris)
        nodes, leaves, root, layout, boxes = t["nodes"], t["leaves"], t["root"], t["layout"], t["boxes"]
        moved = _moved_boxes(boxes, n + algo)
        rng = np.random.default_rng(7 * n + algo)
        lists = {
            "one": np.array([n // 2], dtype=np.uint32),
            "all": np.arange(n, dtype=np.uint32),
            "some": rng.choice(n, max(1, n // 20), replace=False).astype(np.uint32),
        }
        some = lists["some"]
        lists["dups_and_bad"] = rng.permutation(np.concatenate([some, some, some, np.full(50, some[0], dtype=np.uint32),
                                                                np.array([n, n + 5, 0xFFFFFFFF], dtype=np.uint32)])).astype(np.uint32)
        results = {}
        for what, prims in lists.items():
            listed = np.unique(prims[prims < n])
            mixed = boxes.copy(); mixed[listed] = moved[listed]
            full_n, full_l = reference_refit(nodes, leaves, root, n, layout, mixed)
            got_n, got_l, got_b, scene = reference_refit_subset(nodes, leaves, root, n, layout, boxes, moved, prims)
            assert got_n.tobytes() == full_n.tobytes(), f"{name} {what}: nodes differ"
            if leaves is not None:
                assert got_l.tobytes() == full_l.tobytes(), f"{name} {what}: leaves differ"
            assert got_b.tobytes() == mixed.tobytes()
            assert np.array_equal(scene[0], full_n["min"][root]) and np.array_equal(scene[1], full_n["max"][root])
            results[what] = got_n.tobytes()
            # off the paths nothing is read-modified: junk stays junk, on the paths a box is the union of its children's current boxes
            on_path, leaf_dirty = dirty_path_mask(nodes, leaves, root, n, layout, prims)
            junk_n = nodes.copy(); junk_l = None if leaves is None else leaves.copy()
            junk_n["min"][:n - 1][~on_path] = 7.0; junk_n["max"][:n - 1][~on_path] = -7.0
            if layout == 0:
                junk_n["min"][n - 1:][~leaf_dirty] = 7.0; junk_n["max"][n - 1:][~leaf_dirty] = -7.0
            else:
                junk_l["min"][~leaf_dirty] = 7.0; junk_l["max"][~leaf_dirty] = -7.0
            j_n, j_l, _, _ = reference_refit_subset(junk_n, junk_l, root, n, layout, boxes, moved, prims)
            keep = np.concatenate([~on_path, ~leaf_dirty]) if layout == 0 else ~on_path
            assert j_n[keep].tobytes() == junk_n[keep].tobytes(), f"{name} {what}: an off-path node changed"
            if layout == 1:
                assert j_l[~leaf_dirty].tobytes() == junk_l[~leaf_dirty].tobytes(), f"{name} {what}: an off-path leaf changed"
            lo = j_n["min"] if layout == 0 else np.concatenate([j_n["min"], j_l["min"]])
            hi = j_n["max"] if layout == 0 else np.concatenate([j_n["max"], j_l["max"]])
            p = np.nonzero(on_path)[0]
            le, ri = j_n["left"][p].astype(np.int64), j_n["right"][p].astype(np.int64)
            assert np.array_equal(lo[p], np.fmin(lo[le], lo[ri])) and np.array_equal(hi[p], np.fmax(hi[le], hi[ri]))
        assert results["dups_and_bad"] == results["some"]
