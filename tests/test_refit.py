"""CPU: bvh_refit / bvh_refit_ex in the C ABI, the library and the C++ mirror, and the numpy reference refit the GPU refit tests
(tests/test_gpu_refit.py) compare against — itself checked against the oracle's trees."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


def reference_refit(nodes, leaves, root, n, layout, prim_boxes):
    """numpy restatement of bvh_refit: leaf box = prim_boxes[leaf's prim], internal box = componentwise fmin / fmax of its children's boxes, unioned
    deepest level first.  nodes / leaves as bvh_download returns them (BVH2_NODE / PRIMREF, layout 0 or 1).  Returns new (nodes, leaves)."""
    ni = n - 1
    nodes = nodes.copy()
    leaves = leaves.copy() if leaves is not None else None
    if layout == 0:
        prim = nodes["left"][ni:2 * ni + 1]
        nodes["min"][ni:] = prim_boxes["min"][prim]; nodes["max"][ni:] = prim_boxes["max"][prim]
        lo = nodes["min"].copy(); hi = nodes["max"].copy()
    else:
        prim = leaves["prim"]
        leaves["min"] = prim_boxes["min"][prim]; leaves["max"] = prim_boxes["max"][prim]
        lo = np.concatenate([nodes["min"], leaves["min"]]); hi = np.concatenate([nodes["max"], leaves["max"]])
    left = nodes["left"][:ni].astype(np.int64); right = nodes["right"][:ni].astype(np.int64)
    levels, frontier = [], np.array([root], dtype=np.int64)     # internal nodes by depth (the children's parents, from the child links)
    while frontier.size:
        levels.append(frontier)
        ch = np.concatenate([left[frontier], right[frontier]])
        frontier = ch[ch < ni]
    assert sum(len(lv) for lv in levels) == ni, "not a tree over n - 1 internal nodes"
    for lv in reversed(levels):
        lo[lv] = np.fmin(lo[left[lv]], lo[right[lv]]); hi[lv] = np.fmax(hi[left[lv]], hi[right[lv]])
    nodes["min"][:ni] = lo[:ni]; nodes["max"][:ni] = hi[:ni]
    return nodes, leaves


def header_text():
    return open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()


def test_header_declares_and_library_exports_refit(pkg):
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert re.search(r"\bint\s+bvh_refit\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*bvh_result\s*\*\s*\w+\s*,\s*const void\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*bvh_timings\s*\*", text)
    assert re.search(r"\bint\s+bvh_refit_ex\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*bvh_result\s*\*\s*\w+\s*,\s*const bvh_build_input\s*\*\s*\w+\s*,\s*bvh_timings\s*\*", text)
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_refit") and hasattr(L, "bvh_refit_ex")
    assert "bvh_refit" in pkg.EXPORTS and "bvh_refit_ex" in pkg.EXPORTS
    lib = pkg.lib()
    assert lib.bvh_refit(None, None, None, 0, None) == -10001 and lib.bvh_refit_ex(None, None, None, None) == -10001


def test_builder_classes_have_refit(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "refit")) and callable(getattr(cls, "refit_ex"))
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().refit(pkg.meshgen.uniform(8, 1))           # no tree yet


def test_cpp_mirror_refit_compiles(tmp_path):
    src = tmp_path / "refit_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> void animate(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, std::vector<BvhConstruction::Triangle>& b) {
    B bvh; bvh.build(ctx, a); bvh.refit(ctx, b); (void)bvh.m_cost;
}
void all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, std::vector<BvhConstruction::Triangle>& b) {
    animate<BvhConstruction::TwoPassLbvh>(ctx, a, b); animate<BvhConstruction::SinglePassLbvh>(ctx, a, b);
    animate<BvhConstruction::PLOCNew>(ctx, a, b); animate<BvhConstruction::HPLOC>(ctx, a, b);
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _meshes(pkg):
    out = {name: pkg.meshgen.load_tri(os.path.join(GOLDEN, name + ".tri")) for name in ("cornell32", "cornell82", "cornell382")}
    out["uniform20000"] = pkg.meshgen.uniform(20_000, 5)
    return out


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_reference_refit_reproduces_oracle_trees(pkg, orc, algo):
    """refitting the oracle's own tree with the oracle's own primitive boxes returns the oracle's node / leaf arrays exactly: the union order does not
    matter and the leaf boxes are the build's"""
    for name, tris in _meshes(pkg).items():
        n = len(tris)
        t = orc.build_tree(algo, tris)
        nodes, leaves = t["nodes"], t["leaves"]
        # start from scrambled boxes: everything must come from the refit
        junk_n = nodes.copy(); junk_n["min"] = 7.0; junk_n["max"] = -7.0
        junk_l = None
        if leaves is not None:
            junk_l = leaves.copy(); junk_l["min"] = 7.0; junk_l["max"] = -7.0
        got_n, got_l = reference_refit(junk_n, junk_l, t["root"], n, t["layout"], t["boxes"])
        assert got_n.tobytes() == nodes.tobytes(), f"{name}: nodes differ"
        if leaves is not None:
            assert got_l.tobytes() == leaves.tobytes(), f"{name}: leaves differ"
