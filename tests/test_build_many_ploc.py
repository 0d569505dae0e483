"""CPU: the host side of bvh_build_many_ploc — the header's declarations, the output layout helper on a hand-computed case, the binding's structure, the
exported symbols, and bvh_many_ploc_tree (host arithmetic only: it needs neither a context nor a device) on made-up addresses with its rejections."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

E_INVALID = -10001


def test_header_declares_the_entry_points(pkg):
    text = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+bvh_build_many_ploc\s*\(\s*bvh_ctx\s*\*", code)
    assert re.search(r"\bint\s+bvh_many_ploc_tree\s*\(\s*bvh_algo\b", code)
    assert re.search(r"typedef\s+struct\s*\{[^}]*\bd_nodes\b[^}]*\bd_leaves\b[^}]*\bd_prim_aabbs\b[^}]*\bd_scene_extents\b[^}]*\bd_sorted_keys\b[^}]*\bd_sorted_vals\b[^}]*\}\s*bvh_many_ploc_out\s*;", code)
    assert int(re.search(r"#define\s+BVH_ABI_VERSION\s+(\d+)", text).group(1)) == 4            # no struct changed size, no signature changed
    assert re.search(r"\bint\s+bvh_build_many\s*\(\s*bvh_ctx\s*\*", code) and re.search(r"\}\s*bvh_many_out\s*;", code)      # the LBVH call is still there
    assert "bvh_build_many_ploc" in pkg.EXPORTS and "bvh_many_ploc_tree" in pkg.EXPORTS


def test_many_ploc_layout_by_hand(pkg):
    out_off, node_off, total = pkg.many_ploc_layout([3, 5, 2, 64])
    # mesh:          0  1  2   3      leaves start at the sum of the earlier counts; n-1 nodes each: 2, 4, 1, 63 -> node starts 0, 2, 6, 7 = out_off - m
    assert out_off.tolist() == [0, 3, 8, 10] and node_off.tolist() == [0, 2, 6, 7] and total == 74
    assert int(node_off[3]) + 63 == total - 4                               # the node array holds total - n_meshes records


def test_many_ploc_layout_of_nothing(pkg):
    out_off, node_off, total = pkg.many_ploc_layout([])
    assert len(out_off) == 0 and len(node_off) == 0 and total == 0


def test_many_ploc_out_is_six_pointers(pkg):
    assert C.sizeof(pkg.ManyPlocOut) == 48
    assert [f[0] for f in pkg.ManyPlocOut._fields_] == ["d_nodes", "d_leaves", "d_prim_aabbs", "d_scene_extents", "d_sorted_keys", "d_sorted_vals"]
    assert all(getattr(pkg.ManyPlocOut, f).offset == 8 * k for k, (f, _) in enumerate(pkg.ManyPlocOut._fields_))


def test_library_exports_both_symbols(pkg):
    raw = C.CDLL(pkg.LIB_PATH)
    assert hasattr(raw, "bvh_build_many_ploc") and hasattr(raw, "bvh_many_ploc_tree")


def test_many_ploc_tree_is_host_arithmetic(pkg):
    L = pkg.lib()
    counts = [5, 64, 700, 2]
    out_off, node_off, total = pkg.many_ploc_layout(counts)
    base = {"nodes": 0x10000000, "leaves": 0x18000000, "boxes": 0x20000000, "scenes": 0x30000000, "keys": 0x50000000, "vals": 0x60000000}
    out = pkg.ManyPlocOut(base["nodes"], base["leaves"], base["boxes"], base["scenes"], base["keys"], base["vals"])
    firsts = [0, 8, 100, 1000]
    for fmt in (0, 1, 2):
        ranges = pkg.many_check_ranges(list(zip(firsts, counts)), 2000, fmt)
        inp = pkg.BuildInput(fmt, 30, 0x70000000 if fmt != 2 else None, 0x71000000 if fmt == 2 else None, 0x72000000 if fmt == 2 else None, 99 if fmt == 2 else 0, 0)
        for m in range(4):
            r, t = pkg.Result(), pkg.BuildInput()
            assert L.bvh_many_ploc_tree(pkg.ALGO_PLOCPP, C.byref(inp), ranges.ctypes.data, 4, C.byref(out), m, C.byref(r), C.byref(t)) == 0
            assert r.d_nodes == base["nodes"] + 32 * int(node_off[m]) and r.d_leaves == base["leaves"] + 28 * int(out_off[m])
            assert r.d_prim_aabbs == base["boxes"] + 24 * int(out_off[m]) and r.d_scene_extent == base["scenes"] + 24 * m
            assert r.d_sorted_keys == base["keys"] + 4 * int(out_off[m]) and r.d_sorted_vals == base["vals"] + 4 * int(out_off[m])
            assert (r.root, r.n_internal, r.n_leaves, r.layout, r.key_bits) == (0, counts[m] - 1, counts[m], 1, 32)
            assert r.d_morton_keys is None and t.tri_format == fmt and t.morton_bits == 30
            if fmt == 0:
                assert t.d_tris == 0x70000000 + 64 * firsts[m] == r.d_tris
            elif fmt == 1:
                assert t.d_tris == 0x70000000 + 36 * firsts[m] and r.d_tris is None
            else:
                assert t.d_indices == 0x72000000 + 12 * firsts[m] and t.d_vertices == 0x71000000 and t.n_vertices == 99 and r.d_tris is None
        # without the optional arrays the slices name none
        bare = pkg.ManyPlocOut(base["nodes"], base["leaves"], base["boxes"], base["scenes"], None, None)
        r, t = pkg.Result(), pkg.BuildInput()
        assert L.bvh_many_ploc_tree(2, C.byref(inp), ranges.ctypes.data, 4, C.byref(bare), 2, C.byref(r), C.byref(t)) == 0
        assert r.d_sorted_keys is None and r.d_sorted_vals is None


def test_many_ploc_tree_rejections(pkg):
    L = pkg.lib()
    ranges = pkg.many_check_ranges([[0, 5], [8, 64]], 100)
    inp = pkg.BuildInput(0, 30, 0x70000000, None, None, 0, 0)
    out = pkg.ManyPlocOut(0x10000000, 0x18000000, 0x20000000, 0x30000000, None, None)
    r, t = pkg.Result(), pkg.BuildInput()
    args = (C.byref(inp), ranges.ctypes.data, 2, C.byref(out))
    assert L.bvh_many_ploc_tree(2, *args, 1, C.byref(r), C.byref(t)) == 0
    assert L.bvh_many_ploc_tree(2, *args, 2, C.byref(r), C.byref(t)) == E_INVALID                        # m >= n_meshes
    assert L.bvh_many_ploc_tree(2, *args, 0xFFFFFFFF, C.byref(r), C.byref(t)) == E_INVALID
    for algo in (0, 1, 3, 7):                                                                           # BVH_PLOCPP only
        assert L.bvh_many_ploc_tree(algo, *args, 0, C.byref(r), C.byref(t)) == E_INVALID
    assert L.bvh_many_ploc_tree(2, *args, 0, None, C.byref(t)) == E_INVALID
    assert L.bvh_many_ploc_tree(2, *args, 0, C.byref(r), None) == E_INVALID
    assert L.bvh_many_ploc_tree(2, None, ranges.ctypes.data, 2, C.byref(out), 0, C.byref(r), C.byref(t)) == E_INVALID
    no_leaves = pkg.ManyPlocOut(0x10000000, None, 0x20000000, 0x30000000, None, None)
    assert L.bvh_many_ploc_tree(2, C.byref(inp), ranges.ctypes.data, 2, C.byref(no_leaves), 0, C.byref(r), C.byref(t)) == E_INVALID
    wide = pkg.BuildInput(0, 60, 0x70000000, None, None, 0, 0)
    assert L.bvh_many_ploc_tree(2, C.byref(wide), ranges.ctypes.data, 2, C.byref(out), 0, C.byref(r), C.byref(t)) == E_INVALID
