"""CPU: the host side of bvh_build_many — the output layout helper against a direct numpy restatement, the binding's range validation, the host-side packing of
a list of meshes, and the header's declarations (tests/test_abi.py then checks that the library exports them)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.parametrize("counts", [[2], [2, 3, 4], [64, 65, 512, 513, 2], list(range(2, 200, 7))])
def test_many_layout_restated(pkg, counts):
    out_off, node_off, total = pkg.many_layout(counts)
    c = np.asarray(counts, dtype=np.int64)
    assert total == int(c.sum())
    for m in range(len(c)):
        assert out_off[m] == int(c[:m].sum())
        assert node_off[m] == 2 * int(c[:m].sum()) - m
        # mesh m's 2*count-1 records end where mesh m+1's begin; the last one ends at 2*total - n_meshes
        end = node_off[m] + 2 * int(c[m]) - 1
        assert end == (node_off[m + 1] if m + 1 < len(c) else 2 * total - len(c))


def test_many_layout_of_nothing(pkg):
    out_off, node_off, total = pkg.many_layout([])
    assert len(out_off) == 0 and len(node_off) == 0 and total == 0


def test_range_validation(pkg):
    ok = pkg.many_check_ranges([[0, 2], [2, 5], [10, 3]], 13)
    assert ok.dtype == pkg.MESH_RANGE and ok.itemsize == 8 and ok.flags["C_CONTIGUOUS"]
    assert ok["first"].tolist() == [0, 2, 10] and ok["count"].tolist() == [2, 5, 3]
    assert pkg.many_check_ranges(ok, 13).tobytes() == ok.tobytes()          # a MESH_RANGE array goes through as it is
    with pytest.raises(pkg.BvhError):
        pkg.many_check_ranges([], 10)                                       # no mesh
    with pytest.raises(pkg.BvhError):
        pkg.many_check_ranges([[0, 1]], 10)                                 # count < 2
    with pytest.raises(pkg.BvhError):
        pkg.many_check_ranges([[0, 4], [4, 0]], 10)
    with pytest.raises(pkg.BvhError):
        pkg.many_check_ranges([[8, 3]], 10)                                 # first + count > n_tris
    with pytest.raises(pkg.BvhError):
        pkg.many_check_ranges([[0xFFFFFFFE, 4]], 0xFFFFFFFF)                # ... also where a 32-bit sum would wrap
    assert len(pkg.many_check_ranges([[0xFFFFFFF0, 15]], 0xFFFFFFFF)) == 1
    with pytest.raises(pkg.BvhError):
        pkg.many_check_ranges([[0, 4], [6, 4]], 16, pkg.TRI_PACKED36)       # a PACKED36 first that is no multiple of 4
    assert len(pkg.many_check_ranges([[0, 4], [6, 4]], 16, pkg.TRI_PADDED64)) == 2
    assert len(pkg.many_check_ranges([[0, 3], [8, 5]], 16, pkg.TRI_PACKED36)) == 2
    with pytest.raises(pkg.BvhError):
        pkg.many_check_ranges([[0, 2 ** 29], [0, 2 ** 29]], 2 ** 29)        # total >= 2^30 (meshes may share triangles)
    with pytest.raises(pkg.BvhError):
        pkg.many_check_ranges([[-1, 4]], 16)


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_host_meshes_are_laid_out_per_format(pkg, fmt):
    t = pkg.meshgen.uniform(30, 5)
    meshes = [t[:3], t[3:10], t[10:30]]
    host, ranges, n_tris = pkg._many_host_input(meshes, fmt)
    r = pkg.many_check_ranges(ranges, n_tris, fmt)
    assert r["count"].tolist() == [3, 7, 20]
    for m, mesh in enumerate(meshes):
        f, c = int(r["first"][m]), int(r["count"][m])
        want = np.concatenate([mesh["v1"], mesh["v2"], mesh["v3"]], axis=1)
        if fmt == pkg.TRI_PADDED64:
            got = np.concatenate([host["tris"]["v1"][f:f + c], host["tris"]["v2"][f:f + c], host["tris"]["v3"][f:f + c]], axis=1)
        elif fmt == pkg.TRI_PACKED36:
            assert f % 4 == 0 and host["tris"].dtype == np.float32 and host["tris"].shape[1] == 9
            got = host["tris"][f:f + c]
        else:
            idx = host["indices"].reshape(-1, 3)[f:f + c]
            got = host["vertices"][idx].reshape(c, 9)
        assert got.tobytes() == want.tobytes()
    with pytest.raises(pkg.BvhError):
        pkg._many_host_input([np.zeros(4, dtype=np.float32)], fmt)


def test_header_declares_the_entry_points(pkg):
    text = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+bvh_build_many\s*\(\s*bvh_ctx\s*\*", code)
    assert re.search(r"\bint\s+bvh_many_tree\s*\(\s*bvh_algo\b", code)
    assert re.search(r"#define\s+BVH_MANY_LDS_MAX_PRIMS\s+512\b", code) and pkg.MANY_LDS_MAX_PRIMS == 512
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+first\s*,\s*count\s*;\s*\}\s*bvh_mesh_range\s*;", code)
    assert int(re.search(r"#define\s+BVH_ABI_VERSION\s+(\d+)", text).group(1)) == 4            # no struct changed size, no signature changed
    assert "bvh_build_many" in pkg.EXPORTS and "bvh_many_tree" in pkg.EXPORTS
    assert C.sizeof(pkg.ManyOut) == 48 and pkg.MESH_RANGE.itemsize == 8


def test_many_tree_is_host_arithmetic(pkg):
    """bvh_many_tree needs no context and no device: slices of made-up addresses, per format; its rejections"""
    L = pkg.lib()
    counts = [5, 64, 700, 2]
    out_off, node_off, total = pkg.many_layout(counts)
    base = {"nodes": 0x10000000, "boxes": 0x20000000, "scenes": 0x30000000, "roots": 0x40000000, "keys": 0x50000000, "vals": 0x60000000}
    out = pkg.ManyOut(base["nodes"], base["boxes"], base["scenes"], base["roots"], base["keys"], base["vals"])
    roots = np.array([3, 17, 0, 0], dtype=np.uint32)
    for fmt in (0, 1, 2):
        firsts = [0, 8, 100, 1000]
        ranges = pkg.many_check_ranges(list(zip(firsts, counts)), 2000, fmt)
        inp = pkg.BuildInput(fmt, 30, 0x70000000 if fmt != 2 else None, 0x71000000 if fmt == 2 else None, 0x72000000 if fmt == 2 else None, 99 if fmt == 2 else 0, 0)
        for algo in (0, 1):
            for m in range(4):
                r, t = pkg.Result(), pkg.BuildInput()
                rc = L.bvh_many_tree(algo, C.byref(inp), ranges.ctypes.data, 4, C.byref(out), m, roots.ctypes.data if algo == 1 else None, C.byref(r), C.byref(t))
                assert rc == 0
                assert r.d_nodes == base["nodes"] + 32 * int(node_off[m]) and r.d_prim_aabbs == base["boxes"] + 24 * int(out_off[m])
                assert r.d_scene_extent == base["scenes"] + 24 * m and r.d_sorted_keys == base["keys"] + 4 * int(out_off[m]) and r.d_sorted_vals == base["vals"] + 4 * int(out_off[m])
                assert (r.root, r.n_internal, r.n_leaves, r.layout, r.key_bits) == (int(roots[m]) if algo == 1 else 0, counts[m] - 1, counts[m], 0, 32)
                assert r.d_leaves is None and r.d_morton_keys is None and t.tri_format == fmt and t.morton_bits == 30
                if fmt == 0:
                    assert t.d_tris == 0x70000000 + 64 * firsts[m] == r.d_tris
                elif fmt == 1:
                    assert t.d_tris == 0x70000000 + 36 * firsts[m] and r.d_tris is None
                else:
                    assert t.d_indices == 0x72000000 + 12 * firsts[m] and t.d_vertices == 0x71000000 and t.n_vertices == 99 and r.d_tris is None
        r, t = pkg.Result(), pkg.BuildInput()
        args = (C.byref(inp), ranges.ctypes.data, 4, C.byref(out))
        assert L.bvh_many_tree(1, *args, 4, roots.ctypes.data, C.byref(r), C.byref(t)) == -10001          # m >= n_meshes
        assert L.bvh_many_tree(1, *args, 0, None, C.byref(r), C.byref(t)) == -10001                       # single-pass needs the roots
        assert L.bvh_many_tree(3, *args, 0, roots.ctypes.data, C.byref(r), C.byref(t)) == -10001          # not an LBVH builder
        assert L.bvh_many_tree(0, *args, 0, None, None, C.byref(t)) == -10001
        assert L.bvh_many_tree(0, None, ranges.ctypes.data, 4, C.byref(out), 0, None, C.byref(r), C.byref(t)) == -10001
