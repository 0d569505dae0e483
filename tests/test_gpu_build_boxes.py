"""bvh_build_boxes on the GPU: a tree built from the boxes stage E wrote for some triangles is byte-identical to the tree bvh_build_ex builds from those
triangles (nodes, leaves, root, sorted keys and values), for every builder, both key widths and every scheduler."""
import ctypes as C

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

SIZES = [2, 3, 63, 64, 65, 1000, 262_144]
_MESH = {}


def mesh(pkg, n):
    if n not in _MESH:
        _MESH[n] = pkg.meshgen.sponza_like(n, 3) if n >= 262_144 else pkg.meshgen.uniform(n, 11 + n % 7)
    return _MESH[n]


def tree_of(b):
    d = b.download()
    return b.checksum(), d["root"], d["sorted_keys"], d["sorted_vals"]


def check_identical(pkg, ctx, algo, n, bits):
    tris = mesh(pkg, n)
    d_tris = ctx.upload(tris)
    boxes = ctx.alloc(n * pkg.AABB.itemsize)
    try:
        a = pkg.BUILDERS[algo]().build_ex(ctx, n, tris=d_tris, morton_bits=bits)
        ref = tree_of(a)
        assert pkg.lib().bvh_dev_copy(ctx.handle, boxes.ptr, a.result.d_prim_aabbs, n * pkg.AABB.itemsize) == 0
        b = pkg.BUILDERS[algo]().build_boxes(ctx, boxes, n=n, morton_bits=bits)
        got = tree_of(b)
        assert b.result.d_tris is None and b.result.key_bits == (64 if bits == 60 else 32)
        assert got[0] == ref[0] and got[1] == ref[1], f"algo {algo} n {n} bits {bits}: tree differs"
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), f"algo {algo} n {n} bits {bits}: sorted keys / values differ"
    finally:
        d_tris.free(); boxes.free()


@pytest.mark.parametrize("bits", [30, 60])
@pytest.mark.parametrize("algo", [0, 1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_boxes_give_the_triangle_tree(pkg, ctx, algo, n, bits):
    check_identical(pkg, ctx, algo, n, bits)


@pytest.mark.parametrize("opt,value,algos", [("hploc", 1, [3]), ("hploc", 2, [3]), ("lbvh", 1, [0, 1]), ("lbvh", 2, [0, 1])])
def test_boxes_give_the_triangle_tree_2m_schedulers(pkg, ctx, sched_opts, opt, value, algos):
    sched_opts(**{opt: value})
    for algo in algos:
        check_identical(pkg, ctx, algo, 2_000_000, 30)


def test_boxes_in_place_and_host_boxes(pkg, ctx):
    """d_boxes may be the ctx's own d_prim_aabbs; a host AABB array goes through the binding's upload"""
    tris = mesh(pkg, 1000)
    a = pkg.HPLOC().build(ctx, tris)
    ref = tree_of(a)
    host = np.empty(1000, dtype=pkg.AABB)
    assert pkg.lib().bvh_dev_download(ctx.handle, host.ctypes.data, a.result.d_prim_aabbs, host.nbytes) == 0
    b = pkg.HPLOC().build_boxes(ctx, a.result.d_prim_aabbs, n=1000)
    assert tree_of(b)[0] == ref[0]
    c = pkg.HPLOC().build_boxes(ctx, host)
    assert tree_of(c)[0] == ref[0]


def test_build_boxes_errors(pkg, ctx):
    L = pkg.lib()
    r = pkg.Result()
    buf = ctx.alloc(64 * 24)
    try:
        assert L.bvh_build_boxes(ctx.handle, 3, None, 64, 30, C.byref(r), None) == -10001
        assert L.bvh_build_boxes(ctx.handle, 3, buf.ptr, 1, 30, C.byref(r), None) == -10001
        assert L.bvh_build_boxes(ctx.handle, 4, buf.ptr, 64, 30, C.byref(r), None) == -10001
        assert L.bvh_build_boxes(ctx.handle, 3, buf.ptr, 64, 32, C.byref(r), None) == -10001
        assert L.bvh_build_boxes(ctx.handle, 3, buf.ptr, 64, 30, None, None) == -10001
    finally:
        buf.free()
