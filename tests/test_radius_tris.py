"""CPU: bvh_radius_tris in the C ABI, the library, the Python binding and the C++ mirror; the brute force that the GPU tests (tests/test_gpu_radius_tris.py)
compare against — every query triangle against every tree triangle through test_closest_tris.pair_matrix (the numpy restatement of dist2(X, Y) and feature),
the acceptance dist2 <= r2, the self-mode rule j > i, BVH_RADIUS_TRIS_SKIP_SHARED restated as IEEE == on whole vertices, slices in ascending (dist2, prim)
order — the checker of single records, and rule cases whose answers are exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_closest_tris import CROSSING, CTriHit, E_INVALID, box_gap2_f64, pair_matrix, query_ok, radius2, tri_tri_formula, tris_brute_force
from test_intersect_tris import as_triangles, stage_e_boxes, xyz

F32 = np.float32
F64 = np.float64
NAN = float("nan")


# ---- the brute force -----------------------------------------------------------------------------------------------------------------------------------------

def shared_vertex(x, y):
    """pair by pair: does any vertex of X_k equal any vertex of Y_k on all three coordinates under IEEE == (-0 equals +0, a NaN equals nothing)"""
    x, y = xyz(x), xyz(y)
    with np.errstate(invalid="ignore"):
        return (x[:, :, None, :] == y[:, None, :, :]).all(axis=-1).any(axis=(1, 2))


def shared_matrix(queries, tris, chunk=256):
    """(m, n) bool: shared_vertex of every query triangle against every tree triangle"""
    q, t = xyz(queries), xyz(tris)
    out = np.empty((len(q), len(t)), dtype=bool)
    with np.errstate(invalid="ignore"):
        for s in range(0, len(q), chunk):
            out[s:s + chunk] = (q[s:s + chunk, None, :, None, :] == t[None, :, None, :, :]).all(axis=-1).any(axis=(2, 3))
    return out


def accepted_matrix(queries, tris, radius, pairs, self_pairs=False, skip_shared=False):
    """(m, n) bool: the pairs the contract reports — dist2 <= r2 on live queries, in self mode j > i and, with skip_shared, no vertex in common"""
    d2 = pairs[0]
    with np.errstate(invalid="ignore"):
        acc = (d2 <= radius2(radius)) & query_ok(queries, radius)[:, None]
    if self_pairs:
        assert d2.shape[0] == d2.shape[1]
        acc &= np.triu(np.ones(d2.shape, dtype=bool), k=1)
        if skip_shared:
            acc &= ~shared_matrix(queries, tris)
    else:
        assert not skip_shared
    return acc


def radius_tris_brute_force(pkg, queries, tris, radius, pairs=None, self_pairs=False, skip_shared=False):
    """every query triangle against every tree triangle.  Returns dict: offsets (u32[m + 1]), hits (TRI_HIT[total], each slice in ascending (dist2, prim)
    order), counts, well (bool[m]: EVERY accepted pair of the query has the f64 squared gap of its two grown stage-E boxes <= its dist2; an empty slice is
    well-conditioned), ill_pairs (how many accepted pairs fail that).  pairs: pair_matrix(queries, tris), when the caller keeps it across radii"""
    d2, feat = pairs if pairs is not None else pair_matrix(queries, tris)
    acc = accepted_matrix(queries, tris, radius, (d2, feat), self_pairs, skip_shared)
    m = len(d2)
    rows, cols = np.nonzero(acc)
    d = d2[rows, cols]
    assert not np.isnan(d).any() and not np.signbit(d).any()          # an accepted dist2 is never NaN or negative (so the u64 key order is this order)
    order = np.lexsort((cols, d, rows))
    rows, cols, d = rows[order], cols[order], d[order]
    hits = np.zeros(len(rows), dtype=pkg.TRI_HIT)
    hits["dist2"], hits["prim"], hits["feature"] = d, cols, feat[rows, cols]
    counts = acc.sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    well = np.ones(m, dtype=bool)
    ill = 0
    if len(rows):
        bq, bt = stage_e_boxes(xyz(queries)), stage_e_boxes(xyz(tris))
        bad = ~(box_gap2_f64(bq[rows], bt[cols]) <= d.astype(F64))
        ill = int(bad.sum())
        well[np.unique(rows[bad])] = False
    return {"offsets": offsets, "hits": hits, "counts": counts, "well": well, "ill_pairs": ill}


def recompute_records(pkg, queries, tris, radius, offsets, hits, self_pairs=False, skip_shared=False):
    """None if (offsets, hits) is a well-formed answer whose every record is an accepted candidate of its prim — bit-equal dist2, the same feature, reserved 0,
    no prim twice in a slice, j > i in self mode and no shared vertex with skip_shared — otherwise a sentence saying what is wrong"""
    q, t = xyz(queries), xyz(tris)
    off = offsets.astype(np.int64)
    if len(off) != len(q) + 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != len(hits):
        return "the offsets are not a scan that ends at the number of records"
    rows = np.repeat(np.arange(len(q)), np.diff(off))
    pr = hits["prim"].astype(np.int64)
    if (pr >= len(t)).any():
        return "a prim out of range"
    if len(np.unique(rows * len(t) + pr)) != len(pr):
        return "a prim twice in one slice"
    if self_pairs and (pr <= rows).any():
        return "self mode reports a pair with j <= i"
    if (hits["reserved"] != 0).any():
        return "a reserved word is not 0"
    if len(pr) == 0:
        return None
    d, f = tri_tri_formula(q[rows], t[pr])
    with np.errstate(invalid="ignore"):
        acc = (d <= radius2(radius)) & query_ok(q, radius)[rows]
    if not acc.all():
        return f"{np.count_nonzero(~acc)} records are not accepted candidates"
    if (d.view(np.uint32) != hits["dist2"].view(np.uint32)).any():
        return "a dist2 is not bit-equal to its candidate's"
    if (f != hits["feature"]).any():
        return "a feature differs from its candidate's"
    if skip_shared and shared_vertex(q[rows], t[pr]).any():
        return "a pair that shares a vertex is reported"
    return None


def slices(bf):
    o = bf["offsets"].astype(np.int64)
    return [bf["hits"][o[i]:o[i + 1]] for i in range(len(o) - 1)]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_entry_point_and_flags(pkg):
    full = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    ptr = r"\s*\*\s*\w+\s*,\s*"
    assert re.search(r"\bint\s+bvh_radius_tris\s*\(\s*bvh_ctx" + ptr + "const bvh_result" + ptr + "const bvh_build_input" + ptr + "const bvh_build_input" + ptr +
                     r"uint32_t\s+\w+\s*,\s*float\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t" + ptr + "bvh_tri_hit" + ptr +
                     r"uint64_t\s+\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", text)
    for name, value in (("SORTED", 1), ("SELF", 2), ("SKIP_SHARED", 4)):
        assert re.search(rf"#define BVH_RADIUS_TRIS_{name}\s+{value}u\b", text)
        assert getattr(pkg, "RADIUS_TRIS_" + name) == value
    assert "#define BVH_ABI_VERSION 4" in text
    assert "-0 equals +0 and a NaN equals nothing" in full and "the bound never shrinks" in full       # the contract is in the header


def test_library_exports_radius_tris(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_radius_tris") and "bvh_radius_tris" in pkg.EXPORTS
    f = pkg.lib().bvh_radius_tris
    assert len(f.argtypes) == 11 and f.argtypes[5] is C.c_float and f.argtypes[6] is C.c_uint32 and f.argtypes[9] is C.c_uint64 and f.restype is C.c_int
    assert C.sizeof(CTriHit) == 16 and pkg.TRI_HIT.itemsize == 16
    assert pkg.lib().bvh_abi_version() == 4 and pkg.ABI_VERSION == 4
    assert b"0.4" in pkg.lib().bvh_version()


def test_radius_tris_errors_without_a_device(pkg):
    lib = pkg.lib()
    total = C.c_uint64(77)
    assert lib.bvh_radius_tris(None, None, None, None, 0, 1.0, 0, None, None, 0, None) == E_INVALID
    r = pkg.Result(); r.n_leaves = 4; r.layout = 0; r.d_nodes = 64; r.d_tris = 1 << 20
    q = pkg.BuildInput(pkg.TRI_PADDED64, 30, 1 << 21, None, None, 0, 0)
    S, SELF, SKIP = pkg.RADIUS_TRIS_SORTED, pkg.RADIUS_TRIS_SELF, pkg.RADIUS_TRIS_SKIP_SHARED

    def call(queries=q, k=4, flags=S, off=4096, hits=8192, cap=16):
        return lib.bvh_radius_tris(None, C.byref(r), None, C.byref(queries) if queries is not None else None, k, 1.0, flags, off, hits, cap, C.byref(total))
    assert call() == E_INVALID                                          # NULL ctx
    assert call(off=None) == E_INVALID                                  # NULL d_offsets
    assert call(flags=8) == E_INVALID and call(flags=S | 16) == E_INVALID          # an unknown flag bit
    assert call(flags=SKIP) == E_INVALID                                # SKIP_SHARED without SELF
    assert call(queries=None) == E_INVALID                              # NULL queries without SELF
    assert call(flags=SELF) == E_INVALID                                # queries given with SELF
    assert call(queries=None, flags=SELF | SKIP, k=5) == E_INVALID      # SELF with n_queries != n_leaves
    assert call(k=1 << 30) == E_INVALID                                 # too many queries
    assert call(hits=4096 + 8) == E_INVALID                             # d_hits over d_offsets
    assert call(k=0) == E_INVALID                                       # NULL ctx comes before n_queries == 0
    assert total.value == 77                                            # an error writes nothing


def test_builder_classes_have_radius_tris(pkg):
    for cls in pkg.BUILDERS.values():
        assert callable(getattr(cls, "radius_tris"))
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().radius_tris(np.zeros(4, dtype=pkg.meshgen.TRIANGLE), radius=1.0)       # no tree yet
    with pytest.raises(pkg.BvhError):
        pkg.HPLOC().radius_tris(self_pairs=True, radius=1.0)


def test_cpp_mirror_radius_tris_compiles(tmp_path):
    src = tmp_path / "radius_tris_mirror.cpp"
    src.write_text("""#include "bvh/builders.hpp"
template <typename B> void ask(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_build_input* q, uint32_t n, uint32_t* off,
                               bvh_tri_hit* h) {
    B bvh; bvh.build(ctx, a);
    uint64_t total = 0;
    bvh.radiusTris(ctx, q, n, 0.5f, BVH_RADIUS_TRIS_SORTED, off, nullptr, 0, &total);
    bvh.radiusTris(ctx, q, n, 0.5f, BVH_RADIUS_TRIS_SORTED, off, h, total);
    bvh.radiusTris(ctx, nullptr, (uint32_t)a.size(), 0.5f, BVH_RADIUS_TRIS_SELF | BVH_RADIUS_TRIS_SKIP_SHARED, off, h, total, &total);
}
void all(BvhConstruction::Context& ctx, std::vector<BvhConstruction::Triangle>& a, const bvh_build_input* q, uint32_t n, uint32_t* off, bvh_tri_hit* h) {
    ask<BvhConstruction::TwoPassLbvh>(ctx, a, q, n, off, h); ask<BvhConstruction::SinglePassLbvh>(ctx, a, q, n, off, h);
    ask<BvhConstruction::PLOCNew>(ctx, a, q, n, off, h); ask<BvhConstruction::HPLOC>(ctx, a, q, n, off, h);
}
static_assert(BVH_RADIUS_TRIS_SORTED == 1u && BVH_RADIUS_TRIS_SELF == 2u && BVH_RADIUS_TRIS_SKIP_SHARED == 4u, "flags");
""")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------------------------

UNIT = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]


def moved(t, dx=0.0, dy=0.0, dz=0.0):
    return [(x + dx, y + dy, z + dz) for x, y, z in t]


def tri(pkg, *ts):
    return as_triangles(pkg, np.array(ts, dtype=F32))


def plates(pkg, zs):
    return tri(pkg, *[[(-1, -1, z), (3, -1, z), (-1, 3, z)] for z in zs])


def test_parallel_plates_just_below_and_just_at_the_gap(pkg):
    tree = plates(pkg, (0.5, 0.25, 3.0, 0.5))                          # gaps 0.5, 0.25, 3, 0.5 above the query at z = 0
    q = tri(pkg, UNIT)
    pairs = pair_matrix(q, tree)
    assert list(pairs[0][0]) == [0.25, 0.0625, 9.0, 0.25]
    at = radius_tris_brute_force(pkg, q, tree, 0.5, pairs)
    assert list(at["offsets"]) == [0, 3] and list(at["hits"]["prim"]) == [1, 0, 3] and list(at["hits"]["dist2"]) == [0.0625, 0.25, 0.25]
    assert (at["hits"]["feature"] == 0).all() and (at["hits"]["reserved"] == 0).all() and at["well"].all() and at["ill_pairs"] == 0
    below = radius_tris_brute_force(pkg, q, tree, float(np.nextafter(F32(0.5), F32(0.0))), pairs)
    assert list(below["offsets"]) == [0, 1] and list(below["hits"]["prim"]) == [1]
    assert list(radius_tris_brute_force(pkg, q, tree, 0.25, pairs)["hits"]["prim"]) == [1]
    assert len(radius_tris_brute_force(pkg, q, tree, float(np.nextafter(F32(0.25), F32(0.0))), pairs)["hits"]) == 0
    everything = radius_tris_brute_force(pkg, q, tree, np.inf, pairs)
    assert list(everything["hits"]["prim"]) == [1, 0, 3, 2]            # sorted ties (prims 0 and 3 at 0.25) break by prim
    assert recompute_records(pkg, q, tree, np.inf, everything["offsets"], everything["hits"]) is None


def test_a_proper_crossing_is_reported_at_radius_zero_with_feature_15(pkg):
    floor = [(0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0)]
    blade = [(1.0, 1.0, -1.0), (1.0, 1.0, 1.0), (1.5, 1.5, 3.0)]
    tree = tri(pkg, floor, moved(floor, dz=5.0), moved(blade, dx=0.5))
    q = tri(pkg, blade, moved(blade, dz=1.5), floor)
    bf = radius_tris_brute_force(pkg, q, tree, 0.0)
    s = slices(bf)
    assert list(s[0]["prim"]) == [0] and list(s[0]["feature"]) == [CROSSING] and (s[0]["dist2"] == 0).all()     # crosses the floor
    assert len(s[1]) == 0                                              # lifted off the floor: 0.25 away
    assert list(s[2]["prim"]) == [0, 2] and list(s[2]["feature"]) == [0, CROSSING]       # its own copy touches (feature 0); the blade in the tree crosses it
    assert recompute_records(pkg, q, tree, 0.0, bf["offsets"], bf["hits"]) is None
    assert list(radius_tris_brute_force(pkg, q, tree, -0.0)["offsets"]) == list(bf["offsets"])      # radius -0 is radius 0


def test_shared_vertices_and_edges_are_distance_zero_and_skipped(pkg):
    fan = [(0.0, 0.0, 0.0), (-1.0, 0.0, 1.0), (0.0, -1.0, 1.0)]        # shares UNIT's v1
    wing = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, -1.0, 1.0)]        # shares UNIT's edge (v1, v2)
    touch = [(0.25, 0.25, 0.0), (0.25, 0.25, 2.0), (1.0, 1.0, 2.0)]    # a vertex ON UNIT's face: distance 0, no vertex in common
    far = moved(UNIT, dz=7.0)
    mesh = tri(pkg, UNIT, fan, wing, touch, far)
    pairs = pair_matrix(mesh, mesh)
    plain = radius_tris_brute_force(pkg, mesh, mesh, 0.0, pairs, self_pairs=True)
    assert [list(s["prim"]) for s in slices(plain)] == [[1, 2, 3], [2], [], [], []]          # j > i only; fan and wing share the vertex (0,0,0)
    skip = radius_tris_brute_force(pkg, mesh, mesh, 0.0, pairs, self_pairs=True, skip_shared=True)
    assert [list(s["prim"]) for s in slices(skip)] == [[3], [], [], [], []]
    assert recompute_records(pkg, mesh, mesh, 0.0, skip["offsets"], skip["hits"], True, True) is None
    assert recompute_records(pkg, mesh, mesh, 0.0, plain["offsets"], plain["hits"], True, False) is None
    assert recompute_records(pkg, mesh, mesh, 0.0, plain["offsets"], plain["hits"], True, True) == "a pair that shares a vertex is reported"
    wide = radius_tris_brute_force(pkg, mesh, mesh, 10.0, pairs, self_pairs=True, skip_shared=True)
    assert [list(s["prim"]) for s in slices(wide)] == [[3, 4], [3, 4], [3, 4], [4], []]      # the neighbours stay out at every radius


def test_negative_zero_is_shared_and_a_nan_vertex_is_neither_shared_nor_accepted(pkg):
    a = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]
    b = [(-0.0, 0.0, -0.0), (-1.0, 0.0, 1.0), (0.0, -1.0, 1.0)]        # its v1 is a's v1 with other zero signs
    c = [(NAN, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]            # a with a NaN in v1: v2 and v3 equal a's
    d = [(NAN, 0.0, 0.0), (5.0, 5.0, 5.0), (6.0, 5.0, 5.0)]            # its NaN vertex is bit-equal to c's
    assert list(shared_vertex(np.array([a, a, c, a], dtype=F32), np.array([b, c, d, d], dtype=F32))) == [True, True, False, False]
    mesh = tri(pkg, a, b, c, d)
    bf = radius_tris_brute_force(pkg, mesh, mesh, np.inf, self_pairs=True, skip_shared=True)
    assert list(bf["counts"]) == [0, 0, 0, 0]                          # (a, b) shared; c and d are never accepted (NaN dist2) and dead as queries
    plain = radius_tris_brute_force(pkg, mesh, mesh, np.inf, self_pairs=True)
    assert [list(s["prim"]) for s in slices(plain)] == [[1], [], [], []]


def test_dead_queries_and_radii(pkg):
    tree = plates(pkg, (0.5, 1.0))
    q = tri(pkg, UNIT, [(NAN, 0, 0), (1, 0, 0), (0, 1, 0)], moved(UNIT, dz=0.75))
    pairs = pair_matrix(q, tree)
    for radius in (-1.0, -np.inf, np.nan):
        bf = radius_tris_brute_force(pkg, q, tree, radius, pairs)
        assert list(bf["offsets"]) == [0, 0, 0, 0] and len(bf["hits"]) == 0 and bf["well"].all()
    bf = radius_tris_brute_force(pkg, q, tree, np.inf, pairs)
    assert list(bf["offsets"]) == [0, 2, 2, 4]                         # the NaN query is dead at every radius


def test_first_sorted_record_is_the_closest_answer(pkg):
    rng = np.random.default_rng(5)
    tree = as_triangles(pkg, rng.random((40, 1, 3)) + rng.normal(0, 0.08, (40, 3, 3)))
    q = as_triangles(pkg, rng.random((30, 1, 3)) + rng.normal(0, 0.08, (30, 3, 3)))
    pairs = pair_matrix(q, tree)
    for radius in (0.0, 0.1, 0.3, np.inf):
        bf = radius_tris_brute_force(pkg, q, tree, radius, pairs)
        closest = tris_brute_force(pkg, q, tree, radius, pairs)
        assert ((bf["counts"] > 0) == closest["hit"]).all() and (bf["counts"] == closest["n_acc"]).all()
        first = bf["hits"][bf["offsets"][:-1][closest["hit"]]]
        assert first.tobytes() == closest["closest"][closest["hit"]].tobytes()
        assert recompute_records(pkg, q, tree, radius, bf["offsets"], bf["hits"]) is None
    # what recompute_records must catch
    bf = radius_tris_brute_force(pkg, q, tree, 0.3, pairs)
    assert len(bf["hits"]) > 4
    for field, value, msg in (("reserved", 1, "reserved"), ("feature", 14, "feature"), ("dist2", F32(1e-9), "bit-equal")):
        bad = bf["hits"].copy(); bad[field][0] = value
        assert msg in recompute_records(pkg, q, tree, 0.3, bf["offsets"], bad)
    i = int(np.argmax(bf["counts"] > 1)); o = int(bf["offsets"][i])
    bad = bf["hits"].copy(); bad[o + 1] = bad[o]
    assert recompute_records(pkg, q, tree, 0.3, bf["offsets"], bad) == "a prim twice in one slice"
    inf = radius_tris_brute_force(pkg, q, tree, np.inf, pairs)
    assert "not accepted" in recompute_records(pkg, q, tree, 0.3, inf["offsets"], inf["hits"])
