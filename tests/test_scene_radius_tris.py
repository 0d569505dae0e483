"""CPU: bvh_scene_radius_tris in the C ABI, the library and the Python binding; the numpy restatement of its contract — the two-level brute force cut from
test_scene_closest_tris.scene_pair_matrix (tri_tri_formula over the world triangles of every active instance, acceptance dist2 <= r2, slices in ascending
(dist2, instance, prim) order, the well-conditioned flag by the header's two conditions applied to EVERY accepted pair) and the checker of single records —
with hand cases whose answers are exact, the brute force against test_radius_tris.radius_tris_brute_force on the flattened scene and its first records against
test_scene_closest_tris.scene_tris_dist_brute_force.  The GPU tests (tests/test_gpu_scene_radius_tris.py) compare against this file."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_abi import _code_object
from test_closest_tris import CROSSING, E_INVALID, query_ok, radius2, tri_tri_formula
from test_deep_trees import QUERY_STACK
from test_intersect_tris import as_triangles, xyz
from test_radius_tris import radius_tris_brute_force
from test_scene import identity, make_instances, mat34, tris_root_box
from test_scene_closest_tris import (PLATE, SCENE_TRIS_INSTANCE, SCENE_TRIS_QUERY, SMALL, mixed_queries, scene_pair_matrix, scene_tris_dist_brute_force, tri_mesh,
                                     well_conditioned)
from test_scene_intersect_tris import instance_queries, world_tris
from test_scene_point import active_instances, flat_world_tris, instance_set

F32 = np.float32
NAN = float("nan")
SCENE_RADIUS_TRIS_SORTED = 1


# ---- the contract, restated ---------------------------------------------------------------------------------------------------------------------------------

def scene_radius_tris_brute_force(pkg, queries, blas_tris, inst, radius, skip=None, pairs=None, root_boxes=None):
    """every query triangle against every world triangle of every active instance (but instance ``skip``).  Returns dict: offsets (u32[m + 1]), hits
    (INSTANCE_TRI_HIT[total], each slice in ascending (dist2, instance, prim) order), counts, well (bool[m]: EVERY accepted pair of the query meets the
    header's two conditions against its own dist2; an empty slice is well-conditioned), ill_pairs (how many accepted pairs fail them).  pairs:
    scene_pair_matrix(...), when the caller keeps it across radii and skips"""
    (d2, feat), ks, js = pairs if pairs is not None else scene_pair_matrix(pkg, queries, blas_tris, inst)
    if root_boxes is None:
        root_boxes = [tris_root_box(t) for t in blas_tris]
    x = xyz(queries)
    m = len(x)
    with np.errstate(invalid="ignore"):
        acc = (d2 <= radius2(radius)) & query_ok(queries, radius)[:, None]
    if skip is not None:
        acc &= (ks != skip)[None, :]
    rows, cols = np.nonzero(acc)
    d = d2[rows, cols]
    assert not np.isnan(d).any() and not np.signbit(d).any()          # an accepted dist2 is never NaN or negative (so the u64 key order is this order)
    order = np.lexsort((cols, d, rows))                               # (the columns are in (instance, prim) order)
    rows, cols, d = rows[order], cols[order], d[order]
    hits = np.zeros(len(rows), dtype=pkg.INSTANCE_TRI_HIT)
    hits["dist2"], hits["prim"], hits["feature"], hits["instance"] = d, js[cols], feat[rows, cols], ks[cols]
    counts = acc.sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    well = np.ones(m, dtype=bool)
    ill = 0
    for k in np.unique(ks[cols]):
        idx = np.nonzero(ks[cols] == k)[0]
        ok = well_conditioned(pkg, x[rows[idx]], int(k), js[cols[idx]], d[idx], blas_tris, inst, root_boxes)
        ill += int((~ok).sum())
        well[np.unique(rows[idx][~ok])] = False
    return {"offsets": offsets, "hits": hits, "counts": counts, "well": well, "ill_pairs": ill}


def scene_radius_tris_recompute(pkg, queries, blas_tris, inst, radius, offsets, hits, skip=None):
    """None if (offsets, hits) is a well-formed answer — the offsets a scan that ends at the number of records, no (instance, prim) twice in a slice, every
    record an accepted candidate of an active instance other than ``skip`` with bit-equal dist2 and the same feature — otherwise a sentence saying what is
    wrong"""
    x = xyz(queries)
    off = offsets.astype(np.int64)
    if len(off) != len(x) + 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != len(hits):
        return "the offsets are not a scan that ends at the number of records"
    rows = np.repeat(np.arange(len(x)), np.diff(off))
    _, active = active_instances(inst, len(blas_tris))
    ki, pr = hits["instance"].astype(np.int64), hits["prim"].astype(np.int64)
    if (ki >= len(inst)).any() or not active[ki].all():
        return "a record of an inactive instance (or of none)"
    if skip is not None and (ki == skip).any():
        return "a record of the skipped instance"
    sizes = np.array([len(t) for t in blas_tris], dtype=np.int64)[inst["blas"][ki].astype(np.int64)] if len(ki) else np.zeros(0, dtype=np.int64)
    if (pr >= sizes).any():
        return "a prim out of range"
    if len(np.unique(np.stack([rows, ki, pr], axis=1), axis=0)) != len(pr):
        return "an (instance, prim) twice in one slice"
    for k in np.unique(ki):
        idx = np.nonzero(ki == k)[0]
        w = world_tris(inst["object_to_world"][k], blas_tris[int(inst["blas"][k])][pr[idx]])
        d, f = tri_tri_formula(x[rows[idx]], w)
        with np.errstate(invalid="ignore"):
            acc = (d <= radius2(radius)) & query_ok(x, radius)[rows[idx]]
        if not acc.all():
            return f"{np.count_nonzero(~acc)} records are not accepted candidates"
        if (d.view(np.uint32) != hits["dist2"][idx].view(np.uint32)).any():
            return "a dist2 is not bit-equal to its candidate's"
        if (f != hits["feature"][idx]).any():
            return "a feature differs from its candidate's"
    return None


def scene_radius_host_sort(offsets, hits):
    """every slice put into ascending (dist2, instance, prim) order on the host"""
    rows = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets.astype(np.int64)))
    return hits[np.lexsort((hits["prim"], hits["instance"], hits["dist2"], rows))]


def slices(off, hits):
    o = off.astype(np.int64)
    return [hits[o[i]:o[i + 1]] for i in range(len(o) - 1)]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_flag_and_the_entry_point(pkg):
    full = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    ptr = r"\s*\*\s*\w+\s*,\s*"
    assert re.search(r"\bint\s+bvh_scene_radius_tris\s*\(\s*bvh_scene" + ptr + "const bvh_build_input" + ptr + r"uint32_t\s+\w+\s*,\s*int\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*"
                     r"float\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t" + ptr + "bvh_instance_tri_hit" + ptr + r"uint64_t\s+\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"#define BVH_SCENE_RADIUS_TRIS_SORTED\s+1u\b", text) and pkg.SCENE_RADIUS_TRIS_SORTED == SCENE_RADIUS_TRIS_SORTED
    assert "#define BVH_ABI_VERSION 4" in text
    # the contract is in the header
    assert "Every triangle within a radius, on scenes: bvh_scene_radius_tris" in full and "s2_k * lb' * (1 - 2^-20) > r2" in full
    types = open(os.path.join(ROOT, "include", "bvh", "types.h")).read()
    assert "bvh_scene_radius_tris" in types


def test_library_exports_the_symbol(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_scene_radius_tris") and "bvh_scene_radius_tris" in pkg.EXPORTS
    f = pkg.lib().bvh_scene_radius_tris
    assert len(f.argtypes) == 11 and f.argtypes[5] is C.c_float and f.argtypes[6] is C.c_uint32 and f.argtypes[9] is C.c_uint64 and f.restype is C.c_int
    assert pkg.lib().bvh_abi_version() == 4 and pkg.ABI_VERSION == 4
    assert pkg.INSTANCE_TRI_HIT.itemsize == 16 and pkg.INSTANCE_TRI_HIT.names == ("dist2", "prim", "feature", "instance")


def test_cpp_translation_unit_compiles(tmp_path):
    src = tmp_path / "scene_radius_tris_caller.cpp"
    src.write_text("""#include "bvh_mi355x.h"
int ask(bvh_scene* scene, const bvh_build_input* q, uint32_t n, uint32_t* off, bvh_instance_tri_hit* h) {
    uint64_t total = 0;
    int r = bvh_scene_radius_tris(scene, q, n, BVH_SCENE_TRIS_QUERY, 0u, 0.5f, BVH_SCENE_RADIUS_TRIS_SORTED, off, nullptr, 0, &total);
    r |= bvh_scene_radius_tris(scene, q, n, BVH_SCENE_TRIS_QUERY, 0u, 0.5f, BVH_SCENE_RADIUS_TRIS_SORTED, off, h, total, nullptr);
    r |= bvh_scene_radius_tris(scene, nullptr, n, BVH_SCENE_TRIS_INSTANCE, 3u, 0.5f, 0u, off, h, total, &total);
    return r;
}
static_assert(BVH_SCENE_RADIUS_TRIS_SORTED == 1u, "flag");
static_assert(sizeof(bvh_instance_tri_hit) == 16, "size");
""")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_binding_and_errors_without_a_device(pkg):
    assert callable(getattr(pkg.Scene, "radius_tris"))
    L = pkg.lib()
    q = pkg.BuildInput(pkg.TRI_PADDED64, 30, 1 << 21, None, None, 0, 0)
    total = C.c_uint64(77)
    assert L.bvh_scene_radius_tris(None, None, 0, 0, 0, 1.0, 0, None, None, 0, None) == E_INVALID
    assert L.bvh_scene_radius_tris(None, C.byref(q), 4, SCENE_TRIS_QUERY, 0, 1.0, 1, 4096, 8192, 16, C.byref(total)) == E_INVALID      # NULL scene
    assert L.bvh_scene_radius_tris(None, None, 4, SCENE_TRIS_INSTANCE, 0, 1.0, 0, 4096, 8192, 16, C.byref(total)) == E_INVALID
    assert L.bvh_scene_radius_tris(None, C.byref(q), 0, SCENE_TRIS_QUERY, 0, 1.0, 1, 4096, 8192, 16, C.byref(total)) == E_INVALID      # NULL scene comes before n_queries == 0
    assert L.bvh_scene_radius_tris(None, None, 0, SCENE_TRIS_INSTANCE, 0, 1.0, 1, 4096, None, 0, C.byref(total)) == E_INVALID
    assert total.value == 77                                            # an error writes nothing


def test_kernels_use_no_scratch_and_the_walks_16_kib_of_lds(pkg, tmp_path):
    obj = os.path.join(ROOT, "hip-bvh-construction_amd", "csrc", "scene_radius_tris.o")
    assert os.path.exists(obj), "scene_radius_tris.o is missing: the build makes it (a missing object is a failure, not a reason to skip)"
    got = _code_object(obj, str(tmp_path))
    if got is None:
        pytest.skip("the LLVM tools that unbundle a code object are missing")
    _, notes = got
    seen = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "k_scene_radius_tris" in name:
            seen[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)),
                          int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)), int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)))
    walks = [k for k in seen if "k_scene_radius_tris_walk" in k]
    deeps = [k for k in seen if "k_scene_radius_tris_deep" in k]
    assert len(walks) == 6 and len(deeps) == 6 and len(seen) == 12, sorted(seen)      # count, fill and sorted fill in either mode; a deep kernel for each
    for name, (scratch, lds, vgprs) in seen.items():
        assert scratch == 0, (name, "spills to scratch", scratch)
        assert lds == (QUERY_STACK * 64 * 4 if name in walks else 0), (name, lds)
        assert vgprs <= 256, (name, vgprs)                              # two waves per SIMD (VGPRs and AGPR copies together)


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------------------------------

def below(r):
    return float(np.nextafter(F32(r), F32(0.0)))


def test_parallel_plates_just_below_and_just_at_the_gap(pkg):
    mesh = tri_mesh(pkg, PLATE)
    q = tri_mesh(pkg, SMALL)
    mats = [mat34(np.eye(3), (0.0, 0.0, 3.0)),                          # the plate at world z = 4: dist2 16
            mat34(2.0 * np.eye(3)),                                     # ... at z = 2, twice the size: dist2 4
            mat34(np.diag([1.0, 1.0, -1.0]), (0.0, 0.0, -0.5))]         # ... mirrored to z = -1.5: dist2 2.25
    for k, gap in enumerate((4.0, 2.0, 1.5)):
        inst = make_instances(pkg, [mats[k]], [0])
        pairs = scene_pair_matrix(pkg, q, [mesh], inst)
        at = scene_radius_tris_brute_force(pkg, q, [mesh], inst, gap, pairs=pairs)
        assert list(at["offsets"]) == [0, 1] and at["ill_pairs"] == 0 and at["well"].all()
        h = at["hits"][0]
        assert (h["dist2"], h["prim"], h["feature"], h["instance"]) == (F32(gap * gap), 0, 0, 0)      # the three vertex terms tie: index 0
        assert list(scene_radius_tris_brute_force(pkg, q, [mesh], inst, below(gap), pairs=pairs)["offsets"]) == [0, 0]
    inst = make_instances(pkg, mats, [0, 0, 0])
    pairs = scene_pair_matrix(pkg, q, [mesh], inst)
    everything = scene_radius_tris_brute_force(pkg, q, [mesh], inst, np.inf, pairs=pairs)
    assert list(everything["hits"]["instance"]) == [2, 1, 0] and list(everything["hits"]["dist2"]) == [2.25, 4.0, 16.0] and everything["ill_pairs"] == 0
    assert scene_radius_tris_recompute(pkg, q, [mesh], inst, np.inf, everything["offsets"], everything["hits"]) is None
    assert list(scene_radius_tris_brute_force(pkg, q, [mesh], inst, 2.0, pairs=pairs)["hits"]["instance"]) == [2, 1]      # dist2 4 is accepted (<=)
    assert list(scene_radius_tris_brute_force(pkg, q, [mesh], inst, below(2.0), pairs=pairs)["hits"]["instance"]) == [2]
    assert len(scene_radius_tris_brute_force(pkg, q, [mesh], inst, 1.25, pairs=pairs)["hits"]) == 0
    # what the checker must catch
    off, hits = everything["offsets"], everything["hits"]
    for field, value, msg in (("feature", 1, "feature"), ("dist2", F32(2.0), "bit-equal"), ("instance", 7, "inactive"), ("prim", 1, "out of range")):
        bad = hits.copy(); bad[field][0] = value
        assert msg in scene_radius_tris_recompute(pkg, q, [mesh], inst, np.inf, off, bad)
    bad = hits.copy(); bad[1] = bad[0]
    assert scene_radius_tris_recompute(pkg, q, [mesh], inst, np.inf, off, bad) == "an (instance, prim) twice in one slice"
    assert "not accepted" in scene_radius_tris_recompute(pkg, q, [mesh], inst, 2.0, off, hits)
    assert "scan" in scene_radius_tris_recompute(pkg, q, [mesh], inst, np.inf, off, hits[:2])
    assert "skipped" in scene_radius_tris_recompute(pkg, q, [mesh], inst, np.inf, off, hits, skip=1)


def test_a_crossing_across_two_instances_and_coincident_instances(pkg):
    floor = tri_mesh(pkg, [(0, 0, 0), (4, 0, 0), (0, 4, 0)])
    blade = [(1.0, 1.0, -1.0), (1.0, 1.0, 1.0), (1.5, 1.5, 3.0)]      # its edge (v1, v2) passes through z = 0 and z = 0.5 at (1, 1)
    q = tri_mesh(pkg, blade, [(x, y, z + 1.75) for x, y, z in blade])
    inst = make_instances(pkg, [mat34(np.eye(3), (0.0, 0.0, 0.5)), identity(), identity()], [0, 0, 0])
    pairs = scene_pair_matrix(pkg, q, [floor], inst)
    zero = scene_radius_tris_brute_force(pkg, q, [floor], inst, 0.0, pairs=pairs)
    # the blade crosses all three floors: dist2 0 and feature 15, in instance order (the two coincident floors both answer); lifted, it hangs 0.25 over the
    # lifted floor and crosses none
    assert list(zero["offsets"]) == [0, 3, 3] and zero["ill_pairs"] == 0
    assert list(zero["hits"]["instance"]) == [0, 1, 2] and (zero["hits"]["feature"] == CROSSING).all() and (zero["hits"]["dist2"] == 0).all()
    assert list(scene_radius_tris_brute_force(pkg, q, [floor], inst, -0.0, pairs=pairs)["offsets"]) == [0, 3, 3]      # radius -0 is radius 0
    near = scene_radius_tris_brute_force(pkg, q, [floor], inst, 0.25, pairs=pairs)
    s = slices(near["offsets"], near["hits"])
    assert list(s[1]["instance"]) == [0] and s[1]["dist2"][0] == F32(0.0625) and s[1]["feature"][0] == 0
    wide = scene_radius_tris_brute_force(pkg, q, [floor], inst, 0.75, pairs=pairs)
    s = slices(wide["offsets"], wide["hits"])
    assert list(s[1]["instance"]) == [0, 1, 2] and list(s[1]["dist2"]) == [0.0625, 0.5625, 0.5625]      # the coincident pair ties: instance order
    assert scene_radius_tris_recompute(pkg, q, [floor], inst, 0.75, wide["offsets"], wide["hits"]) is None


def test_an_inactive_instance_is_silent(pkg):
    mesh = tri_mesh(pkg, PLATE)
    q = tri_mesh(pkg, SMALL)
    inst = make_instances(pkg, [mat34(np.zeros((3, 3))), identity(), identity()], [0, 0, 7])     # singular; active; a BLAS index out of range
    bf = scene_radius_tris_brute_force(pkg, q, [mesh], inst, np.inf)
    assert list(bf["offsets"]) == [0, 1] and bf["hits"]["instance"][0] == 1 and bf["hits"]["dist2"][0] == F32(1.0)
    for k in (0, 2):
        bad = bf["hits"].copy(); bad["instance"][0] = k
        assert "inactive" in scene_radius_tris_recompute(pkg, q, [mesh], inst, np.inf, bf["offsets"], bad)


def test_instance_mode_skips_its_own_instance_but_not_a_twin(pkg):
    mesh = tri_mesh(pkg, PLATE, [(5, 5, 5), (6, 5, 5), (5, 6, 5)])
    inst = make_instances(pkg, [identity(), identity(), mat34(np.eye(3), (0.0, 0.0, 1.0)), mat34(np.zeros((3, 3)))], [0, 0, 0, 0])
    rows = instance_queries([mesh], inst, 0, 4)                         # four rows over a BLAS of two: the last two are NaN triangles
    bf = scene_radius_tris_brute_force(pkg, rows, [mesh], inst, 1.0, skip=0)
    s = slices(bf["offsets"], bf["hits"])
    assert list(bf["counts"]) == [2, 2, 0, 0]                           # the twin at 0, the lifted copy one unit above; rows beyond the BLAS are empty
    assert list(s[0]["instance"]) == [1, 2] and list(s[0]["prim"]) == [0, 0] and list(s[0]["dist2"]) == [0.0, 1.0]
    assert list(s[1]["instance"]) == [1, 2] and list(s[1]["prim"]) == [1, 1]
    assert scene_radius_tris_recompute(pkg, rows, [mesh], inst, 1.0, bf["offsets"], bf["hits"], skip=0) is None
    assert list(scene_radius_tris_brute_force(pkg, rows, [mesh], inst, 0.0, skip=0)["counts"]) == [1, 1, 0, 0]
    # the rows of an inactive query instance are all empty
    none = scene_radius_tris_brute_force(pkg, instance_queries([mesh], inst, 3, 2), [mesh], inst, np.inf, skip=3)
    assert list(none["offsets"]) == [0, 0, 0] and none["well"].all()


def test_dead_queries_and_radii(pkg):
    mesh = tri_mesh(pkg, PLATE)
    q = tri_mesh(pkg, SMALL, [(NAN, 0, 0), (1, 0, 0), (0, 1, 0)], [(x, y, z + 0.5) for x, y, z in SMALL])
    inst = make_instances(pkg, [identity(), mat34(np.eye(3), (0.0, 0.0, 1.0))], [0, 0])
    pairs = scene_pair_matrix(pkg, q, [mesh], inst)
    for radius in (-1.0, -np.inf, np.nan):
        bf = scene_radius_tris_brute_force(pkg, q, [mesh], inst, radius, pairs=pairs)
        assert list(bf["offsets"]) == [0, 0, 0, 0] and len(bf["hits"]) == 0 and bf["well"].all() and bf["ill_pairs"] == 0
    bf = scene_radius_tris_brute_force(pkg, q, [mesh], inst, np.inf, pairs=pairs)
    assert list(bf["offsets"]) == [0, 2, 2, 4]                         # the NaN query is dead at every radius


# ---- equivalences ---------------------------------------------------------------------------------------------------------------------------------------------

def test_two_level_brute_force_equals_flattened_and_its_first_record_is_the_closest(pkg):
    rng = np.random.default_rng(4)
    meshes = [pkg.meshgen.uniform(40, 1), pkg.meshgen.uniform(25, 2)]
    inst = instance_set(pkg, rng, "shear", 6, n_blas=2)
    inst = np.concatenate([inst, inst[:2]])                             # two coincident pairs: every answer on them ties on dist2
    inst["object_to_world"][3][5] = np.nan                            # and an inactive one
    flat, ks, js = flat_world_tris(pkg, meshes, inst)
    q = mixed_queries(pkg, flat, 300, 5)
    pairs = scene_pair_matrix(pkg, q, meshes, inst)
    assert np.array_equal(pairs[1], ks) and np.array_equal(pairs[2], js)
    totals = []
    for radius in (np.inf, 0.05, 0.0):
        got = scene_radius_tris_brute_force(pkg, q, meshes, inst, radius, pairs=pairs)
        ref = radius_tris_brute_force(pkg, q, flat, radius, pairs[0])
        g, r = got["hits"], ref["hits"]
        assert np.array_equal(got["offsets"], ref["offsets"]) and np.array_equal(got["counts"], ref["counts"])
        assert np.array_equal(g["dist2"].view(np.uint32), r["dist2"].view(np.uint32)) and np.array_equal(g["feature"], r["feature"])
        assert np.array_equal(g["instance"], ks[r["prim"]]) and np.array_equal(g["prim"], js[r["prim"]])
        assert 3 not in g["instance"]                                   # the inactive one
        assert scene_radius_tris_recompute(pkg, q, meshes, inst, radius, got["offsets"], g) is None
        backwards = np.concatenate([s[::-1] for s in slices(got["offsets"], g)])
        assert scene_radius_host_sort(got["offsets"], backwards).tobytes() == g.tobytes()      # the host sort puts any order of a slice back
        closest = scene_tris_dist_brute_force(pkg, q, meshes, inst, radius, pairs=pairs)
        assert np.array_equal(got["counts"] > 0, closest["hit"]) and np.array_equal(got["counts"], closest["n_acc"])
        assert g[got["offsets"][:-1][closest["hit"]]].tobytes() == closest["closest"][closest["hit"]].tobytes()
        totals.append(len(g))
    assert totals[0] == (len(q) - 2) * len(flat) and totals[0] > totals[1] > totals[2] > 0
    zero = scene_radius_tris_brute_force(pkg, q, meshes, inst, 0.0, pairs=pairs)["hits"]
    assert (zero["feature"] == CROSSING).any() and (zero["dist2"] == 0).all()
    # instance mode: the rows of instance 1 against everybody else, the coincident copy (instance 7) included
    rows = as_triangles(pkg, instance_queries(meshes, inst, 1, 30))
    ipairs = scene_pair_matrix(pkg, rows, meshes, inst)
    igot = scene_radius_tris_brute_force(pkg, rows, meshes, inst, 0.0, skip=1, pairs=ipairs)
    assert 1 not in igot["hits"]["instance"] and (igot["counts"][:25] >= 1).all() and not igot["counts"][25:].any()
    for i, s in enumerate(slices(igot["offsets"], igot["hits"])[:25]):  # row i coincides with triangle i of the copy
        assert ((s["instance"] == 7) & (s["prim"] == i)).sum() == 1
    assert scene_radius_tris_recompute(pkg, rows, meshes, inst, 0.0, igot["offsets"], igot["hits"], skip=1) is None
