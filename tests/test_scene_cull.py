"""CPU: bvh_scene_cull in the C ABI, the library and the Python binding; the numpy restatement of the contract's object planes
(pkg.scene_cull_object_planes) — on the identity, and against an f64 evaluation of the world plane at the mapped corners —; the two-level brute force
(pkg.scene_cull_brute_force, the single reference of these tests and of tests/test_gpu_scene_cull.py) on a hand scene with exact records; the checker the GPU
tests use on every answer, pinned by tampered slices; the host restatements of the two-level lane walk and of the group walk's schedule on the CPU oracle's
trees of all four builders, which must return exactly the brute force's sets; the GPU tests' inputs, made here so that their premises (empty slices, long
slices, a volume that touches every instance) are checked without a device; and the kernels' scratch and LDS, read from the object file."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_abi import _code_object
from test_cull import GROUP_BLOCK, PADDING, Tree, box_planes, fat_caterpillar, look_at, perspective
from test_deep_trees import QUERY_STACK, STAIRS, stairs_steps
from test_gpu_query import caterpillar
from test_gpu_refit import no_negzero
from test_gpu_scene import scene_instances
from test_gpu_scene_point import with_shear
from test_overlap import E_INVALID, as_boxes, leaf_boxes_of
from test_scene import identity, make_instances, mat34, rot, world_box
from test_scene_extremes import FAR, RUNGS, SHEAR, UNI, meshes as ladder_meshes, rung_instances
from test_scene_knn import DEEP_OFFSETS, cached, coincident_inputs, inactive_of, moved_inputs
from test_scene_overlap import slice_queries, tri_leaf_boxes, world_leaf_boxes
from test_scene_point import active_instances, shear_matrix

F32, F64 = np.float32, np.float64
N_VOLUMES = 256
PLANE_COUNTS = (1, 4, 6, 8)
SCENE_N_INST = [1, 2, 7, 64]
MESH_SIZES = [2000, 300, 700, 2]        # BLAS b is built by builder b; instance k places BLAS k % 4
MESH_SIZES_64 = [600, 300, 120, 2]      # ... of the 64-instance scene: a half-space holds half of all its leaves, 256 volumes a quarter of the records


def mesh_sizes(n_inst):
    return MESH_SIZES_64 if n_inst == 64 else MESH_SIZES


class CSceneCullHit(C.Structure):
    _fields_ = [("prim", C.c_uint32), ("instance", C.c_uint32), ("straddle", C.c_uint32), ("zero", C.c_uint32)]


# ---- the reference --------------------------------------------------------------------------------------------------------------------------------------------------

def stored_world_boxes(blas_leaf, inst):
    """(marked instances, world boxes): what the scene stores — an inactive instance (tests/test_scene.py's rules) has blas == INVALID and an inverted box,
    an active one the fminf / fmaxf box of the 8 mapped corners of its BLAS's root box (the bitwise union of the leaf boxes)"""
    _, active = active_instances(inst, len(blas_leaf))
    marked = inst.copy(); marked["blas"][~active] = 0xFFFFFFFF
    wb = np.zeros((len(inst), 6), dtype=F32); wb[:, :3] = 1.0
    for k in np.nonzero(active)[0]:
        leaf = as_boxes(blas_leaf[int(inst["blas"][k])])
        wb[k] = world_box(inst["object_to_world"][k], np.concatenate([leaf["min"].min(axis=0), leaf["max"].max(axis=0)]))
    return marked, wb


def reference(pkg, planes, blas_leaf, inst):
    """the brute force on the scene as bvh_scene_build stores it -> dict offsets, recs (ascending (instance, prim) per slice), counts"""
    marked, wb = stored_world_boxes(blas_leaf, inst)
    off, rec = pkg.scene_cull_brute_force(planes, blas_leaf, marked, wb)
    return {"offsets": off, "recs": rec, "counts": np.diff(off.astype(np.int64))}


def scene_cull_host_sort(offsets, recs):
    """every slice in ascending (instance, prim) order: the canonical form of an answer (the order inside a slice is unspecified)"""
    return recs[np.lexsort((recs["prim"], recs["instance"], slice_queries(offsets)))]


def check_scene_cull(pkg, off, recs, ref, what=""):
    """the GPU tests' checker, on EVERY volume: the offsets are a scan from 0 up to len(recs) and equal the brute force's; no (instance, prim) pair appears
    twice in a slice; every zero word is 0; the host-sorted records are the brute force's bytes (pairs and straddle masks; an inactive instance never occurs)"""
    o = off.astype(np.int64)
    m = len(ref["offsets"]) - 1
    assert recs.dtype == pkg.SCENE_CULL_HIT, f"{what}: records of dtype {recs.dtype}"
    assert len(o) == m + 1 and o[0] == 0 and (np.diff(o) >= 0).all() and o[-1] == len(recs), f"{what}: offsets are not a scan of the slices"
    bad = np.nonzero(o != ref["offsets"].astype(np.int64))[0]
    assert bad.size == 0, f"{what}: {bad.size} offsets differ from the brute force's, first at {bad[0]}: {o[bad[0]]} for {ref['offsets'][bad[0]]}"
    assert (recs["zero"] == 0).all(), f"{what}: a record's zero word is not 0"
    q = slice_queries(off)
    srt = recs[np.lexsort((recs["prim"], recs["instance"], q))]
    twice = (srt["prim"][1:] == srt["prim"][:-1]) & (srt["instance"][1:] == srt["instance"][:-1]) & (q[1:] == q[:-1])       # (q is ascending: sorting keeps it)
    assert not twice.any(), f"{what}: an (instance, prim) pair appears twice in a slice"
    assert srt.tobytes() == ref["recs"].tobytes(), f"{what}: the host-sorted slices differ from the brute force"


def has_nan(pkg, planes, blas_leaf, inst):
    """does the brute force meet a NaN in any s (world planes on the stored world boxes) or s' (object planes on the leaf boxes) of an active instance"""
    pl = np.asarray(planes, dtype=F32)
    marked, wb = stored_world_boxes(blas_leaf, inst)
    for k in np.nonzero(marked["blas"] != 0xFFFFFFFF)[0]:
        s = pkg.cull_plane_values(pl, wb[k, :3], wb[k, 3:])
        leaf = as_boxes(blas_leaf[int(inst["blas"][k])])
        obj = pkg.scene_cull_object_planes(pl, inst["object_to_world"][k])
        t = pkg.cull_plane_values(obj[:, :, None, :], leaf["min"][None, None], leaf["max"][None, None])
        if any(np.isnan(a).any() for a in (*s, *t)):
            return True
    return False


# ---- 1. the object planes -------------------------------------------------------------------------------------------------------------------------------------------

def test_object_planes_on_the_identity_are_the_planes(pkg):
    rng = np.random.default_rng(1)
    pl = (rng.normal(size=(4000, 4)) * 10.0 ** rng.uniform(-6, 6, (4000, 1))).astype(F32)
    pl[rng.random((4000, 4)) < 0.1] = 0.0
    pl[rng.random((4000, 4)) < 0.05] = -0.0
    pl[:2] = [PADDING, (-0.0, 0.0, -0.0, -1.0)]
    got = pkg.scene_cull_object_planes(pl, identity())
    assert got.dtype == F32 and got.shape == pl.shape and np.array_equal(got, pl)          # as values: ((a 1 + b 0) + c 0) == a
    assert got[0].tolist() == list(PADDING)
    assert (np.signbit(pl[:, :3]) & (pl[:, :3] == 0)).any()
    # a zero's sign does not change n.k >= 0: the same p-vertices, so the same test and the same masks on any box
    lo = rng.uniform(-5, 0, (4000, 3)).astype(F32); hi = (lo + rng.uniform(0, 5, (4000, 3))).astype(F32)
    a, b = pkg.cull_plane_values(pl, lo, hi), pkg.cull_plane_values(got, lo, hi)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # one volume form and the broadcast form agree; each product and each sum is rounded on its own
    m = mat34(np.diag([2.0, 3.0, 5.0]), (1.0, 2.0 ** -24, 2.0 ** -24))
    assert pkg.scene_cull_object_planes(np.array([1.0, 1.0, 1.0, -1.0], dtype=F32), m).tolist() == [2.0, 3.0, 5.0, 0.0]      # ((1 + 2^-24) + 2^-24) - 1 step by step
    many = pkg.scene_cull_object_planes(pl[:, None, :], np.stack([identity(), m])[None])
    assert many.shape == (4000, 2, 4) and np.array_equal(many[:, 0], pl)


def test_object_planes_against_f64_at_the_mapped_corners(pkg):
    """the f32 test of an object box against the object planes agrees with an f64 evaluation of the WORLD plane at the box's eight mapped corners whenever
    that value is outside a band of 2^-20 of the sum of the absolute terms — under rotations, shears, non-uniform scales and a reflection"""
    rng = np.random.default_rng(2)
    count = 60_000
    mats = np.zeros((count, 12), dtype=F32)
    kinds = 8
    base = []
    for j in range(kinds):
        A = shear_matrix(rng) if j % 2 else rot(rng.integers(3), rng.uniform(0, 6.28)) @ np.diag(rng.uniform(0.25, 4.0, 3)) @ rot(rng.integers(3), rng.uniform(0, 6.28))
        if j == 3:
            A = A @ np.diag([-1.0, 1.0, 1.0])                            # a reflection
        base.append(mat34(A, rng.uniform(-3.0, 3.0, 3)))
    assert np.linalg.det(np.asarray(base[3], dtype=F64).reshape(3, 4)[:, :3]) < 0
    mats[:] = np.asarray(base, dtype=F32)[rng.integers(0, kinds, count)]
    c = rng.uniform(-2.0, 2.0, (count, 3)); h = rng.uniform(0.0, 0.5, (count, 3))
    lo, hi = (c - h).astype(F32), (c + h).astype(F32)
    nrm = rng.normal(size=(count, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pl = np.concatenate([nrm, rng.uniform(-8.0, 8.0, (count, 1))], axis=1).astype(F32)
    obj = pkg.scene_cull_object_planes(pl, mats)
    s_p, _ = pkg.cull_plane_values(obj, lo, hi)
    M = mats.astype(F64).reshape(count, 3, 4); P = pl.astype(F64)
    best, terms = np.full(count, -np.inf), np.zeros(count)
    for corner in range(8):
        x = np.stack([(hi if corner >> ax & 1 else lo)[:, ax] for ax in range(3)], axis=1).astype(F64)
        prod = P[:, :3, None] * M[:, :, :3] * x[:, None, :]               # n_r m_rc x_c
        shift = P[:, :3] * M[:, :, 3]
        best = np.maximum(best, prod.sum(axis=(1, 2)) + shift.sum(axis=1) + P[:, 3])
        terms = np.maximum(terms, np.abs(prod).sum(axis=(1, 2)) + np.abs(shift).sum(axis=1) + np.abs(P[:, 3]))
    margin = 2.0 ** -20 * terms
    above, below = best > margin, best < -margin
    share = (above | below).mean()
    print(f"{share:.4f} of {count} cases outside the margin band, {above.sum()} above, {below.sum()} below")
    assert share >= 0.95 and above.sum() > 1000 and below.sum() > 1000
    assert (s_p[above] >= 0).all(), np.count_nonzero(~(s_p[above] >= 0))
    assert (s_p[below] < 0).all(), np.count_nonzero(~(s_p[below] < 0))


# ---- 2. the brute force on a hand scene, and the checker --------------------------------------------------------------------------------------------------------------

def hand_scene(pkg):
    """four unit boxes in a row along x under: an identity; a translation by (0, 10, 0); a singular instance (inactive); the row turned by 45 degrees about z
    at (0, 20, 0), whose world box is far larger than its oriented row.  Volumes (six box planes each): 0 around prims 0 and 1 of instance 0 (prim 1 touching at
    x = 2), 1 everything, 2 nothing, 3 a corner of instance 3's world box that none of its leaves reaches, 4 inside prim 3 of instance 1"""
    leaf = as_boxes(np.array([[j, 0, 0, j + 1, 1, 1] for j in (0.0, 2.0, 4.0, 6.0)], dtype=F32))
    inst = make_instances(pkg, [identity(), mat34(np.eye(3), (0.0, 10.0, 0.0)), mat34(np.zeros((3, 3))), mat34(rot(2, np.pi / 4), (0.0, 20.0, 0.0))], [0, 0, 0, 0])
    vols = np.array([box_planes((-1, 0.25, 0.25), (2.0, 0.5, 0.5)), box_planes((-50, -50, -50), (50, 50, 50)), box_planes((100, 100, 100), (101, 101, 101)),
                     box_planes((3, 15, -50), (50, 21, 50)), box_planes((6.25, 10.25, 0.25), (6.5, 10.5, 0.5))], dtype=F64).astype(F32)
    return leaf, inst, vols


def test_brute_force_on_a_hand_scene(pkg):
    leaf, inst, vols = hand_scene(pkg)
    ref = reference(pkg, vols, [leaf], inst)
    assert ref["offsets"].tolist() == [0, 2, 14, 14, 14, 15] and ref["recs"].dtype == pkg.SCENE_CULL_HIT
    r = ref["recs"]
    rows = list(zip(r["instance"].tolist(), r["prim"].tolist(), r["straddle"].tolist(), r["zero"].tolist()))
    # volume 0: box 0 lies inside both x planes and crosses the y and z pairs (bits 2 .. 5); box 1 = [2, 3] touches x <= 2 with its p-vertex and crosses it
    assert rows[:2] == [(0, 0, 0b111100, 0), (0, 1, 0b111110, 0)]
    assert rows[2:14] == [(k, j, 0, 0) for k in (0, 1, 3) for j in range(4)]          # everything: the singular instance 2 never answers
    assert rows[14] == (1, 3, 0b111111, 0)
    # volume 3: instance 3's stored world box passes the world planes — bvh_cull on the top-level tree reports it — while none of its leaves does
    marked, wb = stored_world_boxes([leaf], inst)
    assert marked["blas"].tolist() == [0, 0, 0xFFFFFFFF, 0]
    toff, thits = pkg.cull_brute_force(vols, wb)
    assert thits["prim"][toff[3]:toff[4]].tolist() == [3] and ref["counts"][3] == 0
    check_scene_cull(pkg, ref["offsets"], r, ref, "hand scene")
    # a BLAS index out of range and a NaN in the matrix are inactive too
    for edit in (lambda i: i["blas"].__setitem__(1, 7), lambda i: i["object_to_world"][1].__setitem__(5, np.nan)):
        off_inst = inst.copy(); edit(off_inst)
        assert 1 not in reference(pkg, vols, [leaf], off_inst)["recs"]["instance"]
    # one volume given as (planes, 4); no volumes
    one = pkg.scene_cull_brute_force(vols[0], [leaf], marked, wb)
    assert one[0].tolist() == [0, 2] and one[1].tobytes() == r[:2].tobytes()
    none = pkg.scene_cull_brute_force(vols[:0], [leaf], marked, wb)
    assert none[0].tolist() == [0] and len(none[1]) == 0 and none[1].dtype == pkg.SCENE_CULL_HIT


def test_checker_catches_tampered_slices(pkg):
    leaf, inst, vols = hand_scene(pkg)
    ref = reference(pkg, vols, [leaf], inst)
    off, r = ref["offsets"], ref["recs"]

    def shifted(at, by):
        o = off.astype(np.int64); o[at:] += by
        return o.astype(np.uint32)

    def edited(i, field, value):
        c = r.copy(); c[field][i] = value
        return c
    cases = {
        "a missing pair": (shifted(1, -1), np.delete(r, 1)),
        "a missing slice": (shifted(5, -1), np.delete(r, 14)),
        "a duplicated pair": (shifted(2, 1), np.insert(r, 3, r[2])),
        "a pair twice in place of another": (off, np.concatenate([r[:3], r[2:3], r[4:]])),
        "a wrong straddle": (off, edited(0, "straddle", 0b111101)),
        "a straddle mask on an inside box": (off, edited(5, "straddle", 1)),
        "a non-zero zero word": (off, edited(7, "zero", 1)),
        "an inactive instance": (off, edited(6, "instance", 2)),
        "an off-by-one offset": (np.concatenate([off[:1], off[1:2] - 1, off[2:]]).astype(np.uint32), r),
        "offsets that do not end at the total": (shifted(5, 1), r),
        "offsets that do not start at 0": (shifted(0, 1), r),
    }
    for what, (o, recs) in cases.items():
        with pytest.raises(AssertionError):
            check_scene_cull(pkg, o, recs, ref, what)
    check_scene_cull(pkg, off, r[np.r_[1, 0, 13:1:-1, 14]], ref, "any order inside a slice")


# ---- 3. the GPU tests' inputs -----------------------------------------------------------------------------------------------------------------------------------------

def frustum_unit_planes(clip):
    """pkg.frustum_planes' six planes (0 <= z <= w) in f64 with unit normals: planes need not be normalised, but a scene scaled by 2^64 needs planes that fit f32"""
    r0, r1, r2, r3 = np.asarray(clip, dtype=F64)
    pl = np.stack([r3 + r0, r3 - r0, r3 + r1, r3 - r1, r2, r3 - r2])
    return pl / np.linalg.norm(pl[:, :3], axis=1, keepdims=True)


def cut(planes6, per):
    """six planes as ``per``: 8 pads with (0, 0, 0, 1); 4 and 1 keep the first ones (a box's x and y slabs, a frustum's sides; its first plane)"""
    return (list(planes6) + [PADDING, PADDING])[:per]


def scene_volumes(pkg, blas_leaf, inst, per, seed, m=N_VOLUMES, unit_frusta=False):
    """m volumes of ``per`` planes around the world leaf boxes of a scene, by i % 8: 0 a camera frustum from pkg.frustum_planes (``unit_frusta``: the same
    planes normalised in f64), 1 holds everything (the first 16; later ones a large box), 2 holds nothing (a far box), 3 a zero-thickness slab exactly through
    a face of a world leaf box (per 1: the half-space that ends there), 4 nothing again — the far box's planes scaled by 2^-6 with its last two replaced by
    padding planes —, 5 a large box whose normals' zeros are -0, 6 a small box around a world leaf box, 7 a large box.  Returns f32 (m, per, 4)"""
    rng = np.random.default_rng(seed)
    wl = world_leaf_boxes(blas_leaf, inst)
    lo, hi = wl["min"].astype(F64).min(axis=0), wl["max"].astype(F64).max(axis=0)
    ext = np.maximum(hi - lo, 1e-30); ctr = 0.5 * (lo + hi); diag = float(np.linalg.norm(ext))
    far_box = box_planes(hi + 10.0 * ext, hi + 11.0 * ext)
    out = np.zeros((m, per, 4), dtype=F64)
    for i in range(m):
        kind = i % 8
        src = wl[rng.integers(0, len(wl))]
        at = 0.5 * (src["min"].astype(F64) + src["max"])
        if kind == 0:
            eye = ctr + rng.normal(size=3) * ext * rng.choice([0.3, 1.5]); target = lo + rng.random(3) * ext
            if np.linalg.norm(target - eye) < 1e-3 * diag:
                target = eye + (0.0, 0.0, -diag)
            near = rng.choice([0.01, 0.2]); far = near + rng.choice([0.3, 3.0])    # in units of the scene's diagonal, like the camera: the planes' offsets are
            clip = perspective(np.radians(rng.uniform(10.0, 100.0)), rng.choice([1.0, 16.0 / 9.0]), near, far) @ look_at(eye / diag, target / diag) @ np.diag([1.0, 1.0, 1.0, diag])   # scaled back
            six = frustum_unit_planes(clip) if unit_frusta else pkg.frustum_planes(clip).astype(F64)
        elif kind == 1 and i < 16:
            six = box_planes(lo - ext, hi + ext)
        elif kind == 2:
            six = far_box
        elif kind == 3:
            f = float(src["min"][0])
            six = [(1.0, 0.0, 0.0, -f), (-1.0, 0.0, 0.0, f)] + box_planes(lo - ext, hi + ext)[2:]
        elif kind == 4:
            six = [tuple(2.0 ** -6 * np.array(p)) for p in far_box[:4]] + [PADDING, PADDING]
        elif kind == 6:
            h = rng.random(3) * 0.03 * ext
            six = box_planes(at - h, at + h)
        else:
            c = lo + rng.random(3) * ext; h = (0.15 + rng.random(3) * 0.35) * ext
            six = box_planes(c - h, c + h)
            if kind == 5:
                six = [tuple(-0.0 if v == 0.0 else v for v in p[:3]) + (p[3],) for p in six]
        out[i] = np.array(cut(six, per), dtype=F64)
    return out.astype(F32)


def premises(what, inst, n_blas, vols, ref, empty=50, long=50, inactive=()):
    """what every input set must contain for the tests to mean something, asserted on the brute force alone"""
    counts = ref["counts"]
    _, active = active_instances(inst, n_blas)
    r = ref["recs"]
    seen = [set(r["instance"][ref["offsets"][i]:ref["offsets"][i + 1]].tolist()) for i in range(len(counts))]
    everyone = set(np.nonzero(active)[0].tolist())
    print(f"{what}: {len(vols)} volumes, {(counts == 0).sum()} empty slices, {(counts > 32).sum()} longer than 32, longest {counts.max()}, {counts.sum()} records, "
          f"{sum(s == everyone for s in seen)} volumes touch every instance")
    assert (counts == 0).sum() >= empty, f"{what}: {(counts == 0).sum()} empty slices"
    assert (counts > 32).sum() >= long, f"{what}: {(counts > 32).sum()} slices longer than 32"
    assert any(s == everyone for s in seen), f"{what}: no volume touches every instance"
    assert not set(r["instance"].tolist()) & set(inactive), f"{what}: an inactive instance in the brute force"
    assert (r["straddle"] == 0).any() and (r["straddle"] != 0).any(), f"{what}: the straddle masks are all zero or all non-zero"
    assert np.isfinite(vols).all()


def cull_scene_inputs(pkg, n_inst, per):
    """four meshes of 2 to 2000 triangles (mesh_sizes); n_inst instances of every kind of tests/test_gpu_scene.py (identity, translation, rotation, non-uniform scale,
    mirror), every sixth sheared, the trailing ones inactive -> (meshes, inst, volumes, brute force)"""
    def make():
        rng = np.random.default_rng(n_inst)
        meshes = [no_negzero(pkg.meshgen.uniform(n, 31 + n)) for n in mesh_sizes(n_inst)]
        inst = with_shear(pkg, rng, scene_instances(pkg, rng, n_inst, 4, 1.5), n_inst - len(inactive_of(n_inst)))
        leaf = [tri_leaf_boxes(t) for t in meshes]
        vols = scene_volumes(pkg, leaf, inst, per, 500 + 8 * n_inst + per)
        return meshes, inst, vols, reference(pkg, vols, leaf, inst)
    return cached(("scene cull", n_inst, per), make)


def cull_coincident_inputs(pkg, seed):
    """tests/test_scene_knn.py's tie setup: a mesh and the same mesh with a far-off extra triangle appended, under two identity instances"""
    def make():
        mesh, stretched, inst, _ = coincident_inputs(pkg, seed)
        return mesh, stretched, inst, scene_volumes(pkg, [tri_leaf_boxes(mesh), tri_leaf_boxes(stretched)], inst, 6, 19 + seed)
    return cached(("scene cull coincident", seed), make)


def cull_moved_inputs(pkg):
    """tests/test_scene_knn.py's update setup: two meshes, 64 instances as built and as moved (kinds, BLASes and the inactive ones change), the first mesh
    jittered for the refit -> (meshes, inst, moved, volumes, refit meshes, brute force after the move, brute force after the refit)"""
    def make():
        meshes, inst, moved, _, refit, _, _ = moved_inputs(pkg)
        leaf, leaf_refit = [tri_leaf_boxes(t) for t in meshes], [tri_leaf_boxes(t) for t in refit]
        vols = scene_volumes(pkg, leaf, moved, 6, 23)
        return meshes, inst, moved, vols, refit, reference(pkg, vols, leaf, moved), reference(pkg, vols, leaf_refit, moved)
    return cached(("scene cull moved",), make)


def cull_small_inputs(pkg):
    """the scene of the capacity and error tests: uniform(300) under an identity and a translated instance, 200 volumes of 6 planes"""
    def make():
        mesh = no_negzero(pkg.meshgen.uniform(300, 3))
        inst = make_instances(pkg, [identity(), mat34(np.eye(3), (0.5, 0, 0))], [0, 0])
        vols = scene_volumes(pkg, [tri_leaf_boxes(mesh)], inst, 6, 4, m=200)
        return mesh, inst, vols, reference(pkg, vols, [tri_leaf_boxes(mesh)], inst)
    return cached(("scene cull small",), make)


def cull_deep_inputs(pkg, H):
    """test_gpu_query.caterpillar of height H under five translated instances.  Volumes by i % 4: 0 everything of the instance i is aimed at, 1 a z slab over
    a run of its far side nodes, 2 its near triangle alone, 3 nothing -> (tris, nodes, root, n, inst, volumes, brute force)"""
    def make():
        tris, nodes, root, n = caterpillar(pkg, H, 3 + H)
        offs = np.array(DEEP_OFFSETS, dtype=F64)
        inst = make_instances(pkg, [mat34(np.eye(3), t) for t in offs], [0] * len(offs))
        rng = np.random.default_rng(H)
        m = 256
        aimed = rng.integers(0, len(offs), m)
        vols = np.zeros((m, 6, 4))
        for i in range(m):
            a, w = rng.uniform(0, 2 * H - 1), rng.uniform(0, 40)
            q = np.array([(-20, -20, -100, 40, 40, 5000), (-1, -1, 1000 + a, 1, 1, 1000 + a + w), (-1, -1, 0, 1, 1, 0.25), (-1, -1, 0.625, 1, 1, 999)][i % 4], dtype=F64)
            vols[i] = box_planes(q[:3] + offs[aimed[i]], q[3:] + offs[aimed[i]])
        vols = vols.astype(F32)
        return tris, nodes, root, n, inst, vols, reference(pkg, vols, [tri_leaf_boxes(tris)], inst)
    return cached(("scene cull deep", H), make)


def cull_deep_top_inputs(pkg):
    """tests/test_deep_trees.py's deep top level (the construction of test_scene_overlap.overlap_deep_top_inputs): 180 instances of a mesh of 8 triangles on the
    staircase.  Even volumes hold every instance (1440 records), odd ones a box around a single instance -> (mesh, inst, volumes, brute force)"""
    def make():
        mesh = no_negzero(pkg.meshgen.uniform(8, 5))
        p, base = stairs_steps(*STAIRS)
        inst = make_instances(pkg, [mat34(np.eye(3) * (0.05 * p[k]), base[k]) for k in range(len(p))], [0] * len(p))
        rng = np.random.default_rng(6)
        m = 128
        k = rng.integers(0, len(inst), m)
        vols = np.array([box_planes(base[k[i]] - 0.1 * p[k[i]], base[k[i]] + 0.2 * p[k[i]]) if i % 2 else box_planes((-1.0,) * 3, (1.0e19,) * 3) for i in range(m)])
        vols = vols.astype(F32)
        return mesh, inst, vols, reference(pkg, vols, [tri_leaf_boxes(mesh)], inst)
    return cached(("scene cull deep top",), make)


def cull_fat_inputs(pkg, levels):
    """test_cull.fat_caterpillar(levels) under one identity instance, 24 volumes: 0 and 11 hold everything, the others scene_volumes' -> (leaf, nodes, root, n,
    inst, volumes, brute force)"""
    def make():
        leaf, nodes, root, n = fat_caterpillar(pkg, levels)
        inst = make_instances(pkg, [identity()], [0])
        vols = scene_volumes(pkg, [leaf], inst, 6, 5, m=24)
        vols[0] = vols[1]; vols[11] = vols[1]
        return leaf, nodes, root, n, inst, vols, reference(pkg, vols, [leaf], inst)
    return cached(("scene cull fat", levels), make)


def ladder_inputs(pkg, name):
    """a rung of tests/test_scene_extremes.py's instance ladder with 64 volumes of 6 unit-normal planes around its world leaf boxes -> (inst, volumes, brute
    force, whether the brute force met a NaN)"""
    def make():
        inst = rung_instances(pkg, name)
        leaf = [tri_leaf_boxes(t) for t in ladder_meshes(pkg)]
        with np.errstate(all="ignore"):
            vols = scene_volumes(pkg, leaf, inst, 6, 70 + RUNGS.index(name), m=64, unit_frusta=True)
            return inst, vols, reference(pkg, vols, leaf, inst), has_nan(pkg, vols, leaf, inst)
    return cached(("scene cull ladder", name), make)


@pytest.mark.parametrize("n_inst", SCENE_N_INST)
def test_scene_inputs(pkg, n_inst):
    for per in PLANE_COUNTS:
        meshes, inst, vols, ref = cull_scene_inputs(pkg, n_inst, per)
        assert [len(t) for t in meshes] == mesh_sizes(n_inst) and vols.shape == (N_VOLUMES, per, 4)
        premises(f"{n_inst} instances x {per} planes", inst, 4, vols, ref, inactive=inactive_of(n_inst))
        check_scene_cull(pkg, ref["offsets"], ref["recs"], ref)
        if per >= 6:
            assert (ref["counts"][2::8] == 0).all() and (ref["counts"][4::8] == 0).all()
            assert (np.signbit(vols[5::8, :, :3]) & (vols[5::8, :, :3] == 0)).any() and (vols[4::8, 4:6] == np.array(PADDING, dtype=F32)).all()
        if per >= 4:
            assert (ref["counts"][3::8] >= 1).all(), "a slab through a face of a world leaf box holds no leaf"


def test_other_inputs(pkg):
    for seed in (0, 3):
        mesh, stretched, inst, vols = cull_coincident_inputs(pkg, seed)
        for blas in ([mesh, stretched], [stretched, mesh]):
            ref = reference(pkg, vols, [tri_leaf_boxes(t) for t in blas], inst)
            premises("coincident", inst, 2, vols, ref)
            r, q = ref["recs"], slice_queries(ref["offsets"])
            shared = r["prim"] < len(mesh)
            a, b = shared & (r["instance"] == 0), shared & (r["instance"] == 1)
            assert a.sum() == b.sum() > 1000 and np.array_equal(q[a], q[b]) and np.array_equal(r["prim"][a], r["prim"][b]) and np.array_equal(r["straddle"][a], r["straddle"][b])
    meshes, inst, moved, vols, refit, ref_moved, ref_refit = cull_moved_inputs(pkg)
    premises("after update", moved, 2, vols, ref_moved, inactive={61, 62, 63})
    premises("after BLAS refit", moved, 2, vols, ref_refit, inactive={61, 62, 63})
    assert ref_moved["recs"].tobytes() != ref_refit["recs"].tobytes()
    assert reference(pkg, vols, [tri_leaf_boxes(t) for t in meshes], inst)["recs"].tobytes() != ref_moved["recs"].tobytes()
    mesh, inst, vols, ref = cull_small_inputs(pkg)
    premises("small", inst, 1, vols, ref, empty=40, long=40)
    for H in (300, 20):
        tris, nodes, root, n, inst, vols, ref = cull_deep_inputs(pkg, H)
        assert (ref["counts"][::4] == n).all() and (ref["counts"][3::4] == 0).all() and (ref["counts"][2::4] == 1).all()
    mesh, inst, vols, ref = cull_deep_top_inputs(pkg)
    assert (ref["counts"][::2] == 180 * 8).all() and (ref["counts"][1::2] >= 1).all() and ref["counts"][1::2].max() <= 64


def test_ladder_classes(pkg):
    """which rungs the brute force calls exact is decided by the brute force — but the finite uniform scales up to 2^+-64, the shear rungs and the offset rungs
    must be among them, so that the GPU test cannot pass by calling everything ill-conditioned"""
    exact = [name for name in RUNGS if not ladder_inputs(pkg, name)[3]]
    print("rungs without a NaN:", exact)
    assert set(UNI + SHEAR + FAR) <= set(exact), sorted(set(UNI + SHEAR + FAR) - set(exact))
    for name in RUNGS:
        inst, vols, ref, _ = ladder_inputs(pkg, name)
        assert ref["counts"].sum() > 100 and (ref["counts"] == 0).sum() >= 8, (name, ref["counts"].sum())


# ---- 4. the host restatements of the two walks ------------------------------------------------------------------------------------------------------------------------

class HostScene:
    """a scene as the kernels read it: the top-level tree (None with one instance) over the stored world boxes, per instance its activity, matrix and BLAS tree"""

    def __init__(self, pkg, top, trees, inst, blas_leaf):
        self.pkg, self.top, self.trees = pkg, top, trees
        self.marked, self.wb = stored_world_boxes(blas_leaf, inst)
        self.active = (self.marked["blas"] != 0xFFFFFFFF).tolist()
        self.n_inst = len(inst)

    def top_pass(self, volume):
        """per top-level record: does its box pass the world planes"""
        t = self.top
        s_p, _ = self.pkg.cull_plane_values(volume[:, None, :], t.lo[None], t.hi[None])
        with np.errstate(invalid="ignore"):
            return ((t.lo <= t.hi).all(axis=1) & (s_p >= F32(0.0)).all(axis=0)).tolist()

    def world_box_pass(self, volume, k):
        s_p, _ = self.pkg.cull_plane_values(volume, self.wb[k, :3], self.wb[k, 3:])
        return bool((self.wb[k, :3] <= self.wb[k, 3:]).all() and (s_p >= F32(0.0)).all())

    def blas_tests(self, volume, k):
        """(tree, per record: passes the object planes of (volume, k), per record: straddle mask)"""
        tree = self.trees[int(self.marked["blas"][k])]
        obj = self.pkg.scene_cull_object_planes(volume, self.marked["object_to_world"][k])
        s_p, s_n = self.pkg.cull_plane_values(obj[:, None, :], tree.lo[None], tree.hi[None])
        bits = (np.uint32(1) << np.arange(len(volume), dtype=np.uint32))[:, None]
        with np.errstate(invalid="ignore"):
            ok = (tree.lo <= tree.hi).all(axis=1) & (s_p >= F32(0.0)).all(axis=0)
            mask = np.where(s_n >= F32(0.0), np.uint32(0), bits).sum(axis=0, dtype=np.uint32)
        return tree, ok.tolist(), mask.tolist()


def records(pkg, rows):
    """rows of (prim, instance, straddle) in the given order as SCENE_CULL_HIT records"""
    rec = np.zeros(len(rows), dtype=pkg.SCENE_CULL_HIT)
    if rows:
        a = np.array(rows, dtype=np.int64)
        rec["prim"], rec["instance"], rec["straddle"] = a[:, 0], a[:, 1], a[:, 2]
    return rec


def scene_lane_walk(sc, volume):
    """k_scene_cull_walk restated: one stack for both levels; per internal node both children are tested; of two passing children the left is entered and the
    right pushed; at the top level a passing leaf is an instance, entered like a node (when it is popped, if it was pushed); in a BLAS a passing leaf is
    reported at once.  Neither root's own box is tested; a one-instance scene tests its world box.  Returns (records in walk order, deepest stack)"""
    top = sc.top
    out, stack, deepest = [], [], 0
    if top is None:
        cur = ("E", 0) if sc.world_box_pass(volume, 0) else None
    else:
        tpass = sc.top_pass(volume)
        cur = ("T", top.root)
    inst = tree = ok = mask = None
    while True:
        if cur is None:
            if not stack:
                break
            tag, v = stack.pop()
            cur = ("B", v) if tag == "B" else ("T", v) if v < top.ni else ("E", top.prims[v - top.ni])
            continue
        tag, v = cur
        if tag == "E":
            if v < sc.n_inst and sc.active[v]:
                inst = v; tree, ok, mask = sc.blas_tests(volume, v); cur = ("B", tree.root)
            else:
                cur = None
        elif tag == "B":
            kids = []
            for c in tree.kids[v]:
                if ok[c]:
                    if c >= tree.ni:
                        out.append((tree.prims[c - tree.ni], inst, mask[c]))
                    else:
                        kids.append(c)
            if len(kids) == 2:
                stack.append(("B", kids[1])); deepest = max(deepest, len(stack))
            cur = ("B", kids[0]) if kids else None
        else:
            kids = [c for c in top.kids[v] if tpass[c]]
            if len(kids) == 2:
                stack.append(("T", kids[1])); deepest = max(deepest, len(stack))
            cur = None if not kids else ("T", kids[0]) if kids[0] < top.ni else ("E", top.prims[kids[0] - top.ni])
    return records(sc.pkg, out), deepest


def scene_group_walk(sc, volume):
    """k_scene_cull_group's schedule restated: the work stack holds {instance, node} entries, instance None at the top level; each round takes the
    m = min(top, 256) entries at the top, thread t entry top - m + t; a thread on a top-level entry tests both children with the world planes, pushes a passing
    internal child and pushes a passing leaf whose instance is active as {k, that BLAS's root}; a thread on a BLAS entry tests both children with its instance's
    object planes, emits leaf survivors and pushes internal ones; emits and pushes in thread order, left before right.  Returns (records in emission order,
    the largest occupancy after a round's pushes — what the kernel compares with BVH_SCENE_CULL_GROUP_STACK)"""
    top = sc.top
    tests = {}

    def blas(k):
        if k not in tests:
            tests[k] = sc.blas_tests(volume, k)
        return tests[k]
    if top is None:
        stack = [(0, blas(0)[0].root)] if sc.active[0] and sc.world_box_pass(volume, 0) else []
    else:
        tpass = sc.top_pass(volume)
        stack = [(None, top.root)]
    out, peak = [], len(stack)
    while stack:
        m = min(len(stack), GROUP_BLOCK)
        ent = stack[len(stack) - m:]
        del stack[len(stack) - m:]
        for k, v in ent:
            if k is None:
                for c in top.kids[v]:
                    if tpass[c]:
                        if c < top.ni:
                            stack.append((None, c))
                        else:
                            j = top.prims[c - top.ni]
                            if j < sc.n_inst and sc.active[j]:
                                stack.append((j, blas(j)[0].root))
            else:
                tree, ok, mask = blas(k)
                for c in tree.kids[v]:
                    if ok[c]:
                        if c < tree.ni:
                            stack.append((k, c))
                        else:
                            out.append((tree.prims[c - tree.ni], k, mask[c]))
        peak = max(peak, len(stack))
    return records(sc.pkg, out), peak


def host_top_level(pkg, wb):
    """a top-level tree for the host walks: median splits of the world boxes' centres (inverted boxes of inactive instances included, as leaves that never
    pass), internal boxes the fmin / fmax of their children's — any tree with nested boxes gives the same sets.  Returns a test_cull.Tree"""
    n = len(wb); ni = n - 1
    nodes = np.zeros(2 * n - 1, dtype=pkg.BVH2_NODE)
    nodes["min"][ni:] = wb[:, :3]; nodes["max"][ni:] = wb[:, 3:]; nodes["left"][ni:] = np.arange(n); nodes["right"][ni:] = pkg.INVALID
    ctr = 0.5 * (wb[:, :3].astype(F64) + wb[:, 3:])
    nxt = [0]

    def build(idx):
        if len(idx) == 1:
            return ni + int(idx[0])
        v = nxt[0]; nxt[0] += 1
        ax = int(np.argmax(ctr[idx].max(axis=0) - ctr[idx].min(axis=0)))
        idx = idx[np.argsort(ctr[idx, ax], kind="stable")]
        a, b = build(idx[: len(idx) // 2]), build(idx[len(idx) // 2:])
        nodes["left"][v], nodes["right"][v] = a, b
        nodes["min"][v] = np.fmin(nodes["min"][a], nodes["min"][b]); nodes["max"][v] = np.fmax(nodes["max"][a], nodes["max"][b])
        return v
    root = build(np.arange(n))
    return Tree(nodes, None, root, n, 0)


def oracle_trees(pkg, orc, meshes, algos):
    trees = []
    for algo, tris in zip(algos, meshes):
        t = orc.build_tree(algo, tris)
        assert leaf_boxes_of(t["nodes"], t["leaves"], len(tris), t["layout"]).tobytes() == tri_leaf_boxes(tris).tobytes()
        trees.append(Tree(t["nodes"], t["leaves"], t["root"], len(tris), t["layout"]))
    return trees


@pytest.mark.parametrize("n_inst", SCENE_N_INST)
def test_host_walks_equal_the_brute_force(pkg, orc, n_inst):
    """both restatements return the brute force's records and masks on the oracle's trees of all four builders (BLAS b from builder b; with one or two
    instances the BLASes in use are rebuilt by every builder in turn); the largest occupancies seen are reported"""
    meshes, inst, vols, ref = cull_scene_inputs(pkg, n_inst, 6)
    leaf = [tri_leaf_boxes(t) for t in meshes]
    slices = [ref["recs"][ref["offsets"][i]:ref["offsets"][i + 1]] for i in range(N_VOLUMES)]
    pick = list(range(0, 16)) + list(range(16, N_VOLUMES, 24))
    rotations = range(4) if n_inst <= 2 else (0,)
    deepest = peak = checked = 0
    for r in rotations:
        trees = oracle_trees(pkg, orc, meshes, [(b + r) % 4 for b in range(4)])
        sc = HostScene(pkg, None, trees, inst, leaf)
        if n_inst > 1:
            sc.top = host_top_level(pkg, sc.wb)
        for i in pick:
            got, d = scene_lane_walk(sc, vols[i])
            assert scene_cull_host_sort(np.array([0, len(got)]), got).tobytes() == slices[i].tobytes(), f"{n_inst} instances, builders + {r}, volume {i}: lane walk"
            grp, p = scene_group_walk(sc, vols[i])
            assert scene_cull_host_sort(np.array([0, len(grp)]), grp).tobytes() == slices[i].tobytes(), f"{n_inst} instances, builders + {r}, volume {i}: group walk"
            deepest, peak, checked = max(deepest, d), max(peak, p), checked + 1
    print(f"{n_inst} instances: {checked} volumes walked, lane stack up to {deepest} of {QUERY_STACK}, group stack up to {peak} of {pkg.SCENE_CULL_GROUP_STACK}")
    assert deepest <= QUERY_STACK and peak <= pkg.SCENE_CULL_GROUP_STACK and any(len(slices[i]) > 32 for i in pick) and any(len(slices[i]) == 0 for i in pick)


def test_group_schedule_occupancy_on_one_instance(pkg):
    """a one-instance scene over test_cull.fat_caterpillar: the first entry is {0, root}, so the occupancy is bvh_cull's on the BLAS — above
    BVH_SCENE_CULL_GROUP_STACK at 32 levels (8448), exactly full at 31 (8192) — and both answers equal the brute force"""
    for levels, over in ((32, True), (31, False)):
        leaf, nodes, root, n, inst, vols, ref = cull_fat_inputs(pkg, levels)
        sc = HostScene(pkg, None, [Tree(nodes, None, root, n, 0)], inst, [leaf])
        got, peak = scene_group_walk(sc, vols[0])
        assert (peak > pkg.SCENE_CULL_GROUP_STACK) == over and peak == 256 * (levels - 1) + 512, (levels, peak)
        assert len(got) == n and scene_cull_host_sort(np.array([0, n]), got).tobytes() == ref["recs"][: ref["offsets"][1]].tobytes()
        peaks = [scene_group_walk(sc, v)[1] for v in vols[1:]]
        assert peaks[10] == peak and any(p < pkg.SCENE_CULL_GROUP_STACK // 2 for p in peaks)


def test_deep_inputs_need_what_the_gpu_tests_say(pkg):
    """the caterpillar BLAS of height 300 needs more than QUERY_STACK entries of the lane walk's stack for a volume that holds an instance, height 20 does not;
    the covering volumes of the staircase scene need more at the top level on a chain-shaped top-level tree"""
    for H, deep in ((300, True), (20, False)):
        tris, nodes, root, n, inst, vols, ref = cull_deep_inputs(pkg, H)
        sc = HostScene(pkg, None, [Tree(nodes, None, root, n, 0)], inst, [tri_leaf_boxes(tris)])
        sc.top = host_top_level(pkg, sc.wb)
        need = [scene_lane_walk(sc, vols[i])[1] for i in range(8)]
        print(f"caterpillar {H}: stack need {need}")
        assert (max(need[::4]) > QUERY_STACK) == deep and min(need[2::4] + need[3::4]) + len(inst) <= QUERY_STACK, need
        if not deep:
            assert max(need) + len(inst) <= QUERY_STACK
        for i in range(8):
            got, _ = scene_lane_walk(sc, vols[i])
            assert scene_cull_host_sort(np.array([0, len(got)]), got).tobytes() == ref["recs"][ref["offsets"][i]:ref["offsets"][i + 1]].tobytes()


# ---- 5. the ABI -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_type_and_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    assert re.search(r"typedef struct\s*\{\s*uint32_t prim;\s*uint32_t instance;\s*uint32_t straddle;\s*uint32_t zero;\s*\}\s*bvh_scene_cull_hit;", text)
    assert re.search(r"#define\s+BVH_SCENE_CULL_GROUP_STACK\s+8192\b", text)
    assert re.search(r"\bint\s+bvh_scene_cull\s*\(\s*bvh_scene\s*\*\s*\w+\s*,\s*const float\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*int\s+\w+\s*,\s*"
                     r"uint32_t\s*\*\s*\w+\s*,\s*bvh_scene_cull_hit\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"\bint\s+bvh_ctx_query_overflow\s*\(\s*bvh_ctx\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)", text)


def test_library_exports_the_symbol_and_sizes_match(pkg, tmp_path):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_scene_cull") and "bvh_scene_cull" in pkg.EXPORTS and hasattr(L, "bvh_ctx_query_overflow") and "bvh_ctx_query_overflow" in pkg.EXPORTS
    assert pkg.SCENE_CULL_GROUP_STACK == 8192 and pkg.SCENE_CULL_HIT.itemsize == 16 == C.sizeof(CSceneCullHit)
    assert pkg.SCENE_CULL_HIT.names == ("prim", "instance", "straddle", "zero")
    offs = [pkg.SCENE_CULL_HIT.fields[name][1] for name in pkg.SCENE_CULL_HIT.names]
    assert offs == [getattr(CSceneCullHit, f[0]).offset for f in CSceneCullHit._fields_] == [0, 4, 8, 12]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvh_mi355x.h"\nint main(void) { printf("%zu %zu %zu %zu %zu", sizeof(bvh_scene_cull_hit), '
                   'offsetof(bvh_scene_cull_hit, prim), offsetof(bvh_scene_cull_hit, instance), offsetof(bvh_scene_cull_hit, straddle), '
                   'offsetof(bvh_scene_cull_hit, zero)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["g++", "-std=c++17", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout == "16 0 4 8 12"


def test_binding_and_errors_without_a_device(pkg):
    assert callable(getattr(pkg.Scene, "cull")) and callable(getattr(pkg.Scene, "cull_instances")) and callable(getattr(pkg.Context, "query_overflow"))
    L = pkg.lib()
    f = L.bvh_scene_cull
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    assert f.argtypes == [vp, vp, u32, u32, C.c_int32, vp, vp, u64, C.POINTER(u64)] and f.restype == C.c_int32
    total = C.c_uint64(0x77)
    assert f(None, 4096, 1, 6, 0, 8192, 16384, 16, C.byref(total)) == E_INVALID             # a NULL scene is refused before anything else is looked at
    assert f(None, None, 0, 6, 0, None, None, 0, None) == E_INVALID
    for per, path in ((0, 0), (9, 0), (6, 3), (6, -1)):
        assert f(None, 4096, 1, per, path, 8192, 16384, 16, C.byref(total)) == E_INVALID
    assert total.value == 0x77
    assert L.bvh_ctx_query_overflow(None, None, None) == E_INVALID
    with pytest.raises(pkg.BvhError):
        pkg.scene_cull_brute_force(np.zeros((2, 9, 4), dtype=F32), [np.zeros((1, 6), dtype=F32)], make_instances(pkg, [identity()], [0]), np.zeros((1, 6), dtype=F32))


def test_kernels_use_no_scratch_and_the_stacks_are_what_the_header_says(pkg, tmp_path):
    got = _code_object(os.path.join(ROOT, "hip-bvh-construction_amd", "csrc", "scene_cull.o"), str(tmp_path))
    if got is None:
        pytest.skip("LLVM tools or the object file are missing")
    _, notes = got
    seen = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "k_scene_cull_" in name:
            seen[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)),
                          int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)), int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)))
    kinds = {k: [n for n in seen if f"k_scene_cull_{k}" in n] for k in ("walk", "group", "deep")}
    assert all(len(v) == 2 for v in kinds.values()) and len(seen) == 6, sorted(seen)      # count and fill of each
    for name, (scratch, lds, vgprs) in seen.items():
        print(name, "vgprs", vgprs, "lds", lds)
        assert scratch == 0, (name, "spills to scratch", scratch)
        if name in kinds["walk"]:
            assert lds == QUERY_STACK * 64 * 4 == 16 * 1024, (name, lds)
        elif name in kinds["group"]:
            assert lds == 2 * 4 * pkg.SCENE_CULL_GROUP_STACK + 4 * 2 * 4 == 64 * 1024 + 32, (name, lds)     # two u32 columns and four waves' two partial sums
        else:
            assert lds == 0, (name, lds)


def test_every_source_of_the_makefile_is_in_the_variant_build():
    """tools/build_variant.sh compiles its own list of translation units: a source missing there links a variant library with undefined launch symbols"""
    mk = open(os.path.join(ROOT, "hip-bvh-construction_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", mk, flags=re.M).group(1).split()
    assert "scene_cull.hip" in srcs and "cull.hip" in srcs
    script = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    listed = set(re.findall(r"-c (\w+)\.hip", script))
    for line in re.findall(r"^for f in ([\w ]+); do", script, flags=re.M):
        listed |= set(line.split())
    assert listed == {s[:-4] for s in srcs}, sorted(listed ^ {s[:-4] for s in srcs})
