"""hip-bvh-construction_amd — MI355X-native BVH construction (LBVH / PLOC++ / HPLOC) behind the reference's builder API.

The product is the C-ABI shared library ``libbvh_mi355x.so`` (HIP kernels for gfx950, ``csrc/``; header
``include/bvh_mi355x.h``).  This Python package is only the test / bench harness around it: a ctypes binding plus a
mirror of the reference's builder classes (``TwoPassLbvh`` / ``SinglePassLbvh`` / ``PLOCNew`` / ``HPLOC`` ``.build(context,
triangles)``, reference ``src/TwoPassLbvh.h:12-32`` etc.) so that parity tests read like the reference's own driver
(``src/main.cpp:52-65``).  The C++ mirror of the same classes is ``include/bvh/builders.hpp``.

There is no CPU fallback: every entry point fails loudly (``BvhError``) if the native library or a GPU is missing.
The directory name contains a hyphen; import it with ``bvh_pkg.load()`` from the repo root (or importlib).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import weakref

import numpy as np

from . import meshgen  # noqa: F401
from .meshgen import TRIANGLE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BVH_MI355X_LIB", os.path.join(_HERE, "libbvh_mi355x.so"))   # override: A/B builds of the same ABI

AABB = np.dtype([("min", "<f4", 3), ("max", "<f4", 3)])
BVH2_NODE = np.dtype([("left", "<u4"), ("right", "<u4"), ("min", "<f4", 3), ("max", "<f4", 3)])
PRIMREF = np.dtype([("prim", "<u4"), ("min", "<f4", 3), ("max", "<f4", 3)])
BVH4_NODE = np.dtype([("aabb", AABB, 4), ("child", "<u4", 4), ("parent", "<u4"), ("count", "<u4"), ("pad", "<u4", 2)])
PRIM_NODE = np.dtype([("prim", "<u4"), ("parent", "<u4")])
RAY = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("tmin", "<f4"), ("tmax", "<f4")])
HIT = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])      # bvh_hit (bvh_intersect)
INSTANCE = np.dtype([("object_to_world", "<f4", 12), ("blas", "<u4"), ("reserved", "<u4", 3)])                 # bvh_instance (row-major 3x4)
INSTANCE_HIT = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4"), ("instance", "<u4"), ("reserved", "<u4", 3)])   # bvh_instance_hit
INSTANCE_POINT_HIT = np.dtype([("point", "<f4", 3), ("dist2", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4"), ("instance", "<u4")])   # bvh_instance_point_hit
POINT_QUERY = np.dtype([("point", "<f4", 3), ("radius", "<f4")])                                               # bvh_point_query (bvh_closest_point)
POINT_HIT = np.dtype([("point", "<f4", 3), ("dist2", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4"), ("reserved", "<u4")])   # bvh_point_hit
WINDING_MOMENT = np.dtype([("a", "<f4", 3), ("area", "<f4"), ("p", "<f4", 3), ("r", "<f4")])                               # bvh_winding_moment (bvh_winding_prepare)
WINDING_MAP = np.dtype([("c", "<f4", 9), ("smax", "<f4"), ("reserved", "<u4", 6)])                                          # bvh_winding_map (bvh_scene_winding_prepare)
SCENE_WINDING_KEEP_BLAS = 1
KNN_HIT = np.dtype([("dist2", "<f4"), ("prim", "<u4")])                                                         # bvh_knn_hit (bvh_knn)
KNN_MAX_K = 32
TRI_HIT = np.dtype([("dist2", "<f4"), ("prim", "<u4"), ("feature", "<u4"), ("reserved", "<u4")])                   # bvh_tri_hit (bvh_closest_tris)
INSTANCE_KNN_HIT = np.dtype([("dist2", "<f4"), ("prim", "<u4"), ("instance", "<u4"), ("reserved", "<u4")])         # bvh_instance_knn_hit (bvh_scene_knn, bvh_scene_radius_search)
INSTANCE_TRI_HIT = np.dtype([("dist2", "<f4"), ("prim", "<u4"), ("feature", "<u4"), ("instance", "<u4")])          # bvh_instance_tri_hit (bvh_scene_closest_tris, bvh_scene_radius_tris)
INSTANCE_PRIM = np.dtype([("prim", "<u4"), ("instance", "<u4")])                                                   # bvh_instance_prim (bvh_scene_overlap)
CULL_HIT = np.dtype([("prim", "<u4"), ("straddle", "<u4")])                                                        # bvh_cull_hit (bvh_cull)
CULL_AUTO, CULL_LANE, CULL_GROUP = 0, 1, 2   # bvh_cull_path
CULL_PATHS = {"auto": CULL_AUTO, "lane": CULL_LANE, "group": CULL_GROUP}
CULL_MAX_PLANES = 8                          # BVH_CULL_MAX_PLANES
CULL_GROUP_STACK = 8192                      # BVH_CULL_GROUP_STACK
SCENE_CULL_HIT = np.dtype([("prim", "<u4"), ("instance", "<u4"), ("straddle", "<u4"), ("zero", "<u4")])                # bvh_scene_cull_hit (bvh_scene_cull)
SCENE_CULL_GROUP_STACK = 8192                # BVH_SCENE_CULL_GROUP_STACK
CAMERA = np.dtype([("eye", "<f4", 4), ("quat", "<f4", 4), ("fov", "<f4"), ("near", "<f4"), ("far", "<f4"), ("pad", "<f4"), ("pad2", "<f4", 4)])
TRANSFORMATION = np.dtype([("translation", "<f4", 3), ("pad", "<f4"), ("scale", "<f4", 3), ("pad1", "<f4"), ("quat", "<f4", 4), ("pad2", "<f4", 4)])
assert RAY.itemsize == 32 and CAMERA.itemsize == 64 and TRANSFORMATION.itemsize == 64 and INSTANCE.itemsize == 64 and INSTANCE_HIT.itemsize == 32
assert POINT_QUERY.itemsize == 16 and POINT_HIT.itemsize == 32 and KNN_HIT.itemsize == 8 and INSTANCE_POINT_HIT.itemsize == 32
assert INSTANCE_KNN_HIT.itemsize == 16


def qt_rotation(axis_angle):
    """qtRotation (src/Common.h:461-472) in float32"""
    ax = np.asarray(axis_angle[:3], dtype=np.float32); ang = np.float32(axis_angle[3])
    ax = ax / np.sqrt(np.float32(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), dtype=np.float32)
    s = np.float32(np.sin(ang / np.float32(2.0), dtype=np.float32)); c = np.float32(np.cos(ang / np.float32(2.0), dtype=np.float32))
    return np.array([ax[0] * s, ax[1] * s, ax[2] * s, c], dtype=np.float32)


def cornell_view():
    """camera + transformation of the reference's traverseBvh (src/TwoPassLbvh.cpp:202-215)"""
    cam = np.zeros(1, dtype=CAMERA); xf = np.zeros(1, dtype=TRANSFORMATION)
    cam["eye"][0] = (0.0, 2.5, 5.8, 0.0); cam["quat"][0] = qt_rotation((0.0, 0.0, 1.0, -1.57))
    cam["fov"][0] = np.float32(45.0) * np.float32(3.14159265358979323846) / np.float32(180.0); cam["near"][0] = 0.0; cam["far"][0] = 100000.0
    xf["translation"][0] = (0.0, 0.0, -5.0); xf["scale"][0] = (1.0, 1.0, 1.0); xf["quat"][0] = (0.0, 0.0, 0.0, 1.0)
    return cam, xf
assert BVH4_NODE.itemsize == 128 and PRIM_NODE.itemsize == 8
assert AABB.itemsize == 24 and BVH2_NODE.itemsize == 32 and PRIMREF.itemsize == 28
INVALID = 0xFFFFFFFF

ALGO_TWOPASS, ALGO_SINGLEPASS, ALGO_PLOCPP, ALGO_HPLOC = 0, 1, 2, 3
ALGO_NAMES = {0: "TwoPassLbvh", 1: "SinglePassLbvh", 2: "PLOCNew", 3: "HPLOC"}

# every symbol include/bvh_mi355x.h declares (tests check that the library exports all of them)
EXPORTS = [
    "bvh_ctx_create", "bvh_ctx_create_on_stream", "bvh_ctx_destroy", "bvh_ctx_reserve", "bvh_ctx_device", "bvh_ctx_stream",
    "bvh_ctx_set_profiling", "bvh_ctx_kernel_times", "bvh_ctx_synchronize", "bvh_ctx_query_overflow", "bvh_build", "bvh_build_ex", "bvh_stage_extents", "bvh_stage_extents_ex",
    "bvh_stage_morton", "bvh_stage_morton64", "bvh_stage_morton_plan", "bvh_sort_pairs", "bvh_sort_pairs64",
    "bvh_emit_lbvh_single", "bvh_emit_lbvh_two", "bvh_emit_ploc", "bvh_emit_hploc", "bvh_to_lbvh_layout", "bvh_collapse4", "bvh_generate_rays", "bvh_trace_while", "bvh_trace", "bvh_sah_cost",
    "bvh_ctx_set_kernel_filter", "bvh_ctx_set_kernel_sampling", "bvh_bvh4_cost", "bvh_checksum", "bvh_ctx_last_collapse_ms", "bvh_batch_create", "bvh_batch_build", "bvh_batch_download", "bvh_batch_destroy",
    "bvh_ctx_set_option", "bvh_ctx_get_option", "bvh_abi_version", "bvh_abi_struct_sizes",
    "bvh_download", "bvh_dev_alloc", "bvh_dev_free", "bvh_dev_upload", "bvh_dev_download", "bvh_dev_copy", "bvh_batched_build", "bvh_version",
    "bvh_refit", "bvh_refit_ex", "bvh_intersect", "bvh_optimize",
    "bvh_build_boxes", "bvh_scene_create", "bvh_scene_destroy", "bvh_scene_build", "bvh_scene_update", "bvh_scene_intersect", "bvh_scene_tlas", "bvh_scene_closest_point", "bvh_scene_intersect_all", "bvh_scene_knn", "bvh_scene_radius_search", "bvh_scene_overlap", "bvh_scene_intersect_tris", "bvh_scene_collide", "bvh_scene_closest_tris", "bvh_scene_radius_tris",
    "bvh_closest_point", "bvh_overlap", "bvh_cull", "bvh_scene_cull", "bvh_knn", "bvh_intersect_all", "bvh_refit_subset", "bvh_radius_search",
    "bvh_winding_prepare", "bvh_winding_number", "bvh_intersect_tris", "bvh_closest_tris", "bvh_radius_tris",
    "bvh_scene_winding_prepare", "bvh_scene_winding_number", "bvh_scene_winding_moments", "bvh_scene_winding_instances",
    "bvh_split_refs", "bvh_remap_leaves", "bvh_build_many", "bvh_many_tree", "bvh_build_many_ploc", "bvh_many_ploc_tree",
]


class BvhError(RuntimeError):
    pass


class Timings(C.Structure):
    _fields_ = [("ms_extents", C.c_float), ("ms_morton", C.c_float), ("ms_sort", C.c_float), ("ms_build", C.c_float),
                ("ms_collapse", C.c_float), ("ms_total", C.c_float), ("ploc_iterations", C.c_uint32), ("sampled", C.c_uint32),
                ("bytes_algorithmic", C.c_uint64)]


class Result(C.Structure):
    _fields_ = [("d_nodes", C.c_void_p), ("d_leaves", C.c_void_p), ("d_prim_aabbs", C.c_void_p), ("d_scene_extent", C.c_void_p),
                ("d_sorted_keys", C.c_void_p), ("d_sorted_vals", C.c_void_p), ("root", C.c_uint32), ("n_internal", C.c_uint32),
                ("n_leaves", C.c_uint32), ("layout", C.c_uint32), ("key_bits", C.c_uint32), ("reserved", C.c_uint32),
                ("d_tris", C.c_void_p), ("d_morton_keys", C.c_void_p)]


class BatchMesh(C.Structure):
    """bvh_batch_mesh: where one mesh's tree lives after bvh_batch_build"""
    _fields_ = [("device", C.c_int32), ("n_leaves", C.c_uint32), ("n_internal", C.c_uint32), ("n_nodes", C.c_uint32), ("root", C.c_uint32), ("layout", C.c_uint32),
                ("d_nodes", C.c_void_p), ("d_leaves", C.c_void_p)]


class BatchReport(C.Structure):
    """bvh_batch_report"""
    _fields_ = [("root_aabbs", C.POINTER(C.c_float)), ("build_ms", C.POINTER(C.c_float)), ("checksums", C.POINTER(C.c_uint64)),
                ("sah", C.POINTER(C.c_double)), ("allgather_us", C.c_float), ("wall_ms", C.c_float),
                ("meshes", C.POINTER(BatchMesh)), ("lanes_per_device", C.c_int32), ("reserved", C.c_int32)]


TRI_PADDED64, TRI_PACKED36, TRI_INDEXED = 0, 1, 2
QUERY_CLOSEST, QUERY_ANY = 0, 1      # bvh_query_kind
_QUERY_IDS = {"closest": QUERY_CLOSEST, "any": QUERY_ANY}
OVERLAP_BOXES, OVERLAP_SELF = 0, 1   # bvh_overlap_mode
TRIS_QUERY, TRIS_SELF = 0, 1         # bvh_tris_mode (bvh_intersect_tris)
HITS_SORTED = 1                      # BVH_HITS_SORTED (bvh_intersect_all's flag)
RADIUS_SORTED = 1                    # BVH_RADIUS_SORTED (bvh_radius_search's and bvh_scene_radius_search's flag)
RADIUS_TRIS_SORTED, RADIUS_TRIS_SELF, RADIUS_TRIS_SKIP_SHARED = 1, 2, 4   # BVH_RADIUS_TRIS_* (bvh_radius_tris's flags)
SCENE_OVERLAP_SORTED = 1             # BVH_SCENE_OVERLAP_SORTED (bvh_scene_overlap's flag)
SCENE_TRIS_QUERY, SCENE_TRIS_INSTANCE = 0, 1   # bvh_scene_tris_mode (bvh_scene_intersect_tris)
SCENE_TRIS_SORTED = 1                # BVH_SCENE_TRIS_SORTED (bvh_scene_intersect_tris's flag)
SCENE_RADIUS_TRIS_SORTED = 1         # BVH_SCENE_RADIUS_TRIS_SORTED (bvh_scene_radius_tris's flag)
SCENE_COLLIDE_SORTED, SCENE_COLLIDE_BOTH = 1, 2   # bvh_scene_collide's flags
SPLIT_MAX_DEPTH = 16                 # BVH_SPLIT_MAX_DEPTH (bvh_split_refs)
ABI_VERSION = 4                      # BVH_ABI_VERSION of include/bvh_mi355x.h this binding was written against
# bvh_option (bvh_ctx_set_option) and the names this harness accepts for the values
OPT_HPLOC_SCHEDULER, OPT_LBVH_SCHEDULER, OPT_SORT_TEST_KNOBS, OPT_PLOC_SCHEDULER = 0, 1, 2, 3
_OPTION_IDS = {"hploc": OPT_HPLOC_SCHEDULER, "lbvh": OPT_LBVH_SCHEDULER, "sort_knobs": OPT_SORT_TEST_KNOBS, "ploc": OPT_PLOC_SCHEDULER}
_OPTION_VALUES = {"auto": 0, "default": 0, None: 0, "async": 1, "single": 1, "iter": 1, "block": 2, "tiles": 2}


class BuildInput(C.Structure):
    """bvh_build_input: device pointers; tri_format TRI_*, morton_bits 30 / 60"""
    _fields_ = [("tri_format", C.c_uint32), ("morton_bits", C.c_uint32), ("d_tris", C.c_void_p), ("d_vertices", C.c_void_p),
                ("d_indices", C.c_void_p), ("n_vertices", C.c_uint32), ("reserved", C.c_uint32)]


class ManyOut(C.Structure):
    """bvh_many_out: the six caller-owned output arrays of bvh_build_many"""
    _fields_ = [("d_nodes", C.c_void_p), ("d_prim_aabbs", C.c_void_p), ("d_scene_extents", C.c_void_p), ("d_roots", C.c_void_p),
                ("d_sorted_keys", C.c_void_p), ("d_sorted_vals", C.c_void_p)]


class ManyPlocOut(C.Structure):
    """bvh_many_ploc_out: the six caller-owned output arrays of bvh_build_many_ploc"""
    _fields_ = [("d_nodes", C.c_void_p), ("d_leaves", C.c_void_p), ("d_prim_aabbs", C.c_void_p), ("d_scene_extents", C.c_void_p),
                ("d_sorted_keys", C.c_void_p), ("d_sorted_vals", C.c_void_p)]


MESH_RANGE = np.dtype([("first", "<u4"), ("count", "<u4")])                                                       # bvh_mesh_range
MANY_LDS_MAX_PRIMS = 512             # BVH_MANY_LDS_MAX_PRIMS: larger meshes of a build_many batch go through the ordinary build


class Blas(C.Structure):
    """bvh_blas: a bottom-level tree + its triangles (tris.tri_format TRI_PADDED64 with d_tris None: tree.d_tris is Triangle[n_leaves])"""
    _fields_ = [("tree", Result), ("tris", BuildInput)]


def build_native(verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into libbvh_mi355x.so (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j8"], capture_output=True, text=True)
    if r.returncode != 0:
        raise BvhError("native build failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout[-2000:])
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    """Load the native library; raises BvhError if it is not built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BvhError(f"{LIB_PATH} is missing — run __graft_entry__.build() (make -C hip-bvh-construction_amd/csrc); there is no CPU fallback")
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise BvhError(f"cannot load {LIB_PATH}: {e}") from e
    vp, u32, i32, u64 = C.c_void_p, C.c_uint32, C.c_int, C.c_uint64
    sig = {
        "bvh_ctx_create": ([i32, C.POINTER(vp)], i32), "bvh_ctx_create_on_stream": ([i32, vp, C.POINTER(vp)], i32),
        "bvh_ctx_destroy": ([vp], None), "bvh_ctx_reserve": ([vp, u32], i32), "bvh_ctx_device": ([vp], i32),
        "bvh_ctx_stream": ([vp], vp), "bvh_ctx_set_profiling": ([vp, i32], i32), "bvh_ctx_synchronize": ([vp], i32),
        "bvh_ctx_query_overflow": ([vp, C.POINTER(u32), C.POINTER(u32)], i32),
        "bvh_build": ([vp, i32, vp, u32, i32, C.POINTER(Result), C.POINTER(Timings)], i32),
        "bvh_build_ex": ([vp, i32, C.POINTER(BuildInput), u32, C.POINTER(Result), C.POINTER(Timings)], i32),
        "bvh_stage_extents_ex": ([vp, C.POINTER(BuildInput), u32, vp, vp], i32),
        "bvh_stage_morton64": ([vp, vp, u32, vp, vp, i32], i32),
        "bvh_stage_morton_plan": ([vp, vp, i32, C.POINTER(C.c_int32)], i32),
        "bvh_sort_pairs64": ([vp, vp, vp, u32, vp, vp, i32, i32], i32),
        "bvh_stage_extents": ([vp, vp, u32, vp, vp], i32), "bvh_stage_morton": ([vp, vp, u32, vp, vp, vp], i32),
        "bvh_sort_pairs": ([vp, vp, vp, u32, vp, vp, i32, i32], i32),
        "bvh_emit_lbvh_single": ([vp, vp, vp, vp, u32, vp, C.POINTER(u32)], i32),
        "bvh_emit_lbvh_two": ([vp, vp, vp, vp, u32, vp], i32),
        "bvh_emit_ploc": ([vp, vp, vp, u32, vp, vp, C.POINTER(u32)], i32),
        "bvh_emit_hploc": ([vp, vp, vp, vp, u32, vp, vp], i32),
        "bvh_to_lbvh_layout": ([vp, C.POINTER(Result), vp], i32), "bvh_sah_cost": ([vp, C.POINTER(Result), C.POINTER(C.c_double)], i32),
        "bvh_download": ([vp, C.POINTER(Result), vp, vp, vp, vp, vp], i32),
        "bvh_dev_alloc": ([vp, u64, C.POINTER(vp)], i32), "bvh_dev_free": ([vp, vp], i32),
        "bvh_dev_upload": ([vp, vp, vp, u64], i32), "bvh_dev_download": ([vp, vp, vp, u64], i32),
        "bvh_dev_copy": ([vp, vp, vp, u64], i32),
        "bvh_batched_build": ([i32, C.POINTER(i32), i32, C.POINTER(vp), C.POINTER(u32), i32, C.POINTER(C.c_float), C.POINTER(C.c_float)], i32),
        "bvh_generate_rays": ([vp, vp, vp, u32, u32], i32),
        "bvh_trace_while": ([vp, vp, vp, vp, u32, u32, vp, vp, u32, u32], i32),
        "bvh_trace": ([vp, i32, vp, vp, vp, u32, u32, vp, vp, vp, u32, u32], i32),
        "bvh_collapse4": ([vp, C.POINTER(Result), vp, vp, C.POINTER(u32)], i32),
        "bvh_ctx_kernel_times": ([vp, C.c_char_p, u32, C.POINTER(C.c_float), C.POINTER(u32), u32], i32),
        "bvh_version": ([], C.c_char_p),
        "bvh_bvh4_cost": ([vp, vp, u32, vp, vp, u32, C.POINTER(C.c_double)], i32),
        "bvh_checksum": ([vp, C.POINTER(Result), C.POINTER(u64)], i32),
        "bvh_ctx_last_collapse_ms": ([vp, C.POINTER(C.c_float)], i32),
        "bvh_ctx_set_kernel_filter": ([vp, C.c_char_p], i32),
        "bvh_ctx_set_kernel_sampling": ([vp, u32], i32),
        "bvh_batch_create": ([i32, C.POINTER(i32), C.POINTER(vp)], i32),
        "bvh_batch_build": ([vp, i32, C.POINTER(vp), C.POINTER(u32), i32, C.POINTER(BatchReport)], i32),
        "bvh_batch_destroy": ([vp], None), "bvh_batch_download": ([vp, C.POINTER(BatchMesh), vp, vp], i32),
        "bvh_ctx_set_option": ([vp, i32, C.c_int64], i32), "bvh_ctx_get_option": ([vp, i32, C.POINTER(C.c_int64)], i32),
        "bvh_abi_version": ([], u32), "bvh_abi_struct_sizes": ([C.POINTER(u32)], None),
        "bvh_refit": ([vp, C.POINTER(Result), vp, i32, C.POINTER(Timings)], i32),
        "bvh_refit_ex": ([vp, C.POINTER(Result), C.POINTER(BuildInput), C.POINTER(Timings)], i32),
        "bvh_refit_subset": ([vp, C.POINTER(Result), C.POINTER(BuildInput), vp, u32, C.POINTER(Timings)], i32),
        "bvh_intersect": ([vp, C.POINTER(Result), C.POINTER(BuildInput), vp, u32, vp, i32], i32),
        "bvh_optimize": ([vp, C.POINTER(Result), u32, C.POINTER(Timings)], i32),
        "bvh_build_boxes": ([vp, i32, vp, u32, i32, C.POINTER(Result), C.POINTER(Timings)], i32),
        "bvh_scene_create": ([vp, C.POINTER(vp)], i32), "bvh_scene_destroy": ([vp], None),
        "bvh_scene_build": ([vp, i32, C.POINTER(Blas), u32, vp, u32, i32, C.POINTER(Timings)], i32),
        "bvh_scene_update": ([vp, vp, i32, C.POINTER(Timings)], i32),
        "bvh_scene_intersect": ([vp, vp, u32, vp, i32], i32),
        "bvh_scene_tlas": ([vp, C.POINTER(Result)], i32),
        "bvh_scene_closest_point": ([vp, vp, u32, vp, i32], i32),
        "bvh_scene_knn": ([vp, vp, u32, u32, vp, vp], i32),
        "bvh_scene_intersect_all": ([vp, vp, u32, u32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_scene_radius_search": ([vp, vp, u32, u32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_scene_overlap": ([vp, vp, u32, u32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_scene_intersect_tris": ([vp, C.POINTER(BuildInput), u32, i32, u32, u32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_scene_closest_tris": ([vp, C.POINTER(BuildInput), u32, i32, u32, C.c_float, vp, i32], i32),
        "bvh_scene_radius_tris": ([vp, C.POINTER(BuildInput), u32, i32, u32, C.c_float, u32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_scene_collide": ([vp, u32, vp, u32, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)], i32),
        "bvh_scene_winding_prepare": ([vp, u32], i32),
        "bvh_scene_winding_number": ([vp, vp, u32, C.c_float, vp], i32),
        "bvh_scene_winding_moments": ([vp, u32, C.POINTER(vp), C.POINTER(u32)], i32),
        "bvh_scene_winding_instances": ([vp, C.POINTER(vp), C.POINTER(vp)], i32),
        "bvh_closest_point": ([vp, C.POINTER(Result), C.POINTER(BuildInput), vp, u32, vp, i32], i32),
        "bvh_knn": ([vp, C.POINTER(Result), C.POINTER(BuildInput), vp, u32, u32, vp, vp], i32),
        "bvh_overlap": ([vp, C.POINTER(Result), vp, u32, i32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_cull": ([vp, C.POINTER(Result), vp, u32, u32, i32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_scene_cull": ([vp, vp, u32, u32, i32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_intersect_tris": ([vp, C.POINTER(Result), C.POINTER(BuildInput), C.POINTER(BuildInput), u32, i32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_closest_tris": ([vp, C.POINTER(Result), C.POINTER(BuildInput), C.POINTER(BuildInput), u32, C.c_float, vp, i32], i32),
        "bvh_intersect_all": ([vp, C.POINTER(Result), C.POINTER(BuildInput), vp, u32, u32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_radius_search": ([vp, C.POINTER(Result), C.POINTER(BuildInput), vp, u32, u32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_radius_tris": ([vp, C.POINTER(Result), C.POINTER(BuildInput), C.POINTER(BuildInput), u32, C.c_float, u32, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_winding_prepare": ([vp, C.POINTER(Result), C.POINTER(BuildInput), vp], i32),
        "bvh_winding_number": ([vp, C.POINTER(Result), C.POINTER(BuildInput), vp, vp, u32, C.c_float, vp], i32),
        "bvh_split_refs": ([vp, C.POINTER(BuildInput), u32, C.c_float, u32, vp, vp, vp, u64, C.POINTER(u64)], i32),
        "bvh_remap_leaves": ([vp, C.POINTER(Result), vp, u32], i32),
        "bvh_build_many": ([vp, i32, C.POINTER(BuildInput), u32, vp, u32, C.POINTER(ManyOut), C.POINTER(Timings)], i32),
        "bvh_many_tree": ([i32, C.POINTER(BuildInput), vp, u32, C.POINTER(ManyOut), u32, vp, C.POINTER(Result), C.POINTER(BuildInput)], i32),
        "bvh_build_many_ploc": ([vp, i32, C.POINTER(BuildInput), u32, vp, u32, C.POINTER(ManyPlocOut), C.POINTER(Timings)], i32),
        "bvh_many_ploc_tree": ([i32, C.POINTER(BuildInput), vp, u32, C.POINTER(ManyPlocOut), u32, C.POINTER(Result), C.POINTER(BuildInput)], i32),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes, f.restype = args, res
    # ABI guard (include/bvh_mi355x.h BVH_ABI_VERSION): a binding written against another revision must not hand the library its structs
    sizes = (u32 * 3)(); L.bvh_abi_struct_sizes(sizes)
    if L.bvh_abi_version() != ABI_VERSION or tuple(sizes) != (C.sizeof(Result), C.sizeof(Timings), C.sizeof(BuildInput)):
        raise BvhError(f"{LIB_PATH}: ABI revision {L.bvh_abi_version()} / struct sizes {tuple(sizes)} do not match this binding "
                       f"({ABI_VERSION}, {(C.sizeof(Result), C.sizeof(Timings), C.sizeof(BuildInput))})")
    _lib = L
    return L


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise BvhError(f"{what} failed with code {rc}" + (" (hipError %d)" % -rc if -1000 < rc < 0 else ""))


def _ptr(a) -> int:
    """Device pointer of a torch tensor / int, or host pointer of a numpy array."""
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()


class DeviceBuffer:
    """A device allocation made through the C ABI (no torch needed)."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        _check(lib().bvh_dev_alloc(ctx.handle, max(self.nbytes, 1), C.byref(p)), "bvh_dev_alloc")
        self.ptr = p.value

    def upload(self, host: np.ndarray) -> "DeviceBuffer":
        host = np.ascontiguousarray(host)
        assert host.nbytes <= self.nbytes
        _check(lib().bvh_dev_upload(self.ctx.handle, self.ptr, host.ctypes.data, host.nbytes), "bvh_dev_upload")
        return self

    def download(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        _check(lib().bvh_dev_download(self.ctx.handle, out.ctypes.data, self.ptr, out.nbytes), "bvh_dev_download")
        return out

    def data_ptr(self) -> int:
        return self.ptr

    def free(self) -> None:
        if self.ptr:
            lib().bvh_dev_free(self.ctx.handle, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _build_input(tri_format, tris, vertices, indices, n_vertices, morton_bits: int = 30) -> BuildInput:
    return BuildInput(tri_format, morton_bits, _ptr(tris) if tris is not None else None, _ptr(vertices) if vertices is not None else None,
                      _ptr(indices) if indices is not None else None, n_vertices, 0)


def _tri_input(tris, vertices, indices, n_vertices, tri_format):
    """the BuildInput of the device triangles a query names, or None where it names none (the call then reads the tree's own d_tris)"""
    if tris is None and vertices is None and indices is None:
        return None
    return _build_input(tri_format, tris, vertices, indices, n_vertices)


def _ref(struct):
    return C.byref(struct) if struct is not None else None


def _device_count(buf, n, itemsize, name, what):
    """the record count of a device query array: given, or a DeviceBuffer's size"""
    if n is None and isinstance(buf, DeviceBuffer):
        n = buf.nbytes // itemsize
    if n is None:
        raise BvhError(f"{name} is required for device {what}")
    return n


def _uploaded(ctx, host):
    """a host query array -> (device buffer or None for no queries, n, the same buffer: the caller frees it after the call)"""
    n = host.shape[0]
    own = ctx.upload(np.ascontiguousarray(host)) if n else None
    return own, n, own


def _as_rays(ctx, rays, n, name="n_rays"):
    """a host RAY array or device rays with their count -> (device pointer or buffer, n, the buffer uploaded for the call or None)"""
    if isinstance(rays, np.ndarray):
        if rays.dtype != RAY:
            raise BvhError("rays must have dtype RAY (32-byte records)")
        return _uploaded(ctx, rays)
    return rays, _device_count(rays, n, RAY.itemsize, name, "rays"), None


def _as_points(ctx, points, radius, n):
    """a host POINT_QUERY array, a host (n, 3) float array whose radius is ``radius`` (None: +inf) or device POINT_QUERY records with their count ->
    (device pointer or buffer, n, the buffer uploaded for the call or None)"""
    if isinstance(points, np.ndarray):
        if points.dtype != POINT_QUERY:
            xyz = np.asarray(points, dtype=np.float32)
            if xyz.ndim != 2 or xyz.shape[1] != 3:
                raise BvhError("points must have dtype POINT_QUERY or shape (n, 3)")
            points = np.zeros(xyz.shape[0], dtype=POINT_QUERY)
            points["point"] = xyz
            points["radius"] = np.float32(np.inf) if radius is None else np.asarray(radius, dtype=np.float32)
        elif radius is not None:
            raise BvhError("radius fills (n, 3) points only: POINT_QUERY records carry their own")
        return _uploaded(ctx, points)
    return points, _device_count(points, n, POINT_QUERY.itemsize, "n_points", "points"), None


def _as_boxes(ctx, boxes, n, name="n", rows_only=True):
    """a host AABB array, host floats ((m, 6) with ``rows_only``, as the builders' overlap takes them; any shape of 6 floats per box without, as Scene.overlap
    does) or device bvh_aabb records with their count -> (device pointer or buffer, n, the buffer uploaded for the call or None)"""
    if isinstance(boxes, np.ndarray):
        if boxes.dtype != AABB:
            f = np.ascontiguousarray(boxes, dtype=np.float32)
            if rows_only:
                if f.ndim != 2 or f.shape[1] != 6:
                    raise BvhError("boxes must have dtype AABB or shape (m, 6)")
            elif f.size % 6 or (f.ndim >= 2 and int(np.prod(f.shape[1:])) != 6):
                raise BvhError("boxes must have dtype AABB or 6 floats per box")
            boxes = f.reshape(-1, 6)
        return _uploaded(ctx, boxes)
    return boxes, _device_count(boxes, n, AABB.itemsize, name, "boxes"), None


def _as_mesh(ctx, other, tri_format, vertices, indices, n, without):
    """the query mesh of an intersect_tris call: a host TRIANGLE array, host floats ((m, 9) or (m, 3, 3), uploaded as TRI_PACKED36), device records in
    ``tri_format`` or a device TRI_INDEXED mesh (``vertices`` / ``indices``), the device ones with their count ``n`` unless a DeviceBuffer's size gives it ->
    (device pointer or buffer, tri_format, n, the buffer uploaded for the call or None).  ``without``: the argument that goes without a mesh, for the message"""
    own = None
    if isinstance(other, np.ndarray):
        if other.dtype == TRIANGLE:
            tri_format = TRI_PADDED64
        else:
            f = np.asarray(other, dtype=np.float32)
            if f.ndim not in (2, 3) or f.size != f.shape[0] * 9:
                raise BvhError("other must have dtype TRIANGLE or shape (m, 9) / (m, 3, 3)")
            other, tri_format = f.reshape(-1, 9), TRI_PACKED36
        other, n, own = _uploaded(ctx, other)
    elif other is None and vertices is None and indices is None:
        raise BvhError(f"another mesh is required (only {without} goes without)")
    elif n is None:
        stride = {TRI_PADDED64: 64, TRI_PACKED36: 36}.get(tri_format)
        n = other.nbytes // stride if isinstance(other, DeviceBuffer) and stride else (indices.nbytes // 12 if isinstance(indices, DeviceBuffer) else None)
        if n is None:
            raise BvhError("n is required for a device mesh")
    return other, tri_format, n, own


def _count_fill(ctx, call, n, rec_dtype, count_only, capacity, what, own=None):
    """The host side of a count -> scan -> fill call over n queries.  ``call(offsets_ptr, records_ptr, capacity, total_ref)`` makes the C call and returns its
    code.  ``count_only`` or no ``capacity``: a count-only call first; then up to two calls with a record buffer, the second with the total the first
    reported when the capacity was too small.  Returns offsets u32[n + 1] (``count_only``) or (offsets, records rec_dtype[total]); frees its buffers and ``own``."""
    offsets, out = ctx.alloc((n + 1) * 4), None
    try:
        total = C.c_uint64()
        if count_only or capacity is None:
            _check(call(offsets.ptr, None, 0, C.byref(total)), what)
            if count_only:
                return offsets.download(np.uint32, n + 1)
            cap = total.value
        else:
            cap = int(capacity)
        for _ in range(2):
            out = ctx.alloc(max(cap, 1) * np.dtype(rec_dtype).itemsize)
            _check(call(offsets.ptr, out.ptr, cap, C.byref(total)), what)
            if total.value <= cap:
                break
            out.free(); out = None
            cap = total.value
        return offsets.download(np.uint32, n + 1), out.download(rec_dtype, total.value)
    finally:
        offsets.free()
        if out is not None:
            out.free()
        if own is not None:
            own.free()


def _no_queries(count_only, rec_dtype):
    """the answer to no queries, given without a call"""
    off = np.zeros(1, dtype=np.uint32)
    return off if count_only else (off, np.zeros(0, dtype=rec_dtype))


def frustum_planes(m, depth_zero_to_one: bool = True) -> np.ndarray:
    """The six Gribb-Hartmann planes of a row-major 4x4 clip matrix in the column-vector convention (clip = m @ [x, y, z, 1]): left, right, bottom, top, near,
    far as an f32 (6, 4) array of (a, b, c, d), not normalised, inside-positive (a x + b y + c z + d >= 0), as bvh_cull takes them.  The depth pair follows
    0 <= z <= w (``depth_zero_to_one``) or -w <= z <= w."""
    m = np.asarray(m, dtype=np.float32).reshape(4, 4)
    r0, r1, r2, r3 = m
    return np.stack([r3 + r0, r3 - r0, r3 + r1, r3 - r1, r2 if depth_zero_to_one else r3 + r2, r3 - r2]).astype(np.float32)


def _box_corners(leaf_boxes):
    """(lo, hi), each f32 (n, 3), of AABB records or an (n, 6) float array (min xyz, max xyz)"""
    b = np.asarray(leaf_boxes)
    if b.dtype == AABB:
        return np.ascontiguousarray(b["min"], dtype=np.float32), np.ascontiguousarray(b["max"], dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 6)
    return b[:, :3], b[:, 3:]


def cull_plane_values(planes, lo, hi):
    """bvh_cull's plane test in numpy f32, every product and every sum a separate np.float32 operation: planes (..., 4) against boxes lo / hi (..., 3), shapes
    broadcast.  A product whose plane coefficient is +-0 contributes +0.0 whatever the coordinate (never 0 * inf = NaN).  Returns (s_p, s_n): s at the p-vertex
    (p.k = hi.k where n.k >= 0, else lo.k) and at the n-vertex (the other choice)."""
    pl = np.asarray(planes, dtype=np.float32); lo = np.asarray(lo, dtype=np.float32); hi = np.asarray(hi, dtype=np.float32)
    d = pl[..., 3]; zero = np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        sel = [pl[..., k] >= zero for k in range(3)]

        def s_of(v):
            x, y, z = (np.where(pl[..., k] == zero, zero, pl[..., k] * v[k]) for k in range(3))
            t = x + y
            t = t + z
            return (t + d).astype(np.float32)
        s_p = s_of([np.where(sel[k], hi[..., k], lo[..., k]) for k in range(3)])
        s_n = s_of([np.where(sel[k], lo[..., k], hi[..., k]) for k in range(3)])
    return s_p, s_n


def cull_brute_force(planes, leaf_boxes):
    """bvh_cull's defined answer by testing every leaf box against every volume (the reference of the CPU and of the GPU tests).  ``planes``: floats
    (n_volumes, planes_per_volume, 4), or (planes_per_volume, 4) for one volume; ``leaf_boxes``: AABB records or (n, 6) floats, indexed by primitive.  A box
    passes a volume iff it is valid (min <= max on every axis, a NaN fails) and s(p-vertex) >= 0 for every plane; bit k of its straddle mask is
    !(s(n-vertex of plane k) >= 0).  Returns (offsets u32[n_volumes + 1], hits CULL_HIT[total]), every slice in ascending prim order."""
    pl = np.asarray(planes, dtype=np.float32)
    if pl.ndim == 2:
        pl = pl[None]
    if pl.ndim != 3 or pl.shape[2] != 4 or not 1 <= pl.shape[1] <= CULL_MAX_PLANES:
        raise BvhError("planes must have shape (n_volumes, 1..8, 4) or (1..8, 4)")
    lo, hi = _box_corners(leaf_boxes)
    with np.errstate(invalid="ignore"):
        valid = (lo <= hi).all(axis=1)
    bits = (np.uint32(1) << np.arange(pl.shape[1], dtype=np.uint32))[:, None]
    counts, rows = np.zeros(len(pl) + 1, dtype=np.uint64), []
    for i, vol in enumerate(pl):
        s_p, s_n = cull_plane_values(vol[:, None, :], lo[None], hi[None])             # (planes, n)
        with np.errstate(invalid="ignore"):
            inside = valid & (s_p >= np.float32(0.0)).all(axis=0)
            mask = np.where(s_n >= np.float32(0.0), np.uint32(0), bits).sum(axis=0, dtype=np.uint32)
        prims = np.nonzero(inside)[0]
        rec = np.zeros(len(prims), dtype=CULL_HIT)
        rec["prim"] = prims; rec["straddle"] = mask[prims]
        rows.append(rec); counts[i + 1] = len(prims)
    offsets = np.minimum(np.cumsum(counts), 0xFFFFFFFF).astype(np.uint32)
    return offsets, (np.concatenate(rows) if rows else np.zeros(0, dtype=CULL_HIT))


def cull(ctx, result, planes, path="auto", count_only: bool = False, capacity: int | None = None):
    """bvh_cull on any tree bvh_overlap accepts (``result``: a builder's result, a bvh_build_boxes tree, Scene.tlas(), caller-filled arrays): which primitives'
    leaf boxes pass each convex volume.  ``planes``: host floats (n_volumes, planes_per_volume, 4) — or (planes_per_volume, 4) for one volume —, each plane
    (a, b, c, d) with its inside a x + b y + c z + d >= 0, 1 to 8 planes per volume (frustum_planes gives a camera's six).  ``path``: "auto", "lane" (one volume
    per lane) or "group" (one volume per workgroup), or a bvh_cull_path value.  Returns host arrays (offsets u32[n_volumes + 1], hits CULL_HIT[total]): volume
    i's records are hits[offsets[i]:offsets[i + 1]], in no particular order; ``straddle == 0`` marks a box wholly inside the volume.  ``count_only`` returns
    offsets alone.  ``capacity`` None: a count-only call first, then a call with the exact capacity; a given capacity that is too small is re-allocated with
    the total the call reported and the call repeated once."""
    pl = np.ascontiguousarray(planes, dtype=np.float32)
    if pl.ndim == 2:
        pl = pl[None]
    if pl.ndim != 3 or pl.shape[2] != 4 or not 1 <= pl.shape[1] <= CULL_MAX_PLANES:
        raise BvhError("planes must have shape (n_volumes, 1..8, 4) or (1..8, 4)")
    if path not in CULL_PATHS and path not in CULL_PATHS.values():
        raise BvhError('path must be "auto", "lane" or "group"')
    mode = CULL_PATHS.get(path, path)
    n, per = pl.shape[0], pl.shape[1]
    if n == 0:                                            # no volumes: the empty answer, without a call
        return _no_queries(count_only, CULL_HIT)
    own = ctx.upload(pl)
    res = C.byref(result)
    return _count_fill(ctx, lambda off, out, cap, tot: lib().bvh_cull(ctx.handle, res, own.ptr, n, per, mode, off, out, cap, tot), n, CULL_HIT, count_only,
                       capacity, "bvh_cull", own)


def _as_volumes(planes):
    """planes as f32 (n_volumes, planes_per_volume, 4); (planes_per_volume, 4) is one volume"""
    pl = np.ascontiguousarray(planes, dtype=np.float32)
    if pl.ndim == 2:
        pl = pl[None]
    if pl.ndim != 3 or pl.shape[2] != 4 or not 1 <= pl.shape[1] <= CULL_MAX_PLANES:
        raise BvhError("planes must have shape (n_volumes, 1..8, 4) or (1..8, 4)")
    return pl


def scene_cull_object_planes(planes, object_to_world):
    """bvh_scene_cull's object planes in numpy f32, every product and every sum a separate np.float32 operation: world planes (..., 4) under the forward
    matrix ``object_to_world`` (..., 12) (row-major 3x4, m_rc = object_to_world[4r + c]), shapes broadcast:
    a' = (a m00 + b m10) + c m20, b' and c' with columns 1 and 2, d' = ((a m03 + b m13) + c m23) + d.  Returns f32 (..., 4)."""
    pl = np.asarray(planes, dtype=np.float32); m = np.asarray(object_to_world, dtype=np.float32)
    a, b, c, d = pl[..., 0], pl[..., 1], pl[..., 2], pl[..., 3]
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for col in range(4):
            x = a * m[..., col]; y = b * m[..., 4 + col]; z = c * m[..., 8 + col]
            t = x + y
            t = t + z
            out.append((t + d) if col == 3 else t)
    return np.stack(np.broadcast_arrays(*out), axis=-1).astype(np.float32)


def scene_cull_brute_force(planes, blas_leaf_boxes, instances, world_boxes):
    """bvh_scene_cull's defined answer by testing every leaf box of every active instance against every volume (the reference of the CPU and of the GPU
    tests).  ``planes``: world-space floats (n_volumes, planes_per_volume, 4), or (planes_per_volume, 4) for one volume; ``blas_leaf_boxes``: per BLAS, AABB
    records or (n, 6) floats indexed by primitive; ``instances``: INSTANCE records, ``blas`` == INVALID (or out of range) marking an inactive one;
    ``world_boxes``: the scene's stored world box of every instance, AABB records or (n_instances, 6) floats.  Pair (k, j) passes volume i iff k is active,
    k's world box passes cull_plane_values' p-vertex test against the world planes, and leaf box j of k's BLAS is valid and passes it against
    scene_cull_object_planes(planes[i], object_to_world[k]); bit p of straddle is !(s'(n-vertex of object plane p) >= 0).  Returns (offsets
    u32[n_volumes + 1], records SCENE_CULL_HIT[total]), every slice in ascending (instance, prim) order."""
    pl = _as_volumes(planes)
    nv, per = pl.shape[0], pl.shape[1]
    wlo, whi = _box_corners(world_boxes)
    inst = np.asarray(instances)
    bits = (np.uint32(1) << np.arange(per, dtype=np.uint32))[None, :, None]
    zero = np.float32(0.0)
    parts = []                                            # (volume, instance, prim, straddle) arrays
    for k in range(len(inst)):
        bl = int(inst["blas"][k])
        if bl >= len(blas_leaf_boxes):
            continue
        with np.errstate(invalid="ignore"):
            s_w, _ = cull_plane_values(pl, wlo[k], whi[k])                               # (volumes, planes)
            enter = bool((wlo[k] <= whi[k]).all()) & (s_w >= zero).all(axis=1)
        vols = np.nonzero(enter)[0]
        if len(vols) == 0:
            continue
        lo, hi = _box_corners(blas_leaf_boxes[bl])
        obj = scene_cull_object_planes(pl[vols], inst["object_to_world"][k])              # (v, planes, 4)
        s_p, s_n = cull_plane_values(obj[:, :, None, :], lo[None, None], hi[None, None])  # (v, planes, n)
        with np.errstate(invalid="ignore"):
            inside = (lo <= hi).all(axis=1)[None] & (s_p >= zero).all(axis=1)
            mask = np.where(s_n >= zero, np.uint32(0), bits).sum(axis=1, dtype=np.uint32)
        vi, pj = np.nonzero(inside)
        parts.append((vols[vi], np.full(len(vi), k, dtype=np.int64), pj, mask[vi, pj]))
    rec = np.zeros(sum(len(p[0]) for p in parts), dtype=SCENE_CULL_HIT)
    offsets = np.zeros(nv + 1, dtype=np.uint64)
    if len(rec):
        v, k, j, msk = (np.concatenate([p[c] for p in parts]) for c in range(4))
        order = np.lexsort((j, k, v))
        rec["prim"], rec["instance"], rec["straddle"] = j[order], k[order], msk[order]
        offsets[1:] = np.cumsum(np.bincount(v, minlength=nv))
    return np.minimum(offsets, 0xFFFFFFFF).astype(np.uint32), rec


def many_layout(counts):
    """bvh_build_many's output layout: (out_off, node_off, total) for the meshes' triangle counts — mesh m's d_prim_aabbs / d_sorted_* slices start at
    out_off[m] (the exclusive scan of the counts), its 2*count-1 node records at record node_off[m] = 2*out_off[m] - m; total = the sum of the counts."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    out_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if len(counts) else np.zeros(0, np.int64)
    node_off = 2 * out_off - np.arange(len(counts), dtype=np.int64)
    return out_off, node_off, int(counts.sum())


def many_ploc_layout(counts):
    """bvh_build_many_ploc's output layout: (out_off, node_off, total) — mesh m's d_leaves / d_prim_aabbs / d_sorted_* slices start at out_off[m] (the exclusive
    scan of the counts), its count-1 node records at record node_off[m] = out_off[m] - m; total = the sum of the counts."""
    out_off, _, total = many_layout(counts)
    return out_off, out_off - np.arange(len(out_off), dtype=np.int64), total


def many_check_ranges(ranges, n_tris: int, tri_format: int = TRI_PADDED64) -> np.ndarray:
    """the host-side part of bvh_build_many's validation: ``ranges`` (rows of (first, count), or a MESH_RANGE array) as a contiguous MESH_RANGE array; BvhError
    for no mesh, a count < 2, first + count > n_tris, a PACKED36 first that is not a multiple of 4, or 2^30 triangles and more in all."""
    if isinstance(ranges, np.ndarray) and ranges.dtype == MESH_RANGE:
        first, count = ranges["first"].astype(np.int64), ranges["count"].astype(np.int64)
    else:
        r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
        first, count = r[:, 0], r[:, 1]
    if len(first) == 0:
        raise BvhError("build_many needs at least one mesh")
    if (first < 0).any() or (first >= 2 ** 32).any() or (count >= 2 ** 32).any():
        raise BvhError("mesh ranges must fit 32 bits")
    if (count < 2).any():
        raise BvhError(f"mesh {int(np.argmax(count < 2))} has fewer than 2 triangles")
    if (first + count > int(n_tris)).any():
        raise BvhError(f"mesh {int(np.argmax(first + count > int(n_tris)))} reaches past the {int(n_tris)} triangles of the input")
    if tri_format == TRI_PACKED36 and (first % 4 != 0).any():
        raise BvhError(f"PACKED36: the first triangle of mesh {int(np.argmax(first % 4 != 0))} is not a multiple of 4 (its records would not be 16-byte aligned)")
    if int(count.sum()) >= 2 ** 30:
        raise BvhError("build_many: 2^30 triangles or more in one batch")
    out = np.empty(len(first), dtype=MESH_RANGE)
    out["first"], out["count"] = first, count
    return out


class ManyTrees:
    """The trees of one Context.build_many call.  Owns the output buffers (and the input it uploaded); they live outside the context's arena, so later builds on
    the context leave them alone and ``blas(m)`` can go straight into a Scene on the same context."""

    def __init__(self, ctx, algo, inp, n_tris, ranges, out, buffers):
        self.ctx, self.algo, self.input, self.n_tris, self.ranges, self.out = ctx, int(algo), inp, int(n_tris), ranges, out
        self._buffers = buffers                           # DeviceBuffers kept alive: outputs, uploaded inputs
        self.n_meshes = len(ranges)
        self.out_off, self.node_off, self.total = many_layout(ranges["count"])
        self.timings = Timings()
        self._roots = None

    def roots(self) -> np.ndarray:
        """u32[n_meshes]: every mesh's root (read back once; two-pass: all 0, no read-back)"""
        if self._roots is None:
            if self.algo == ALGO_TWOPASS:
                self._roots = np.zeros(self.n_meshes, dtype=np.uint32)
            else:
                self._roots = np.empty(self.n_meshes, dtype=np.uint32)
                _check(lib().bvh_dev_download(self.ctx.handle, self._roots.ctypes.data, self.out.d_roots, self._roots.nbytes), "bvh_dev_download")
        return self._roots

    def _slice(self, m: int):
        r, t = Result(), BuildInput()
        roots = self.roots()
        _check(lib().bvh_many_tree(self.algo, C.byref(self.input), self.ranges.ctypes.data, self.n_meshes, C.byref(self.out), int(m), roots.ctypes.data,
                                   C.byref(r), C.byref(t)), "bvh_many_tree")
        return r, t

    def tree(self, m: int) -> Result:
        """bvh_many_tree: mesh m's slice as a Result"""
        return self._slice(m)[0]

    def tris(self, m: int) -> BuildInput:
        """the BuildInput that names mesh m's triangles"""
        return self._slice(m)[1]

    def blas(self, m: int) -> Blas:
        """mesh m as a bottom-level tree for Scene.build (the scene's context must be this one's device; the call orders nothing: synchronize first if the scene
        lives on another context)"""
        r, t = self._slice(m)
        return Blas(r, t)

    def builder(self, m: int) -> "_Builder":
        """mesh m's tree behind the builders' query / refit / download methods (intersect, closest_point, knn, refit_ex ...).  Trees from PACKED36 / INDEXED input
        take their triangles as those methods' tris / vertices / indices arguments (``tris(m)`` names them); reserve the context for the mesh's size first."""
        b = BUILDERS[self.algo]()
        b.result, b._ctx, b._many = self.tree(m), self.ctx, self
        return b._publish()

    def download(self, m: int) -> dict:
        """mesh m's arrays as numpy: dict(nodes, leaves=None, sorted_keys, sorted_vals, scene, prim_aabbs, root, layout)"""
        n, off, noff = int(self.ranges["count"][m]), int(self.out_off[m]), int(self.node_off[m])
        L, h = lib(), self.ctx.handle
        nodes = np.empty(2 * n - 1, dtype=BVH2_NODE); boxes = np.empty(n, dtype=AABB); scene = np.empty(1, dtype=AABB)
        _check(L.bvh_dev_download(h, nodes.ctypes.data, self.out.d_nodes + noff * 32, nodes.nbytes), "bvh_dev_download")
        _check(L.bvh_dev_download(h, boxes.ctypes.data, self.out.d_prim_aabbs + off * 24, boxes.nbytes), "bvh_dev_download")
        _check(L.bvh_dev_download(h, scene.ctypes.data, self.out.d_scene_extents + m * 24, scene.nbytes), "bvh_dev_download")
        keys = vals = None
        if self.out.d_sorted_keys:
            keys = np.empty(n, dtype=np.uint32)
            _check(L.bvh_dev_download(h, keys.ctypes.data, self.out.d_sorted_keys + off * 4, keys.nbytes), "bvh_dev_download")
        if self.out.d_sorted_vals:
            vals = np.empty(n, dtype=np.uint32)
            _check(L.bvh_dev_download(h, vals.ctypes.data, self.out.d_sorted_vals + off * 4, vals.nbytes), "bvh_dev_download")
        return {"nodes": nodes, "leaves": None, "sorted_keys": keys, "sorted_vals": vals, "scene": scene, "prim_aabbs": boxes, "root": int(self.roots()[m]), "layout": 0}

    def download_all(self) -> dict:
        """the six output arrays whole: dict(nodes, prim_aabbs, scenes, roots, sorted_keys, sorted_vals); slice them with out_off / node_off"""
        L, h = lib(), self.ctx.handle

        def get(ptr, dtype, count):
            a = np.empty(count, dtype=dtype)
            _check(L.bvh_dev_download(h, a.ctypes.data, ptr, a.nbytes), "bvh_dev_download")
            return a
        return {"nodes": get(self.out.d_nodes, BVH2_NODE, 2 * self.total - self.n_meshes), "prim_aabbs": get(self.out.d_prim_aabbs, AABB, self.total),
                "scenes": get(self.out.d_scene_extents, AABB, self.n_meshes), "roots": get(self.out.d_roots, np.uint32, self.n_meshes),
                "sorted_keys": get(self.out.d_sorted_keys, np.uint32, self.total) if self.out.d_sorted_keys else None,
                "sorted_vals": get(self.out.d_sorted_vals, np.uint32, self.total) if self.out.d_sorted_vals else None}

    def free(self) -> None:
        for b in self._buffers:
            b.free()
        self._buffers = []


class ManyPlocTrees(ManyTrees):
    """The trees of one Context.build_many_ploc call: ManyTrees' surface over PLOC-layout slices (n-1 nodes + n PrimRef leaves per mesh, every root 0)."""

    def __init__(self, ctx, inp, n_tris, ranges, out, buffers):
        super().__init__(ctx, ALGO_PLOCPP, inp, n_tris, ranges, out, buffers)
        self.out_off, self.node_off, self.total = many_ploc_layout(ranges["count"])

    def roots(self) -> np.ndarray:
        """u32[n_meshes]: all 0 (no read-back)"""
        if self._roots is None:
            self._roots = np.zeros(self.n_meshes, dtype=np.uint32)
        return self._roots

    def _slice(self, m: int):
        r, t = Result(), BuildInput()
        _check(lib().bvh_many_ploc_tree(self.algo, C.byref(self.input), self.ranges.ctypes.data, self.n_meshes, C.byref(self.out), int(m), C.byref(r), C.byref(t)),
               "bvh_many_ploc_tree")
        return r, t

    def _get(self, ptr, dtype, count):
        a = np.empty(count, dtype=dtype)
        _check(lib().bvh_dev_download(self.ctx.handle, a.ctypes.data, ptr, a.nbytes), "bvh_dev_download")
        return a

    def download(self, m: int) -> dict:
        """mesh m's arrays as numpy: dict(nodes, leaves, sorted_keys, sorted_vals, scene, prim_aabbs, root, layout)"""
        n, off, noff = int(self.ranges["count"][m]), int(self.out_off[m]), int(self.node_off[m])
        o = self.out
        return {"nodes": self._get(o.d_nodes + noff * 32, BVH2_NODE, n - 1), "leaves": self._get(o.d_leaves + off * 28, PRIMREF, n),
                "sorted_keys": self._get(o.d_sorted_keys + off * 4, np.uint32, n) if o.d_sorted_keys else None,
                "sorted_vals": self._get(o.d_sorted_vals + off * 4, np.uint32, n) if o.d_sorted_vals else None,
                "scene": self._get(o.d_scene_extents + m * 24, AABB, 1), "prim_aabbs": self._get(o.d_prim_aabbs + off * 24, AABB, n), "root": 0, "layout": 1}

    def download_all(self) -> dict:
        """the six output arrays whole: dict(nodes, leaves, prim_aabbs, scenes, sorted_keys, sorted_vals); slice them with out_off / node_off"""
        o = self.out
        return {"nodes": self._get(o.d_nodes, BVH2_NODE, self.total - self.n_meshes), "leaves": self._get(o.d_leaves, PRIMREF, self.total),
                "prim_aabbs": self._get(o.d_prim_aabbs, AABB, self.total), "scenes": self._get(o.d_scene_extents, AABB, self.n_meshes),
                "sorted_keys": self._get(o.d_sorted_keys, np.uint32, self.total) if o.d_sorted_keys else None,
                "sorted_vals": self._get(o.d_sorted_vals, np.uint32, self.total) if o.d_sorted_vals else None}


def _many_host_input(meshes, tri_format):
    """a list of host TRIANGLE arrays -> (host arrays of the chosen format, ranges, n_tris).  PACKED36 pads every mesh to a multiple of 4 records."""
    for t in meshes:
        if not isinstance(t, np.ndarray) or t.dtype != TRIANGLE:
            raise BvhError("meshes must be host arrays of dtype TRIANGLE (64-byte records)")
    counts = [len(t) for t in meshes]
    if tri_format == TRI_PACKED36:
        firsts, at = [], 0
        for c in counts:
            firsts.append(at); at += (c + 3) // 4 * 4
        n_tris = at
        flat = np.zeros((max(n_tris, 1), 9), dtype=np.float32)
        for f, t in zip(firsts, meshes):
            flat[f:f + len(t)] = np.concatenate([t["v1"], t["v2"], t["v3"]], axis=1)
        return {"tris": flat}, np.array(list(zip(firsts, counts)), dtype=np.int64).reshape(-1, 2), n_tris
    allt = np.concatenate(meshes) if meshes else np.zeros(0, dtype=TRIANGLE)
    firsts = np.concatenate([[0], np.cumsum(counts)[:-1]]) if counts else []
    ranges = np.array(list(zip(firsts, counts)), dtype=np.int64).reshape(-1, 2)
    if tri_format == TRI_INDEXED:
        verts = np.stack([allt["v1"], allt["v2"], allt["v3"]], axis=1).reshape(-1, 3).astype(np.float32)
        return {"vertices": verts, "indices": np.arange(3 * len(allt), dtype=np.uint32)}, ranges, len(allt)
    return {"tris": np.ascontiguousarray(allt)}, ranges, len(allt)


class Context:
    """Mirror of the reference's ``Context`` (src/Context.h:8-18): owns the device binding; here also stream + arena."""

    def __init__(self, device: int = 0, stream: int | None = None):
        h = C.c_void_p()
        if stream:
            _check(lib().bvh_ctx_create_on_stream(device, stream, C.byref(h)), "bvh_ctx_create_on_stream")
        else:
            _check(lib().bvh_ctx_create(device, C.byref(h)), "bvh_ctx_create")
        self.handle = h
        self.device = device
        self._scenes = weakref.WeakSet()                  # bvh_scene objects bound to this ctx: destroyed before it

    @property
    def stream(self) -> int:
        """bvh_ctx_stream: the hipStream_t the context enqueues on (the caller's own, if it was created on one)"""
        return lib().bvh_ctx_stream(self.handle) or 0

    def set_profiling(self, level) -> None:
        """0 off, 1 stage events (reference Timer tokens), 2 + per-kernel events"""
        _check(lib().bvh_ctx_set_profiling(self.handle, int(level)), "bvh_ctx_set_profiling")

    def set_kernel_filter(self, name) -> None:
        """with set_profiling(2): events for this kernel only (None: all kernels)"""
        _check(lib().bvh_ctx_set_kernel_filter(self.handle, name.encode() if name else None), "bvh_ctx_set_kernel_filter")

    def set_kernel_sampling(self, every: int) -> None:
        """with set_profiling(2): per-kernel events for every `every`-th build only"""
        _check(lib().bvh_ctx_set_kernel_sampling(self.handle, int(every)), "bvh_ctx_set_kernel_sampling")

    def kernel_times(self) -> dict:
        """{kernel name: (summed ms, launches)} since set_profiling(2)"""
        names = C.create_string_buffer(4096); ms = (C.c_float * 64)(); cnt = (C.c_uint32 * 64)()
        k = lib().bvh_ctx_kernel_times(self.handle, names, 4096, ms, cnt, 64)
        if k < 0:
            _check(k, "bvh_ctx_kernel_times")
        nm = names.value.decode().split("\n")
        return {nm[i]: (float(ms[i]), int(cnt[i])) for i in range(k)}

    def set_option(self, option, value) -> None:
        """bvh_ctx_set_option: option = OPT_* or "hploc" / "lbvh" / "ploc" / "sort_knobs"; value = int or "auto" / "async" / "single" / "block" ..."""
        opt = _OPTION_IDS[option] if isinstance(option, str) else int(option)
        val = _OPTION_VALUES[value] if (value is None or isinstance(value, str)) else int(value)
        _check(lib().bvh_ctx_set_option(self.handle, opt, val), "bvh_ctx_set_option")

    def get_option(self, option) -> int:
        opt = _OPTION_IDS[option] if isinstance(option, str) else int(option)
        v = C.c_int64()
        _check(lib().bvh_ctx_get_option(self.handle, opt, C.byref(v)), "bvh_ctx_get_option")
        return int(v.value)

    def options(self, **kw):
        """context manager: with ctx.options(hploc="block", lbvh="block"): ...  (restores the previous values)"""
        ctx = self

        class _Scope:
            def __enter__(self_inner):
                self_inner.saved = {k: ctx.get_option(k) for k in kw}
                for k, v in kw.items():
                    ctx.set_option(k, v)
                return ctx

            def __exit__(self_inner, *exc):
                for k, v in self_inner.saved.items():
                    ctx.set_option(k, v)
                return False
        return _Scope()

    def reserve(self, n: int) -> None:
        _check(lib().bvh_ctx_reserve(self.handle, n), "bvh_ctx_reserve")

    def synchronize(self) -> None:
        _check(lib().bvh_ctx_synchronize(self.handle), "bvh_ctx_synchronize")

    def query_overflow(self) -> tuple[int, int]:
        """bvh_ctx_query_overflow: how many queries the stack walks of the last query call's first (count) pass and of its fill pass left to the stackless
        kernels (waits for the stream)"""
        a, b = C.c_uint32(), C.c_uint32()
        _check(lib().bvh_ctx_query_overflow(self.handle, C.byref(a), C.byref(b)), "bvh_ctx_query_overflow")
        return a.value, b.value

    def upload(self, host: np.ndarray) -> DeviceBuffer:
        return DeviceBuffer(self, host.nbytes).upload(host)

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def split_refs(self, tris=None, sa_max: float = 3.4028234663852886e38, max_depth: int = SPLIT_MAX_DEPTH, n: int | None = None, vertices=None, indices=None,
                   n_vertices: int = 0, tri_format: int = TRI_PADDED64, count_only: bool = False, keep_on_device: bool = False):
        """bvh_split_refs: early split clipping.  ``tris`` a host TRIANGLE array (uploaded for the call) or device inputs in ``tri_format`` as for build_ex
        (with ``n``).  Count, allocate, fill.  Returns (offsets u32[n + 1], ref_boxes AABB[total], ref_prims u32[total], total) as host arrays —
        triangle p's references are [offsets[p], offsets[p + 1]) — or, with ``keep_on_device``, the three DeviceBuffers (the caller frees them) and the total.
        ``count_only``: (offsets, None, None, total)."""
        own = None
        if isinstance(tris, np.ndarray):
            if tris.dtype != TRIANGLE:
                raise BvhError("tris must have dtype TRIANGLE (64-byte records)")
            n = tris.shape[0]
            own = tris = self.upload(np.ascontiguousarray(tris))
            tri_format = TRI_PADDED64
        elif n is None:
            raise BvhError("n is required for device inputs")
        inp = _build_input(tri_format, tris, vertices, indices, n_vertices)
        offsets = self.alloc((n + 1) * 4)
        boxes = prims = None
        done = False
        try:
            total = C.c_uint64()
            _check(lib().bvh_split_refs(self.handle, C.byref(inp), n, float(sa_max), int(max_depth), offsets.ptr, None, None, 0, C.byref(total)), "bvh_split_refs")
            if count_only:
                return offsets.download(np.uint32, n + 1), None, None, int(total.value)
            cap = int(total.value)
            boxes = self.alloc(max(cap, 1) * AABB.itemsize); prims = self.alloc(max(cap, 1) * 4)
            _check(lib().bvh_split_refs(self.handle, C.byref(inp), n, float(sa_max), int(max_depth), offsets.ptr, boxes.ptr, prims.ptr, cap, C.byref(total)),
                   "bvh_split_refs")
            if total.value != cap:
                raise BvhError(f"bvh_split_refs: the fill found {total.value} references, the count pass {cap}")
            if keep_on_device:
                done = True
                return offsets, boxes, prims, cap
            return offsets.download(np.uint32, n + 1), boxes.download(AABB, cap), prims.download(np.uint32, cap), cap
        finally:
            if own is not None:
                own.free()                                # (hipFree waits for the kernels that read it)
            if not done:
                for bfr in (offsets, boxes, prims):
                    if bfr is not None:
                        bfr.free()

    def _many_input(self, meshes, tri_format, vertices, indices, n_vertices, n_tris, keep):
        """build_many's / build_many_ploc's input conventions -> (BuildInput, MESH_RANGE array, n_tris); what it uploads is appended to ``keep``"""
        if isinstance(meshes, tuple):
            tris, ranges = meshes
            if isinstance(tris, np.ndarray):
                if tris.dtype != TRIANGLE:
                    raise BvhError("tris must have dtype TRIANGLE (64-byte records)")
                n_tris, tri_format = len(tris), TRI_PADDED64
                tris = self.upload(np.ascontiguousarray(tris)); keep.append(tris)
            elif n_tris is None:
                raise BvhError("n_tris is required for device inputs")
        else:
            host, ranges, n_tris = _many_host_input(list(meshes), tri_format)
            bufs = {k: self.upload(v) for k, v in host.items()}
            keep.extend(bufs.values())
            tris, vertices, indices = bufs.get("tris"), bufs.get("vertices"), bufs.get("indices")
            if tri_format == TRI_INDEXED:
                n_vertices = len(host["vertices"])
        ranges = many_check_ranges(ranges, n_tris, tri_format)
        inp = _build_input(tri_format, tris, vertices, indices, n_vertices)
        return inp, ranges, n_tris

    def build_many(self, meshes, algo: int = ALGO_TWOPASS, tri_format: int = TRI_PADDED64, vertices=None, indices=None, n_vertices: int = 0,
                   n_tris: int | None = None, sorted_arrays: bool = True) -> "ManyTrees":
        """bvh_build_many: the LBVH of every mesh of a batch in one call.  ``meshes``: a list of host TRIANGLE arrays (concatenated, converted to ``tri_format`` and
        uploaded), or a pair (tris, ranges) — ``tris`` one host TRIANGLE array (uploaded as PADDED64) or a device buffer in ``tri_format`` (None for INDEXED, whose
        device ``vertices`` / ``indices`` / ``n_vertices`` are keyword arguments; ``n_tris`` = records / index triples in the buffers), ``ranges`` rows of
        (first, count) or a MESH_RANGE array.  algo ALGO_TWOPASS (every root 0) or ALGO_SINGLEPASS.  Returns a ManyTrees that owns the output buffers."""
        if algo not in (ALGO_TWOPASS, ALGO_SINGLEPASS):
            raise BvhError("build_many builds LBVH trees: algo ALGO_TWOPASS or ALGO_SINGLEPASS (PLOC++ trees: build_many_ploc)")
        keep = []
        try:
            inp, ranges, n_tris = self._many_input(meshes, tri_format, vertices, indices, n_vertices, n_tris, keep)
            _, _, total = many_layout(ranges["count"])
            n = len(ranges)
            outs = [self.alloc((2 * total - n) * 32), self.alloc(total * 24), self.alloc(n * 24), self.alloc(n * 4),
                    self.alloc(total * 4) if sorted_arrays else None, self.alloc(total * 4) if sorted_arrays else None]
            keep.extend(b for b in outs if b is not None)
            out = ManyOut(*[b.ptr if b is not None else None for b in outs])
            mt = ManyTrees(self, algo, inp, n_tris, ranges, out, keep)
            _check(lib().bvh_build_many(self.handle, int(algo), C.byref(inp), n_tris, ranges.ctypes.data, n, C.byref(out), C.byref(mt.timings)), "bvh_build_many")
            keep = []
            return mt
        finally:
            for b in keep:
                b.free()

    def build_many_ploc(self, meshes, tri_format: int = TRI_PADDED64, vertices=None, indices=None, n_vertices: int = 0, n_tris: int | None = None,
                        sorted_arrays: bool = True) -> "ManyPlocTrees":
        """bvh_build_many_ploc: the PLOC++ tree of every mesh of a batch in one call; input conventions as build_many.  Returns a ManyPlocTrees that owns the
        output buffers."""
        keep = []
        try:
            inp, ranges, n_tris = self._many_input(meshes, tri_format, vertices, indices, n_vertices, n_tris, keep)
            _, _, total = many_ploc_layout(ranges["count"])
            n = len(ranges)
            outs = [self.alloc((total - n) * 32), self.alloc(total * 28), self.alloc(total * 24), self.alloc(n * 24),
                    self.alloc(total * 4) if sorted_arrays else None, self.alloc(total * 4) if sorted_arrays else None]
            keep.extend(b for b in outs if b is not None)
            out = ManyPlocOut(*[b.ptr if b is not None else None for b in outs])
            mt = ManyPlocTrees(self, inp, n_tris, ranges, out, keep)
            _check(lib().bvh_build_many_ploc(self.handle, ALGO_PLOCPP, C.byref(inp), n_tris, ranges.ctypes.data, n, C.byref(out), C.byref(mt.timings)),
                   "bvh_build_many_ploc")
            keep = []
            return mt
        finally:
            for b in keep:
                b.free()

    def close(self) -> None:
        if self.handle:
            for sc in list(self._scenes):
                sc.close()
            lib().bvh_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Builder:
    """Common part of the four builders.  After ``build``: ``m_rootNodeIdx``, ``m_nInternalNodes``, ``m_timer`` (dict of
    the reference's TimerCodes tokens -> ms), and device pointers ``d_bvhNodes`` / ``d_leafNodes`` /
    ``d_sortedMortonCodeKeys`` / ``d_sortedMortonCodeValues`` / ``d_triangleAabb`` / ``d_sceneExtents`` as plain ints."""
    ALGO = -1

    def __init__(self):
        self.result = Result()
        self.timings = Timings()
        self.m_rootNodeIdx = 0
        self.m_nInternalNodes = 0
        self.m_cost = 0.0
        self.m_timer = {}
        self._ctx = None
        self._split = None                                # build_split's device arrays: {"tris", "offsets", "ref_boxes", "ref_prims", "n_tris", "total"}
        self._winding = None                              # winding_prepare's (triangle key, moments DeviceBuffer) of the current tree

    def build(self, context: Context, primitives, on_device: bool = False, n: int | None = None) -> "_Builder":
        """``primitives``: numpy array of dtype TRIANGLE (host; copied H2D untimed like the reference) or, with
        ``on_device=True``, anything with ``data_ptr()`` / an int device address plus ``n``."""
        if isinstance(primitives, np.ndarray):
            if primitives.dtype != TRIANGLE:
                raise BvhError("primitives must have dtype TRIANGLE (64-byte records)")
            primitives = np.ascontiguousarray(primitives)
            n = primitives.shape[0]
            on_device = False
        elif n is None:
            raise BvhError("n is required for device inputs")
        self._ctx = context
        self._free_split()                                # (a tree over triangles: no kept references)
        _check(lib().bvh_build(context.handle, self.ALGO, _ptr(primitives), n, int(on_device), C.byref(self.result), C.byref(self.timings)),
               f"{ALGO_NAMES[self.ALGO]}::build")
        return self._publish()

    def build_ex(self, context: Context, n: int, tris=None, vertices=None, indices=None, n_vertices: int = 0, tri_format: int = TRI_PADDED64,
                 morton_bits: int = 30) -> "_Builder":
        """bvh_build_ex: device inputs in any bvh_tri_format, 30- or 60-bit Morton codes."""
        self._ctx = context
        self._free_split()
        inp = _build_input(tri_format, tris, vertices, indices, n_vertices, morton_bits)
        _check(lib().bvh_build_ex(context.handle, self.ALGO, C.byref(inp), n, C.byref(self.result), C.byref(self.timings)), f"{ALGO_NAMES[self.ALGO]}::build_ex")
        return self._publish()

    def build_boxes(self, context: Context, boxes, n: int | None = None, morton_bits: int = 30, _keep_split: bool = False) -> "_Builder":
        """bvh_build_boxes: a tree over caller-supplied boxes — a host AABB array (copied to the device for the call) or a device buffer / int address with
        ``n``.  The result has no triangles (d_tris NULL): intersect / refit need explicit ones."""
        own = None
        if isinstance(boxes, np.ndarray):
            if boxes.dtype != AABB:
                raise BvhError("boxes must have dtype AABB (24-byte records)")
            n = boxes.shape[0]
            own = boxes = context.upload(np.ascontiguousarray(boxes))
        elif n is None:
            raise BvhError("n is required for device boxes")
        self._ctx = context
        if not _keep_split:
            self._free_split()                            # (build_split's arrays belong to the tree it built)
        try:
            _check(lib().bvh_build_boxes(context.handle, self.ALGO, _ptr(boxes), n, int(morton_bits), C.byref(self.result), C.byref(self.timings)),
                   f"{ALGO_NAMES[self.ALGO]}::build_boxes")
        finally:
            if own is not None:
                own.free()                                # (hipFree waits for the build that read it)
        return self._publish()

    def build_split(self, context: Context, primitives, sa_max: float, max_depth: int = SPLIT_MAX_DEPTH, morton_bits: int = 30, relabel: bool = True) -> "_Builder":
        """Early split clipping in front of the build: bvh_split_refs (count, allocate, fill), bvh_build_boxes over the reference boxes and, with ``relabel``,
        bvh_remap_leaves so that the leaves name the original triangles.  ``primitives``: a host TRIANGLE array.  The builder keeps the triangles and the
        reference arrays on the device (``split_arrays()`` downloads them); a later intersect / closest_point on this builder passes the triangles as ``tris``
        by default.  A tree over fewer than 2 references cannot be built (bvh_build_boxes' rule).  Not for refit / refit_subset (include/bvh_mi355x.h)."""
        if not isinstance(primitives, np.ndarray) or primitives.dtype != TRIANGLE:
            raise BvhError("primitives must be a host array of dtype TRIANGLE (64-byte records)")
        self._free_split()
        n = primitives.shape[0]
        d_tris = context.upload(np.ascontiguousarray(primitives))
        try:
            offsets, boxes, prims, total = context.split_refs(tris=d_tris, n=n, sa_max=sa_max, max_depth=max_depth, keep_on_device=True)
        except Exception:
            d_tris.free()
            raise
        self._split = {"tris": d_tris, "offsets": offsets, "ref_boxes": boxes, "ref_prims": prims, "n_tris": n, "total": total}
        self.build_boxes(context, boxes, n=total, morton_bits=morton_bits, _keep_split=True)
        if relabel:
            self.remap_leaves(prims, n_map=total)
        return self

    def remap_leaves(self, map, n_map: int | None = None) -> "_Builder":
        """bvh_remap_leaves: every leaf's primitive index q < n_map becomes map[q].  ``map``: a numpy array (converted to u32 and uploaded for the call) or a
        device buffer of u32 (DeviceBuffer / int address, with ``n_map``)."""
        if self._ctx is None:
            raise BvhError("remap_leaves needs a built tree")
        own = None
        if isinstance(map, np.ndarray):
            host = np.ascontiguousarray(map, dtype=np.uint32).ravel()
            n_map = host.shape[0]
            own = map = self._ctx.upload(host)
        elif n_map is None:
            n_map = map.nbytes // 4 if isinstance(map, DeviceBuffer) else None
            if n_map is None:
                raise BvhError("n_map is required for device maps")
        try:
            self._free_winding()                          # (the leaves name other primitives)
            _check(lib().bvh_remap_leaves(self._ctx.handle, C.byref(self.result), _ptr(map) or None, int(n_map)), f"{ALGO_NAMES[self.ALGO]}::remap_leaves")
        finally:
            if own is not None:
                own.free()                                # (hipFree waits for the kernel that read it)
        return self

    def split_arrays(self):
        """build_split's (offsets u32[n_tris + 1], ref_boxes AABB[total], ref_prims u32[total]) as host arrays"""
        sp = self._split
        if sp is None:
            raise BvhError("split_arrays needs build_split")
        return (sp["offsets"].download(np.uint32, sp["n_tris"] + 1), sp["ref_boxes"].download(AABB, sp["total"]), sp["ref_prims"].download(np.uint32, sp["total"]))

    def _free_split(self) -> None:
        if self._split is not None:
            for k in ("tris", "offsets", "ref_boxes", "ref_prims"):
                self._split[k].free()
            self._split = None

    def refit(self, primitives, on_device: bool = False, n: int | None = None) -> "_Builder":
        """bvh_refit: recompute every box of this builder's tree from new triangle positions (same count, same order), topology kept.
        ``primitives`` as for ``build``; runs on the context of the last build.  download / checksum / sah_cost / collapse4 / render then see the refit tree."""
        if self._ctx is None:
            raise BvhError("refit needs a built tree")
        if isinstance(primitives, np.ndarray):
            if primitives.dtype != TRIANGLE:
                raise BvhError("primitives must have dtype TRIANGLE (64-byte records)")
            primitives = np.ascontiguousarray(primitives)
            n = primitives.shape[0]
            on_device = False
        elif n is None:
            raise BvhError("n is required for device inputs")
        if n != self.result.n_leaves:
            raise BvhError(f"refit with {n} triangles of a tree over {self.result.n_leaves}")
        _check(lib().bvh_refit(self._ctx.handle, C.byref(self.result), _ptr(primitives), int(on_device), C.byref(self.timings)),
               f"{ALGO_NAMES[self.ALGO]}::refit")
        return self._publish()

    def refit_ex(self, n: int | None = None, tris=None, vertices=None, indices=None, n_vertices: int = 0, tri_format: int = TRI_PADDED64) -> "_Builder":
        """bvh_refit_ex: device inputs in any bvh_tri_format (as build_ex; the Morton width is the tree's own)."""
        if self._ctx is None:
            raise BvhError("refit needs a built tree")
        if n is not None and n != self.result.n_leaves:
            raise BvhError(f"refit with {n} triangles of a tree over {self.result.n_leaves}")
        inp = _build_input(tri_format, tris, vertices, indices, n_vertices)
        _check(lib().bvh_refit_ex(self._ctx.handle, C.byref(self.result), C.byref(inp), C.byref(self.timings)), f"{ALGO_NAMES[self.ALGO]}::refit_ex")
        return self._publish()

    def refit_subset(self, prims, n_dirty: int | None = None, tris=None, vertices=None, indices=None, n_vertices: int = 0,
                     tri_format: int = TRI_PADDED64) -> "_Builder":
        """bvh_refit_subset: new boxes for the listed primitives' leaves and the paths from them to the root only.  ``prims``: the primitive indices whose
        triangles changed — a numpy array (converted to u32 and uploaded for the call) or a device buffer of u32 (DeviceBuffer / int address, with ``n_dirty``).
        Triangles: the COMPLETE arrays with the moved triangles updated in place, device inputs in ``tri_format`` as for refit_ex; none given: the tree's own
        d_tris (Triangle[n]).  An upload through the context makes the next call renew the cached parent plan and leaf map: an animation loop keeps its list in
        a DeviceBuffer."""
        if self._ctx is None:
            raise BvhError("refit_subset needs a built tree")
        ctx = self._ctx
        own = None
        if isinstance(prims, np.ndarray):
            host = np.ascontiguousarray(prims, dtype=np.uint32).ravel()
            n_dirty = host.shape[0]
            own = prims = ctx.upload(host)
        elif n_dirty is None:
            n_dirty = prims.nbytes // 4 if isinstance(prims, DeviceBuffer) else None
            if n_dirty is None:
                raise BvhError("n_dirty is required for device lists")
        inp = None
        if tris is not None or vertices is not None or indices is not None or tri_format != TRI_PADDED64:
            inp = C.byref(_build_input(tri_format, tris, vertices, indices, n_vertices))
        try:
            _check(lib().bvh_refit_subset(ctx.handle, C.byref(self.result), inp, _ptr(prims) or None, int(n_dirty), C.byref(self.timings)),
                   f"{ALGO_NAMES[self.ALGO]}::refit_subset")
        finally:
            if own is not None:
                own.free()                                # (hipFree waits for the kernels that read it)
        return self._publish()

    def optimize(self, rounds: int = 3) -> "_Builder":
        """bvh_optimize: lower this builder's tree's SAH in place by treelet restructuring (``rounds`` 1 .. 8), on the context of the last build.
        download / checksum / sah_cost / intersect / refit / collapse4 / render then see the optimised tree."""
        if self._ctx is None:
            raise BvhError("optimize needs a built tree")
        _check(lib().bvh_optimize(self._ctx.handle, C.byref(self.result), int(rounds), C.byref(self.timings)), f"{ALGO_NAMES[self.ALGO]}::optimize")
        return self._publish()

    def intersect(self, rays, query="closest", tris=None, vertices=None, indices=None, n_vertices: int = 0, tri_format: int = TRI_PADDED64,
                  n_rays: int | None = None) -> np.ndarray:
        """bvh_intersect on this builder's tree: ``rays`` a host RAY array or a device buffer (DeviceBuffer / int address, with ``n_rays``); returns a host
        HIT array.  query "closest" / "any" (or QUERY_*).  Triangles: tree's d_tris (Triangle[n]) unless tris / vertices / indices give device inputs in
        ``tri_format`` as for build_ex."""
        if self._ctx is None:
            raise BvhError("intersect needs a built tree")
        ctx = self._ctx
        q = _QUERY_IDS[query] if isinstance(query, str) else int(query)
        rays, n_rays, own = _as_rays(ctx, rays, n_rays)
        tris, tri_format = self._own_tris(tris, vertices, indices, tri_format)
        inp = _tri_input(tris, vertices, indices, n_vertices, tri_format)
        hits = ctx.alloc(max(n_rays, 1) * HIT.itemsize)
        try:
            _check(lib().bvh_intersect(ctx.handle, C.byref(self.result), _ref(inp), _ptr(rays) if rays is not None else None, n_rays, hits.ptr, q),
                   f"{ALGO_NAMES[self.ALGO]}::intersect")
            return hits.download(HIT, n_rays)
        finally:
            hits.free()
            if own is not None:
                own.free()
    def closest_point(self, points, radius=None, query="closest", tris=None, vertices=None, indices=None, n_vertices: int = 0,
                      tri_format: int = TRI_PADDED64, n_points: int | None = None) -> np.ndarray:
        """bvh_closest_point on this builder's tree: ``points`` a host POINT_QUERY array, a host (n, 3) float array whose radius is ``radius`` (None: +inf),
        or a device buffer of POINT_QUERY records (DeviceBuffer / int address, with ``n_points``); returns a host POINT_HIT array.  query "closest" / "any"
        (or QUERY_*).  Triangles as for intersect."""
        if self._ctx is None:
            raise BvhError("closest_point needs a built tree")
        ctx = self._ctx
        q = _QUERY_IDS[query] if isinstance(query, str) else int(query)
        points, n_points, own = _as_points(ctx, points, radius, n_points)
        tris, tri_format = self._own_tris(tris, vertices, indices, tri_format)
        inp = _tri_input(tris, vertices, indices, n_vertices, tri_format)
        hits = ctx.alloc(max(n_points, 1) * POINT_HIT.itemsize)
        try:
            _check(lib().bvh_closest_point(ctx.handle, C.byref(self.result), _ref(inp), _ptr(points) if points is not None else None, n_points, hits.ptr, q),
                   f"{ALGO_NAMES[self.ALGO]}::closest_point")
            return hits.download(POINT_HIT, n_points)
        finally:
            hits.free()
            if own is not None:
                own.free()
    def _own_tris(self, tris, vertices, indices, tri_format):
        """(tris, tri_format) of a call that names no triangles on a build_split tree, which has no d_tris of its own: the triangles the builder kept"""
        if tris is None and vertices is None and indices is None and self._split is not None:
            return self._split["tris"], TRI_PADDED64
        return tris, tri_format

    def _free_winding(self) -> None:
        if self._winding is not None:
            self._winding[1].free()
            self._winding = None

    def _winding_input(self, tris, vertices, indices, n_vertices, tri_format):
        """(key, BuildInput or None) of the triangles a winding call names, as intersect's"""
        tris, tri_format = self._own_tris(tris, vertices, indices, tri_format)
        inp = _tri_input(tris, vertices, indices, n_vertices, tri_format)
        return (None if inp is None else (int(tri_format), _ptr(tris), _ptr(vertices), _ptr(indices), int(n_vertices))), inp
    def winding_prepare(self, tris=None, vertices=None, indices=None, n_vertices: int = 0, tri_format: int = TRI_PADDED64) -> DeviceBuffer:
        """bvh_winding_prepare on this builder's tree: the per-node moments (WINDING_MOMENT[n_leaves - 1]) in a device buffer the builder keeps and returns.
        Triangles as for intersect.  build* / refit* / optimize / remap_leaves free the buffer: the moments of the old tree are stale."""
        if self._ctx is None:
            raise BvhError("winding_prepare needs a built tree")
        key, inp = self._winding_input(tris, vertices, indices, n_vertices, tri_format)
        self._free_winding()
        buf = self._ctx.alloc((self.result.n_leaves - 1) * WINDING_MOMENT.itemsize)
        try:
            _check(lib().bvh_winding_prepare(self._ctx.handle, C.byref(self.result), _ref(inp), buf.ptr),
                   f"{ALGO_NAMES[self.ALGO]}::winding_prepare")
        except Exception:
            buf.free()
            raise
        self._winding = (key, buf)
        return buf

    def winding_number(self, points, beta: float = 2.0, tris=None, vertices=None, indices=None, n_vertices: int = 0, tri_format: int = TRI_PADDED64,
                       n_points: int | None = None) -> np.ndarray:
        """bvh_winding_number on this builder's tree: ``points`` a host (n, 3) float array, a host POINT_QUERY array (the radius is ignored) or a device buffer
        of POINT_QUERY records (DeviceBuffer / int address, with ``n_points``); returns f32[n].  Prepares the moments on first use, and again when other
        triangles are named than the kept moments were made from."""
        if self._ctx is None:
            raise BvhError("winding_number needs a built tree")
        ctx = self._ctx
        key, inp = self._winding_input(tris, vertices, indices, n_vertices, tri_format)
        if self._winding is None or self._winding[0] != key:
            self.winding_prepare(tris, vertices, indices, n_vertices, tri_format)
        points, n_points, own = _as_points(ctx, points, None, n_points)      # (the radius is not read)
        if n_points == 0:
            return np.empty(0, dtype=np.float32)
        w = ctx.alloc(n_points * 4)
        try:
            _check(lib().bvh_winding_number(ctx.handle, C.byref(self.result), _ref(inp), self._winding[1].ptr, _ptr(points), n_points, float(beta), w.ptr),
                   f"{ALGO_NAMES[self.ALGO]}::winding_number")
            return w.download(np.float32, n_points)
        finally:
            w.free()
            if own is not None:
                own.free()
    def signed_distance(self, points, beta: float = 2.0, tris=None, vertices=None, indices=None, n_vertices: int = 0, tri_format: int = TRI_PADDED64):
        """-> (sd f32[n], hits POINT_HIT[n]): closest_point's distance sqrt(dist2) (unbounded radius), negated where winding_number > 0.5 (inside).  ``points``: a
        host (n, 3) float array or POINT_QUERY records (their radius is replaced by +inf).  Plain composition of the two calls."""
        if isinstance(points, np.ndarray) and points.dtype == POINT_QUERY:
            points = np.ascontiguousarray(points["point"])
        xyz = np.asarray(points, dtype=np.float32)
        hits = self.closest_point(xyz, tris=tris, vertices=vertices, indices=indices, n_vertices=n_vertices, tri_format=tri_format)
        w = self.winding_number(xyz, beta=beta, tris=tris, vertices=vertices, indices=indices, n_vertices=n_vertices, tri_format=tri_format)
        with np.errstate(invalid="ignore"):
            d = np.sqrt(hits["dist2"])
            return np.where(w > np.float32(0.5), -d, d).astype(np.float32), hits

    def knn(self, points, k: int, radius=None, tris=None, vertices=None, indices=None, n_vertices: int = 0, tri_format: int = TRI_PADDED64,
            n_points: int | None = None):
        """bvh_knn on this builder's tree: the ``k`` (1 .. KNN_MAX_K) nearest triangles within each query's radius.  ``points`` as for closest_point (a host
        POINT_QUERY array, a host (n, 3) float array whose radius is ``radius`` (None: +inf), or a device buffer of POINT_QUERY records with ``n_points``).
        Returns host arrays (hits KNN_HIT[n, k], counts u32[n]): hits[i, :counts[i]] is query i's list in ascending (dist2, prim) order, the slots past it
        are {radius * radius, INVALID}.  Triangles as for intersect."""
        if self._ctx is None:
            raise BvhError("knn needs a built tree")
        ctx = self._ctx
        k = int(k)
        if not 1 <= k <= KNN_MAX_K:
            raise BvhError(f"k must be 1 .. {KNN_MAX_K}")
        points, n_points, own = _as_points(ctx, points, radius, n_points)
        inp = _tri_input(tris, vertices, indices, n_vertices, tri_format)
        hits = ctx.alloc(max(n_points * k, 1) * KNN_HIT.itemsize)
        counts = ctx.alloc(max(n_points, 1) * 4)
        try:
            _check(lib().bvh_knn(ctx.handle, C.byref(self.result), _ref(inp), _ptr(points) if points is not None else None, n_points, k, hits.ptr, counts.ptr),
                   f"{ALGO_NAMES[self.ALGO]}::knn")
            return hits.download(KNN_HIT, n_points * k).reshape(n_points, k), counts.download(np.uint32, n_points)
        finally:
            hits.free(); counts.free()
            if own is not None:
                own.free()
    def overlap(self, boxes=None, self_pairs: bool = False, capacity: int | None = None, n: int | None = None):
        """bvh_overlap on this builder's tree: which primitives' boxes each query box touches.  ``boxes`` a host AABB array, a host (m, 6) float array
        (min xyz, max xyz), or a device buffer of bvh_aabb records (DeviceBuffer / int address, with ``n``).  ``self_pairs=True`` is BVH_OVERLAP_SELF: ``boxes``
        defaults to the result's own d_prim_aabbs and only primitives above the query's index are reported.  Returns host arrays (offsets u32[m + 1], prims
        u32[total]): query i's primitives are prims[offsets[i]:offsets[i + 1]], in no particular order.  ``capacity`` is the first guess of the total (default
        8 per query); when it is too small the call is repeated with the total it reported."""
        if self._ctx is None:
            raise BvhError("overlap needs a built tree")
        ctx = self._ctx
        own = None
        if boxes is None:
            if not self_pairs or not self.result.d_prim_aabbs:
                raise BvhError("boxes are required (only self_pairs=True defaults them to the tree's own primitive boxes)")
            boxes, n = self.result.d_prim_aabbs, self.result.n_leaves
        else:
            boxes, n, own = _as_boxes(ctx, boxes, n)
        mode = OVERLAP_SELF if self_pairs else OVERLAP_BOXES
        if n == 0 and not self_pairs:                     # no queries: the empty answer, without a call
            return _no_queries(False, np.uint32)
        res = C.byref(self.result)
        return _count_fill(ctx, lambda off, out, cap, tot: lib().bvh_overlap(ctx.handle, res, _ptr(boxes), n, mode, off, out, cap, tot), n, np.uint32, False,
                           max(int(capacity) if capacity is not None else 8 * n, 1), f"{ALGO_NAMES[self.ALGO]}::overlap", own)
    def cull(self, planes, path="auto", count_only: bool = False, capacity: int | None = None):
        """bvh_cull on this builder's tree: which primitives' leaf boxes pass each convex volume of ``planes`` (see the module's cull)."""
        if self._ctx is None:
            raise BvhError("cull needs a built tree")
        return cull(self._ctx, self.result, planes, path, count_only, capacity)
    def intersect_tris(self, other=None, self_pairs: bool = False, capacity: int | None = None, tri_format: int = TRI_PADDED64, vertices=None, indices=None,
                       n_vertices: int = 0, n: int | None = None, tree_tris=None, tree_vertices=None, tree_indices=None, tree_n_vertices: int = 0,
                       tree_tri_format: int = TRI_PADDED64):
        """bvh_intersect_tris on this builder's tree: which of the tree's triangles each triangle of another mesh properly crosses.  ``other`` a host TRIANGLE
        array, a host (m, 9) or (m, 3, 3) float array (uploaded as TRI_PACKED36), or a device buffer of records in ``tri_format`` (DeviceBuffer / int address,
        with ``n``); ``vertices`` / ``indices`` / ``n_vertices`` / ``n`` name a device TRI_INDEXED mesh instead.  ``self_pairs=True`` is BVH_TRIS_SELF: no other
        mesh, the tree's own triangles against each other, every unordered pair once (j > i); refused on a build_split tree, which has more leaves than
        triangles (pass the mesh as ``other`` there).  The tree's triangles are its d_tris unless tree_tris /
        tree_vertices / tree_indices give device inputs in ``tree_tri_format`` as for intersect.  Returns host arrays (offsets u32[m + 1], prims u32[total]):
        query triangle i crosses prims[offsets[i]:offsets[i + 1]], in no particular order.  ``capacity`` is the first guess of the total (default 1 per
        query); when it is too small the call is repeated with the total it reported."""
        if self._ctx is None:
            raise BvhError("intersect_tris needs a built tree")
        ctx = self._ctx
        own = None
        qin = None
        if self_pairs:
            if other is not None or vertices is not None or indices is not None:
                raise BvhError("self_pairs=True takes no other mesh")
            if self._split is not None:
                # (BVH_TRIS_SELF reads triangle i for every i < n_leaves; a build_split tree has more leaves — references — than triangles)
                raise BvhError("self_pairs=True is not available on a build_split tree: it has more leaves than triangles; pass the mesh as `other` instead")
            n = self.result.n_leaves
        else:
            other, tri_format, n, own = _as_mesh(ctx, other, tri_format, vertices, indices, n, "self_pairs=True")
            if n == 0:                                    # no queries: the empty answer, without a call
                return _no_queries(False, np.uint32)
            qin = _build_input(tri_format, other, vertices, indices, n_vertices)
        tree_tris, tree_tri_format = self._own_tris(tree_tris, tree_vertices, tree_indices, tree_tri_format)
        tin = _tri_input(tree_tris, tree_vertices, tree_indices, tree_n_vertices, tree_tri_format)
        mode = TRIS_SELF if self_pairs else TRIS_QUERY
        res = C.byref(self.result)
        return _count_fill(ctx, lambda off, out, cap, tot: lib().bvh_intersect_tris(ctx.handle, res, _ref(tin), _ref(qin), n, mode, off, out, cap, tot), n,
                           np.uint32, False, max(int(capacity) if capacity is not None else n, 1), f"{ALGO_NAMES[self.ALGO]}::intersect_tris", own)
    def closest_tris(self, other, radius=None, query="closest", tri_format: int = TRI_PADDED64, vertices=None, indices=None, n_vertices: int = 0,
                     n: int | None = None, tree_tris=None, tree_vertices=None, tree_indices=None, tree_n_vertices: int = 0,
                     tree_tri_format: int = TRI_PADDED64) -> np.ndarray:
        """bvh_closest_tris on this builder's tree: the nearest tree triangle to each triangle of another mesh within ``radius`` (one bound for the call; None:
        +inf), or with query "any" some tree triangle within it.  ``other`` as intersect_tris takes it: a host TRIANGLE array, a host (m, 9) or (m, 3, 3) float
        array (uploaded as TRI_PACKED36), or a device buffer of records in ``tri_format`` (DeviceBuffer / int address, with ``n``); ``vertices`` / ``indices`` /
        ``n_vertices`` / ``n`` name a device TRI_INDEXED mesh instead.  The tree's triangles as for intersect_tris (tree_*).  Returns a host TRI_HIT array:
        {dist2, prim, feature, 0} per query triangle, a miss {radius * radius, INVALID, 0, 0}."""
        if self._ctx is None:
            raise BvhError("closest_tris needs a built tree")
        ctx = self._ctx
        q = _QUERY_IDS[query] if isinstance(query, str) else int(query)
        other, tri_format, n, own = _as_mesh(ctx, other, tri_format, vertices, indices, n, "no call")
        hits = None
        try:
            if n == 0:                                        # no queries: the empty answer, without a call
                return np.zeros(0, dtype=TRI_HIT)
            qin = _build_input(tri_format, other, vertices, indices, n_vertices)
            tree_tris, tree_tri_format = self._own_tris(tree_tris, tree_vertices, tree_indices, tree_tri_format)
            tin = _tri_input(tree_tris, tree_vertices, tree_indices, tree_n_vertices, tree_tri_format)
            hits = ctx.alloc(n * TRI_HIT.itemsize)
            _check(lib().bvh_closest_tris(ctx.handle, C.byref(self.result), _ref(tin), _ref(qin), n, float("inf") if radius is None else float(radius), hits.ptr, q),
                   f"{ALGO_NAMES[self.ALGO]}::closest_tris")
            return hits.download(TRI_HIT, n)
        finally:
            if hits is not None:
                hits.free()
            if own is not None:
                own.free()
    def radius_tris(self, other=None, radius=None, self_pairs: bool = False, skip_shared: bool = True, sorted: bool = True, count_only: bool = False,
                    capacity: int | None = None, tri_format: int = TRI_PADDED64, vertices=None, indices=None, n_vertices: int = 0, n: int | None = None,
                    tree_tris=None, tree_vertices=None, tree_indices=None, tree_n_vertices: int = 0, tree_tri_format: int = TRI_PADDED64):
        """bvh_radius_tris on this builder's tree: EVERY tree triangle within ``radius`` (one bound for the call; None: +inf) of each triangle of another mesh.
        ``other`` as intersect_tris takes it: a host TRIANGLE array, a host (m, 9) or (m, 3, 3) float array (uploaded as TRI_PACKED36), or a device buffer of
        records in ``tri_format`` (DeviceBuffer / int address, with ``n``); ``vertices`` / ``indices`` / ``n_vertices`` / ``n`` name a device TRI_INDEXED mesh
        instead.  ``self_pairs=True`` is BVH_RADIUS_TRIS_SELF: no other mesh, the tree's own triangles against each other, every unordered pair once (j > i),
        and with ``skip_shared`` (BVH_RADIUS_TRIS_SKIP_SHARED; read only with self_pairs) without the pairs that share a vertex; refused on a build_split tree,
        which has more leaves than triangles (pass the mesh as ``other`` there).  The tree's triangles as for intersect_tris (tree_*).  Returns host arrays
        (offsets u32[m + 1], hits TRI_HIT[total]): query triangle i's partners are hits[offsets[i]:offsets[i + 1]], {dist2, prim, feature, 0} each, in
        ascending (dist2, prim) order when ``sorted`` (BVH_RADIUS_TRIS_SORTED; quadratic in a slice's length), in no particular order otherwise; an empty
        slice is "nothing within the radius".  ``count_only`` returns offsets alone (the partner counts in scanned form).  ``capacity`` None: a count-only
        call first, then a call with the exact capacity; a given capacity that is too small is re-allocated with the total the call reported and the call
        repeated."""
        if self._ctx is None:
            raise BvhError("radius_tris needs a built tree")
        ctx = self._ctx
        own = None
        qin = None
        flags = RADIUS_TRIS_SORTED if sorted else 0
        if self_pairs:
            if other is not None or vertices is not None or indices is not None:
                raise BvhError("self_pairs=True takes no other mesh")
            if self._split is not None:
                # (BVH_RADIUS_TRIS_SELF reads triangle i for every i < n_leaves; a build_split tree has more leaves — references — than triangles)
                raise BvhError("self_pairs=True is not available on a build_split tree: it has more leaves than triangles; pass the mesh as `other` instead")
            n = self.result.n_leaves
            flags |= RADIUS_TRIS_SELF | (RADIUS_TRIS_SKIP_SHARED if skip_shared else 0)
        else:
            other, tri_format, n, own = _as_mesh(ctx, other, tri_format, vertices, indices, n, "self_pairs=True")
            if n == 0:                                    # no queries: the empty answer, without a call
                if own is not None:
                    own.free()
                return _no_queries(count_only, TRI_HIT)
            qin = _build_input(tri_format, other, vertices, indices, n_vertices)
        tree_tris, tree_tri_format = self._own_tris(tree_tris, tree_vertices, tree_indices, tree_tri_format)
        tin = _tri_input(tree_tris, tree_vertices, tree_indices, tree_n_vertices, tree_tri_format)
        r = float("inf") if radius is None else float(radius)
        res = C.byref(self.result)
        return _count_fill(ctx, lambda off, out, cap, tot: lib().bvh_radius_tris(ctx.handle, res, _ref(tin), _ref(qin), n, r, flags, off, out, cap, tot), n,
                           TRI_HIT, count_only, capacity, f"{ALGO_NAMES[self.ALGO]}::radius_tris", own)
    def distance_to(self, other, **mesh):
        """-> (distance, query index, prim index): the distance between this builder's mesh and ``other`` (as closest_tris takes it, with its keyword
        arguments) — sqrt of the smallest dist2 of one unbounded "closest" call, the query triangle that attains it (the lowest index on a tie) and its nearest
        tree triangle; (inf, -1, -1) when nothing was found (no query triangles, or all of them with a NaN)"""
        rec = self.closest_tris(other, radius=None, query="closest", **mesh)
        idx = np.nonzero(rec["prim"] != INVALID)[0]
        if len(idx) == 0:
            return float("inf"), -1, -1
        i = int(idx[np.argmin(rec["dist2"][idx])])              # (a hit's dist2 is never a NaN; argmin keeps the first of equal values)
        return float(np.sqrt(np.float64(rec["dist2"][i]))), i, int(rec["prim"][i])
    def intersect_all(self, rays, sorted: bool = True, count_only: bool = False, capacity: int | None = None, tris=None, vertices=None, indices=None,
                      n_vertices: int = 0, tri_format: int = TRI_PADDED64, n: int | None = None):
        """bvh_intersect_all on this builder's tree: every accepted hit along each ray.  ``rays`` a host RAY array or a device buffer (DeviceBuffer / int
        address, with ``n``).  Returns host arrays (offsets u32[n + 1], hits HIT[total]): ray i's hits are hits[offsets[i]:offsets[i + 1]], in ascending
        (t, prim) order when ``sorted`` (BVH_HITS_SORTED), in no particular order otherwise; an empty slice is a miss.  ``count_only`` returns offsets alone
        (the crossing numbers in scanned form).  ``capacity`` None: a count-only call first, then a call with the exact capacity; a given capacity that is too
        small is re-allocated with the total the call reported and the call repeated.  Triangles as for intersect."""
        if self._ctx is None:
            raise BvhError("intersect_all needs a built tree")
        ctx = self._ctx
        rays, n, own = _as_rays(ctx, rays, n, "n")
        if n == 0:                                        # no rays: the empty answer, without a call
            return _no_queries(count_only, HIT)
        inp = _tri_input(tris, vertices, indices, n_vertices, tri_format)
        res, flags = C.byref(self.result), HITS_SORTED if sorted else 0
        return _count_fill(ctx, lambda off, out, cap, tot: lib().bvh_intersect_all(ctx.handle, res, _ref(inp), _ptr(rays), n, flags, off, out, cap, tot), n,
                           HIT, count_only, capacity, f"{ALGO_NAMES[self.ALGO]}::intersect_all", own)
    def radius_search(self, points, radius=None, sorted: bool = True, count_only: bool = False, capacity: int | None = None, tris=None, vertices=None,
                      indices=None, n_vertices: int = 0, tri_format: int = TRI_PADDED64, n_points: int | None = None):
        """bvh_radius_search on this builder's tree: every triangle within each query's radius.  ``points`` as for closest_point (a host POINT_QUERY array, a
        host (n, 3) float array whose radius is ``radius`` (a scalar or an array of n; None: +inf), or a device buffer of POINT_QUERY records with ``n_points``).
        Returns host arrays (offsets u32[n + 1], hits KNN_HIT[total]): query i's neighbours are hits[offsets[i]:offsets[i + 1]], in ascending (dist2, prim)
        order when ``sorted`` (BVH_RADIUS_SORTED), in no particular order otherwise; an empty slice is "nothing within the radius".  ``count_only`` returns
        offsets alone (the neighbour counts in scanned form).  ``capacity`` None: a count-only call first, then a call with the exact capacity; a given
        capacity that is too small is re-allocated with the total the call reported and the call repeated.  Triangles as for intersect."""
        if self._ctx is None:
            raise BvhError("radius_search needs a built tree")
        ctx = self._ctx
        points, n, own = _as_points(ctx, points, radius, n_points)
        if n == 0:                                        # no queries: the empty answer, without a call
            return _no_queries(count_only, KNN_HIT)
        inp = _tri_input(tris, vertices, indices, n_vertices, tri_format)
        res, flags = C.byref(self.result), RADIUS_SORTED if sorted else 0
        return _count_fill(ctx, lambda off, out, cap, tot: lib().bvh_radius_search(ctx.handle, res, _ref(inp), _ptr(points), n, flags, off, out, cap, tot), n,
                           KNN_HIT, count_only, capacity, f"{ALGO_NAMES[self.ALGO]}::radius_search", own)
    def _publish(self) -> "_Builder":
        self._free_winding()                              # (a build, refit or optimise: the kept winding moments are stale)
        r, t = self.result, self.timings
        self.m_rootNodeIdx, self.m_nInternalNodes = r.root, r.n_internal
        self.d_bvhNodes, self.d_leafNodes = r.d_nodes, r.d_leaves
        self.d_sortedMortonCodeKeys, self.d_sortedMortonCodeValues = r.d_sorted_keys, r.d_sorted_vals
        self.d_triangleAabb, self.d_sceneExtents = r.d_prim_aabbs, r.d_scene_extent
        self.m_timer = {"CalculateCentroidExtentsTime": t.ms_extents, "CalculateMortonCodesTime": t.ms_morton, "SortingTime": t.ms_sort,
                        "BvhBuildTime": t.ms_build, "CollapseBvhTime": t.ms_collapse, "TotalTime": t.ms_total}
        return self

    # ---- read-backs (the reference's d_x.getData()) ------------------------------------------------------------
    def download(self):
        """-> dict(nodes, leaves (or None), sorted_keys, sorted_vals, scene) as numpy arrays."""
        r = self.result
        n = r.n_leaves
        nodes = np.empty(2 * n - 1 if r.layout == 0 else n - 1, dtype=BVH2_NODE)
        leaves = np.empty(n, dtype=PRIMREF) if r.layout == 1 else None
        keys = np.empty(n, dtype=np.uint64 if r.key_bits == 64 else np.uint32); vals = np.empty(n, dtype=np.uint32); scene = np.empty(1, dtype=AABB)
        _check(lib().bvh_download(self._ctx.handle, C.byref(r), nodes.ctypes.data, leaves.ctypes.data if leaves is not None else None,
                                  keys.ctypes.data, vals.ctypes.data, scene.ctypes.data), "bvh_download")
        return {"nodes": nodes, "leaves": leaves, "sorted_keys": keys, "sorted_vals": vals, "scene": scene, "root": r.root, "layout": r.layout}

    def sah_cost(self) -> float:
        c = C.c_double()
        _check(lib().bvh_sah_cost(self._ctx.handle, C.byref(self.result), C.byref(c)), "bvh_sah_cost")
        self.m_cost = c.value
        return c.value

    def collapse4(self):
        """BVH2 -> BVH4 (CollapseToWide4Bvh): returns (Bvh4Node[n_wide], PrimNode[n], n_wide) as numpy arrays"""
        n = self.result.n_leaves
        wide = self._ctx.alloc(n * BVH4_NODE.itemsize); prims = self._ctx.alloc(n * PRIM_NODE.itemsize)
        nw = C.c_uint32()
        _check(lib().bvh_collapse4(self._ctx.handle, C.byref(self.result), wide.ptr, prims.ptr, C.byref(nw)), "bvh_collapse4")
        out = wide.download(BVH4_NODE, nw.value), prims.download(PRIM_NODE, n), int(nw.value)
        wide.free(); prims.free()
        return out

    def checksum(self) -> int:
        """bvh_checksum: order-independent 64-bit checksum of nodes + leaves + root (== checksum_host of the downloaded arrays)"""
        v = C.c_uint64()
        _check(lib().bvh_checksum(self._ctx.handle, C.byref(self.result), C.byref(v)), "bvh_checksum")
        return int(v.value)

    def collapse4_cost(self):
        """the tail of the reference's build(): CollapseToWide4Bvh, then m_cost = Utility::calculatebvh4Cost, both on the device.
        Returns (BVH4 cost, n_wide, collapse ms)."""
        n = self.result.n_leaves
        wide = self._ctx.alloc(n * BVH4_NODE.itemsize); prims = self._ctx.alloc(n * PRIM_NODE.itemsize)
        nw = C.c_uint32(); cost = C.c_double(); ms = C.c_float()
        try:
            _check(lib().bvh_collapse4(self._ctx.handle, C.byref(self.result), wide.ptr, prims.ptr, C.byref(nw)), "bvh_collapse4")
            _check(lib().bvh_bvh4_cost(self._ctx.handle, wide.ptr, nw.value, prims.ptr, self.result.d_prim_aabbs, n, C.byref(cost)), "bvh_bvh4_cost")
            lib().bvh_ctx_last_collapse_ms(self._ctx.handle, C.byref(ms))
        finally:
            wide.free(); prims.free()
        self.m_cost = cost.value
        return cost.value, int(nw.value), float(ms.value)

    def render(self, tris_host: np.ndarray, camera: np.ndarray, transform: np.ndarray, width: int = 512, kind: int = 0, counts: bool = False):
        """traverseBvh's image: GenerateRays + traversal of this tree (through the LBVH-layout adapter for PLOC/HPLOC).  kind: 0 while-while,
        1 restart trail, 2 if-if, 3 speculative while-while.  Returns (rgba uint8[width*width*4], rays RAY[width*width])
        (+ triangle tests per ray if counts)."""
        ctx, n = self._ctx, self.result.n_leaves
        d_tris = ctx.upload(tris_host)
        d_nodes = ctx.alloc((2 * n - 1) * BVH2_NODE.itemsize)
        _check(lib().bvh_to_lbvh_layout(ctx.handle, C.byref(self.result), d_nodes.ptr), "bvh_to_lbvh_layout")
        d_rays = ctx.alloc(width * width * RAY.itemsize); d_rgba = ctx.alloc(width * width * 4)
        cam = np.ascontiguousarray(camera); xf = np.ascontiguousarray(transform)
        _check(lib().bvh_generate_rays(ctx.handle, cam.ctypes.data, d_rays.ptr, width, width), "bvh_generate_rays")
        d_cnt = ctx.alloc(width * width * 4)
        _check(lib().bvh_trace(ctx.handle, kind, d_rays.ptr, d_tris.ptr, d_nodes.ptr, self.result.root, n - 1, xf.ctypes.data, d_rgba.ptr, d_cnt.ptr, width, width), "bvh_trace")
        out = d_rgba.download(np.uint8, width * width * 4), d_rays.download(RAY, width * width)
        if counts:
            out = out + (d_cnt.download(np.uint32, width * width),)
        for bfr in (d_tris, d_nodes, d_rays, d_rgba, d_cnt):
            bfr.free()
        return out

    def to_lbvh_layout(self) -> np.ndarray:
        n = self.result.n_leaves
        buf = self._ctx.alloc((2 * n - 1) * BVH2_NODE.itemsize)
        _check(lib().bvh_to_lbvh_layout(self._ctx.handle, C.byref(self.result), buf.ptr), "bvh_to_lbvh_layout")
        out = buf.download(BVH2_NODE, 2 * n - 1)
        buf.free()
        return out


class TwoPassLbvh(_Builder):
    ALGO = ALGO_TWOPASS


class SinglePassLbvh(_Builder):
    ALGO = ALGO_SINGLEPASS


class PLOCNew(_Builder):
    ALGO = ALGO_PLOCPP


class HPLOC(_Builder):
    ALGO = ALGO_HPLOC


from .batched import BatchedBuildInput, BatchedBvhBuilder, shard  # noqa: E402,F401

def batched_build(meshes, algo: int = ALGO_HPLOC, devices=(0,)):
    """bvh_batched_build: single-process multi-GPU scene shard -> (root_aabbs (M,6) float32, build ms per mesh)"""
    m = len(meshes)
    arrs = [np.ascontiguousarray(t) for t in meshes]
    ptrs = (C.c_void_p * m)(*[a.ctypes.data for a in arrs]); counts = (C.c_uint32 * m)(*[a.shape[0] for a in arrs])
    devs = (C.c_int * len(devices))(*devices)
    roots = np.zeros((m, 6), dtype=np.float32); ms = np.zeros(m, dtype=np.float32)
    _check(lib().bvh_batched_build(len(devices), devs, algo, ptrs, counts, m, roots.ctypes.data_as(C.POINTER(C.c_float)), ms.ctypes.data_as(C.POINTER(C.c_float))), "bvh_batched_build")
    return roots, ms


class Batch:
    """bvh_batch: per-device contexts + RCCL communicator kept across builds (single process, one host thread per device)"""

    def __init__(self, devices=(0,)):
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _check(lib().bvh_batch_create(len(devices), devs, C.byref(h)), "bvh_batch_create")
        self.handle = h

    def build(self, meshes, algo: int = ALGO_HPLOC, checksums: bool = True, sah: bool = False, keep: bool = False) -> dict:
        """keep: every mesh's tree stays on its device (bvh_batch_mesh records under "meshes"; read one back with download(m))"""
        m = len(meshes)
        arrs = [np.ascontiguousarray(t) for t in meshes]
        ptrs = (C.c_void_p * m)(*[a.ctypes.data for a in arrs]); counts = (C.c_uint32 * m)(*[a.shape[0] for a in arrs])
        roots = np.zeros((m, 6), dtype=np.float32); ms = np.zeros(m, dtype=np.float32); ck = np.zeros(m, dtype=np.uint64); sh = np.zeros(m, dtype=np.float64)
        self._meshes = (BatchMesh * m)() if keep else None
        rep = BatchReport(roots.ctypes.data_as(C.POINTER(C.c_float)), ms.ctypes.data_as(C.POINTER(C.c_float)),
                          ck.ctypes.data_as(C.POINTER(C.c_uint64)) if checksums else None, sh.ctypes.data_as(C.POINTER(C.c_double)) if sah else None, 0.0, 0.0,
                          C.cast(self._meshes, C.POINTER(BatchMesh)) if keep else None, 0, 0)
        _check(lib().bvh_batch_build(self.handle, algo, ptrs, counts, m, C.byref(rep)), "bvh_batch_build")
        out = {"root_aabbs": roots, "build_ms": ms, "checksums": ck, "sah": sh, "allgather_us": float(rep.allgather_us), "wall_ms": float(rep.wall_ms),
               "lanes_per_device": int(rep.lanes_per_device)}
        if keep:
            out["meshes"] = [{f: getattr(self._meshes[i], f) for f, _ in BatchMesh._fields_} for i in range(m)]
        return out

    def download(self, m: int):
        """bvh_batch_download of mesh m of the last build(keep=True): (nodes, leaves or None)"""
        bm = self._meshes[m]
        nodes = np.zeros(bm.n_nodes, dtype=BVH2_NODE); leaves = np.zeros(bm.n_leaves, dtype=PRIMREF) if bm.d_leaves else None
        _check(lib().bvh_batch_download(self.handle, C.byref(bm), nodes.ctypes.data, leaves.ctypes.data if leaves is not None else None), "bvh_batch_download")
        return nodes, leaves

    def close(self) -> None:
        if self.handle:
            lib().bvh_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def checksum_host(nodes: np.ndarray, leaves, root: int) -> int:
    """numpy mirror of bvh_checksum (csrc/misc.hip k_checksum)"""
    M = np.uint64(0xff51afd7ed558ccd); G = np.uint64(0x9E3779B97F4A7C15)
    def mix(h, w):
        h = (h ^ w.astype(np.uint64)) * M
        return h ^ (h >> np.uint64(32))
    total = np.uint64(0)
    with np.errstate(over="ignore"):
        for tag, arr, words in ((1, nodes, 8), (2, leaves, 7)):
            if arr is None:
                continue
            w = np.ascontiguousarray(arr).view(np.uint32).reshape(len(arr), words)
            h = G * (np.arange(len(arr), dtype=np.uint64) + np.uint64(1)) + np.uint64(tag)
            for k in range(words):
                h = mix(h, w[:, k])
            total = total + h.sum(dtype=np.uint64)
        total = total + mix(np.array([3], dtype=np.uint64), np.array([root], dtype=np.uint32))[0]
    return int(total)


BUILDERS = {ALGO_TWOPASS: TwoPassLbvh, ALGO_SINGLEPASS: SinglePassLbvh, ALGO_PLOCPP: PLOCNew, ALGO_HPLOC: HPLOC}


def _as_blas(b):
    """a Blas (the caller orders its writes before the scene's reads), a built _Builder (its tree's d_tris as Triangle[n]) or a (built _Builder, BuildInput)
    pair -> (Blas, the builder's Context or None)"""
    if isinstance(b, Blas):
        return b, None
    tris = None
    if isinstance(b, tuple):
        b, tris = b
    if not isinstance(b, _Builder) or b._ctx is None:
        raise BvhError("a BLAS is a Blas, a built builder or (built builder, BuildInput)")
    return Blas(Result.from_buffer_copy(b.result), tris if tris is not None else BuildInput(TRI_PADDED64, 30, None, None, None, 0, 0)), b._ctx


class Scene:
    """bvh_scene: instances of bottom-level trees under a top-level tree, bound to one Context (see include/bvh_mi355x.h for the contract).
    BLASes must not live in this context's arena: build them on other contexts."""

    def __init__(self, ctx: Context):
        h = C.c_void_p()
        _check(lib().bvh_scene_create(ctx.handle, C.byref(h)), "bvh_scene_create")
        self.ctx, self.handle, self.timings, self.n_instances = ctx, h, Timings(), 0
        ctx._scenes.add(self)

    def build(self, algo: int, blas, instances) -> "Scene":
        """blas: list of Blas / built builders / (builder, BuildInput); instances: host INSTANCE array, or (device buffer / address, count)"""
        pairs = [_as_blas(b) for b in blas]
        arr = (Blas * len(pairs))(*[d for d, _ in pairs])
        # the builders' contexts: their builds / refits run on other streams, which nothing orders before the scene's reads (include/bvh_mi355x.h)
        self._blas_ctxs = list({id(c): c for _, c in pairs if c is not None}.values())
        self._sync_blas()
        ptr, n, dev = self._instances(instances)
        _check(lib().bvh_scene_build(self.handle, int(algo), arr, len(pairs), ptr, n, dev, C.byref(self.timings)), "bvh_scene_build")
        self.n_instances = n
        self._winding_ready = False                       # (the build discarded the winding moments)
        self._max_leaves = max((int(d.tree.n_leaves) for d, _ in pairs), default=0)       # (intersect_tris(instance=k): enough rows for any BLAS)
        self._blas_leaves = np.array([int(d.tree.n_leaves) for d, _ in pairs], dtype=np.int64)          # (collide: the rows of a host instance array)
        return self

    def update(self, instances) -> "Scene":
        ptr, n, dev = self._instances(instances)
        if n != self.n_instances:
            raise BvhError(f"update with {n} instances of a scene built with {self.n_instances}")
        self._sync_blas()                                 # (a BLAS refit since the build must be complete: update re-reads the root boxes)
        _check(lib().bvh_scene_update(self.handle, ptr, dev, C.byref(self.timings)), "bvh_scene_update")
        self._winding_ready = False                       # (the instance and top-level moments are stale)
        return self

    def _sync_blas(self) -> None:
        for c in getattr(self, "_blas_ctxs", ()):
            if c.handle:
                c.synchronize()

    def _instances(self, instances):
        if isinstance(instances, np.ndarray):
            if instances.dtype != INSTANCE:
                raise BvhError("instances must have dtype INSTANCE (64-byte records)")
            self._host = np.ascontiguousarray(instances)
            self._host_current = True
            return self._host.ctypes.data, len(self._host), 0
        buf, n = instances
        self._host_current = False                        # (the instance records are the device's: collide cannot count their rows)
        return _ptr(buf), int(n), 1

    def intersect(self, rays, query="closest", n_rays: int | None = None) -> np.ndarray:
        """bvh_scene_intersect: host RAY array or device buffer (+ n_rays) -> host INSTANCE_HIT array"""
        q = _QUERY_IDS[query] if isinstance(query, str) else int(query)
        if n_rays is None and not isinstance(rays, np.ndarray):
            raise BvhError("n_rays is required for device rays")      # (not taken from a DeviceBuffer's size here)
        rays, n_rays, own = _as_rays(self.ctx, rays, n_rays)
        hits = self.ctx.alloc(max(n_rays, 1) * INSTANCE_HIT.itemsize)
        self._sync_blas()
        try:
            _check(lib().bvh_scene_intersect(self.handle, _ptr(rays) if rays is not None else None, n_rays, hits.ptr, q), "bvh_scene_intersect")
            return hits.download(INSTANCE_HIT, n_rays)
        finally:
            hits.free()
            if own is not None:
                own.free()
    def closest_point(self, points, radius=None, query="closest", n_points: int | None = None) -> np.ndarray:
        """bvh_scene_closest_point: ``points`` as for the builders' closest_point (a host POINT_QUERY array, a host (n, 3) float array whose radius is ``radius``
        (None: +inf), or a device buffer of POINT_QUERY records with ``n_points``) -> host INSTANCE_POINT_HIT array, point and dist2 in world space"""
        q = _QUERY_IDS[query] if isinstance(query, str) else int(query)
        points, n_points, own = _as_points(self.ctx, points, radius, n_points)
        hits = self.ctx.alloc(max(n_points, 1) * INSTANCE_POINT_HIT.itemsize)
        self._sync_blas()
        try:
            _check(lib().bvh_scene_closest_point(self.handle, _ptr(points) if points is not None else None, n_points, hits.ptr, q), "bvh_scene_closest_point")
            return hits.download(INSTANCE_POINT_HIT, n_points)
        finally:
            hits.free()
            if own is not None:
                own.free()
    def knn(self, points, k: int, radius=None, n_points: int | None = None):
        """bvh_scene_knn: the ``k`` (1 .. KNN_MAX_K) nearest triangles within each query's radius over all active instances.  ``points`` as for closest_point
        (a host POINT_QUERY array, a host (n, 3) float array whose radius is ``radius`` (None: +inf), or a device buffer of POINT_QUERY records with
        ``n_points``).  Returns host arrays (hits INSTANCE_KNN_HIT[n, k], counts u32[n]): hits[i, :counts[i]] is query i's list in ascending
        (dist2, instance, prim) order, dist2 in world space; the slots past it are {radius * radius, INVALID, INVALID, 0}."""
        k = int(k)
        if not 1 <= k <= KNN_MAX_K:
            raise BvhError(f"k must be 1 .. {KNN_MAX_K}")
        points, n_points, own = _as_points(self.ctx, points, radius, n_points)
        hits = self.ctx.alloc(max(n_points * k, 1) * INSTANCE_KNN_HIT.itemsize)
        counts = self.ctx.alloc(max(n_points, 1) * 4)
        self._sync_blas()
        try:
            _check(lib().bvh_scene_knn(self.handle, _ptr(points) if points is not None else None, n_points, k, hits.ptr, counts.ptr), "bvh_scene_knn")
            return hits.download(INSTANCE_KNN_HIT, n_points * k).reshape(n_points, k), counts.download(np.uint32, n_points)
        finally:
            hits.free(); counts.free()
            if own is not None:
                own.free()
    def intersect_all(self, rays, sorted: bool = True, count_only: bool = False, capacity: int | None = None, n_rays: int | None = None):
        """bvh_scene_intersect_all: every accepted hit along each ray over all active instances.  ``rays`` a host RAY array or a device buffer (DeviceBuffer /
        int address, with ``n_rays``).  Returns host arrays (offsets u32[n + 1], hits INSTANCE_HIT[total]): ray i's hits are hits[offsets[i]:offsets[i + 1]],
        in ascending (t, instance, prim) order when ``sorted`` (BVH_HITS_SORTED), in no particular order otherwise; an empty slice is a miss.  ``count_only``
        returns offsets alone.  ``capacity`` None: a count-only call first, then a call with the exact capacity; a given capacity that is too small is
        re-allocated with the total the call reported and the call repeated once."""
        rays, n, own = _as_rays(self.ctx, rays, n_rays)
        if n == 0:                                        # no rays: the empty answer, without a call
            return _no_queries(count_only, INSTANCE_HIT)
        flags = HITS_SORTED if sorted else 0
        self._sync_blas()
        return _count_fill(self.ctx, lambda off, out, cap, tot: lib().bvh_scene_intersect_all(self.handle, _ptr(rays), n, flags, off, out, cap, tot), n,
                           INSTANCE_HIT, count_only, capacity, "bvh_scene_intersect_all", own)
    def radius_search(self, points, radius=None, sorted: bool = True, count_only: bool = False, capacity: int | None = None, n_points: int | None = None):
        """bvh_scene_radius_search: every triangle of every active instance within each query's radius.  ``points`` as for knn (a host POINT_QUERY array, a
        host (n, 3) float array whose radius is ``radius`` (None: +inf), or a device buffer of POINT_QUERY records with ``n_points``).  Returns host arrays
        (offsets u32[n + 1], hits INSTANCE_KNN_HIT[total]): query i's records are hits[offsets[i]:offsets[i + 1]], in ascending (dist2, instance, prim) order
        when ``sorted`` (BVH_RADIUS_SORTED; quadratic in a slice's length), in no particular order otherwise; an empty slice is "nothing within the radius".
        ``count_only`` returns offsets alone.  ``capacity`` None: a count-only call first, then a call with the exact capacity; a given capacity that is too
        small is re-allocated with the total the call reported and the call repeated once."""
        points, n, own = _as_points(self.ctx, points, radius, n_points)
        if n == 0:                                        # no points: the empty answer, without a call
            return _no_queries(count_only, INSTANCE_KNN_HIT)
        flags = RADIUS_SORTED if sorted else 0
        self._sync_blas()
        return _count_fill(self.ctx, lambda off, out, cap, tot: lib().bvh_scene_radius_search(self.handle, _ptr(points), n, flags, off, out, cap, tot), n,
                           INSTANCE_KNN_HIT, count_only, capacity, "bvh_scene_radius_search", own)
    def overlap(self, boxes, sorted: bool = True, count_only: bool = False, capacity: int | None = None, n_boxes: int | None = None):
        """bvh_scene_overlap: every (instance, triangle) pair whose mapped leaf box touches each world-space query box.  ``boxes`` is a host array of n
        boxes ((n, 6) or (n, 2, 3) floats, or dtype AABB) or a device buffer of bvh_aabb records with ``n_boxes``.  Returns host arrays (offsets u32[n + 1],
        records INSTANCE_PRIM[total]): query i's records are records[offsets[i]:offsets[i + 1]], in ascending (instance, prim) order when ``sorted``
        (BVH_SCENE_OVERLAP_SORTED; quadratic in a slice's length), in no particular order otherwise; an empty slice is "touches nothing".  ``count_only``
        returns offsets alone.  ``capacity`` None: a count-only call first, then a call with the exact capacity; a given capacity that is too small is
        re-allocated with the total the call reported and the call repeated once."""
        boxes, n, own = _as_boxes(self.ctx, boxes, n_boxes, "n_boxes", rows_only=False)
        if n == 0:                                        # no boxes: the empty answer, without a call
            return _no_queries(count_only, INSTANCE_PRIM)
        flags = SCENE_OVERLAP_SORTED if sorted else 0
        self._sync_blas()
        return _count_fill(self.ctx, lambda off, out, cap, tot: lib().bvh_scene_overlap(self.handle, _ptr(boxes), n, flags, off, out, cap, tot), n,
                           INSTANCE_PRIM, count_only, capacity, "bvh_scene_overlap", own)

    def intersect_tris(self, other=None, instance: int | None = None, sorted: bool = True, count_only: bool = False, capacity: int | None = None,
                       tri_format: int = TRI_PADDED64, vertices=None, indices=None, n_vertices: int = 0, n: int | None = None):
        """bvh_scene_intersect_tris: every (instance, triangle) pair whose world triangle each query triangle properly crosses.  Either ``other``, a mesh in
        WORLD space as the builders' intersect_tris takes it — a host TRIANGLE array, a host (m, 9) or (m, 3, 3) float array (uploaded as TRI_PACKED36), or a
        device buffer of records in ``tri_format`` (DeviceBuffer / int address, with ``n``); ``vertices`` / ``indices`` / ``n_vertices`` / ``n`` name a device
        TRI_INDEXED mesh instead — or ``instance=k`` (BVH_SCENE_TRIS_INSTANCE): the rows are the world triangles of instance k's BLAS, instance k itself is
        skipped, and the BLAS is looked up on the device; the answer then has ``n`` rows, those at or beyond the instance's n_leaves empty.  The default
        ``n`` is an UPPER BOUND, not the instance's own count: the largest n_leaves among the BLASes as ``build`` recorded them (the host does not know which
        BLAS a device-resident instance record names), so rows are launched, and offsets returned, for the largest BLAS; pass ``n`` to cut that.  The
        scene copies each BLAS's n_leaves when it is built, so a BLAS rebuilt with another triangle count needs a new ``build`` in any case.  Returns host arrays (offsets u32[n + 1], records INSTANCE_PRIM[total]): query i's records are
        records[offsets[i]:offsets[i + 1]], in ascending (instance, prim) order when ``sorted`` (BVH_SCENE_TRIS_SORTED; quadratic in a slice's length), in no
        particular order otherwise.  ``count_only`` returns offsets alone.  ``capacity`` None: a count-only call first, then a call with the exact capacity;
        a given capacity that is too small is re-allocated with the total the call reported and the call repeated once."""
        own, qin = None, None
        if instance is not None:
            if other is not None or vertices is not None or indices is not None:
                raise BvhError("instance=k takes no other mesh")
            mode, k = SCENE_TRIS_INSTANCE, int(instance)
            if not 0 <= k < self.n_instances:
                raise BvhError(f"instance {k} of a scene of {self.n_instances}")
            n = int(n) if n is not None else getattr(self, "_max_leaves", 0)
        else:
            mode, k = SCENE_TRIS_QUERY, 0
            other, tri_format, n, own = _as_mesh(self.ctx, other, tri_format, vertices, indices, n, "instance=k")
        if n == 0:                                        # no queries: the empty answer, without a call
            return _no_queries(count_only, INSTANCE_PRIM)
        if instance is None:
            qin = _build_input(tri_format, other, vertices, indices, n_vertices)
        flags = SCENE_TRIS_SORTED if sorted else 0
        self._sync_blas()
        return _count_fill(self.ctx, lambda off, out, cap, tot: lib().bvh_scene_intersect_tris(self.handle, _ref(qin), n, mode, k, flags, off, out, cap, tot), n,
                           INSTANCE_PRIM, count_only, capacity, "bvh_scene_intersect_tris", own)

    def closest_tris(self, other=None, instance: int | None = None, radius=None, query="closest", tri_format: int = TRI_PADDED64, vertices=None,
                     indices=None, n_vertices: int = 0, n: int | None = None) -> np.ndarray:
        """bvh_scene_closest_tris: the nearest (instance, triangle) to each query triangle within ``radius`` (one bound for the call; None: +inf), or with
        query "any" some triangle within it.  The query side as for intersect_tris: ``other``, a mesh in WORLD space (a host TRIANGLE array, a host (m, 9) or
        (m, 3, 3) float array, a device buffer of records in ``tri_format`` with ``n``, or ``vertices`` / ``indices`` / ``n_vertices`` / ``n`` for a device
        TRI_INDEXED mesh), or ``instance=k`` (BVH_SCENE_TRIS_INSTANCE): the rows are the world triangles of instance k's BLAS, instance k itself is skipped,
        and the default ``n`` is the same upper bound (the largest n_leaves among the BLASes), rows at or beyond the instance's n_leaves missing.  Returns a
        host INSTANCE_TRI_HIT array: {dist2, prim, feature, instance} per query triangle, dist2 in world space; a miss {radius * radius, INVALID, 0, INVALID}."""
        q = _QUERY_IDS[query] if isinstance(query, str) else int(query)
        own, qin, hits = None, None, None
        if instance is not None:
            if other is not None or vertices is not None or indices is not None:
                raise BvhError("instance=k takes no other mesh")
            mode, k = SCENE_TRIS_INSTANCE, int(instance)
            if not 0 <= k < self.n_instances:
                raise BvhError(f"instance {k} of a scene of {self.n_instances}")
            n = int(n) if n is not None else getattr(self, "_max_leaves", 0)
        else:
            mode, k = SCENE_TRIS_QUERY, 0
            other, tri_format, n, own = _as_mesh(self.ctx, other, tri_format, vertices, indices, n, "instance=k")
        try:
            if n == 0:                                    # no queries: the empty answer, without a call
                return np.zeros(0, dtype=INSTANCE_TRI_HIT)
            if instance is None:
                qin = _build_input(tri_format, other, vertices, indices, n_vertices)
            hits = self.ctx.alloc(n * INSTANCE_TRI_HIT.itemsize)
            self._sync_blas()
            _check(lib().bvh_scene_closest_tris(self.handle, _ref(qin), n, mode, k, float("inf") if radius is None else float(radius), hits.ptr, q),
                   "bvh_scene_closest_tris")
            return hits.download(INSTANCE_TRI_HIT, n)
        finally:
            if hits is not None:
                hits.free()
            if own is not None:
                own.free()

    def radius_tris(self, other=None, instance: int | None = None, radius=None, sorted: bool = True, count_only: bool = False,
                    capacity: int | None = None, tri_format: int = TRI_PADDED64, vertices=None, indices=None, n_vertices: int = 0, n: int | None = None):
        """bvh_scene_radius_tris: EVERY (instance, triangle) within ``radius`` (one bound for the call; None: +inf) of each query triangle, with its squared
        world distance and feature pair.  The query side as for closest_tris: ``other``, a mesh in WORLD space (a host TRIANGLE array, a host (m, 9) or
        (m, 3, 3) float array, a device buffer of records in ``tri_format`` with ``n``, or ``vertices`` / ``indices`` / ``n_vertices`` / ``n`` for a device
        TRI_INDEXED mesh), or ``instance=k`` (BVH_SCENE_TRIS_INSTANCE): the rows are the world triangles of instance k's BLAS, instance k itself is skipped,
        and the default ``n`` is the same upper bound (the largest n_leaves among the BLASes), rows at or beyond the instance's n_leaves empty.  Returns host
        arrays (offsets u32[n + 1], records INSTANCE_TRI_HIT[total]): query i's records {dist2, prim, feature, instance} are
        records[offsets[i]:offsets[i + 1]], in ascending (dist2, instance, prim) order when ``sorted`` (BVH_SCENE_RADIUS_TRIS_SORTED; quadratic in a slice's
        length), in no particular order otherwise.  ``count_only`` returns offsets alone.  ``capacity`` None: a count-only call first, then a call with the
        exact capacity; a given capacity that is too small is re-allocated with the total the call reported and the call repeated once."""
        own, qin = None, None
        if instance is not None:
            if other is not None or vertices is not None or indices is not None:
                raise BvhError("instance=k takes no other mesh")
            mode, k = SCENE_TRIS_INSTANCE, int(instance)
            if not 0 <= k < self.n_instances:
                raise BvhError(f"instance {k} of a scene of {self.n_instances}")
            n = int(n) if n is not None else getattr(self, "_max_leaves", 0)
        else:
            mode, k = SCENE_TRIS_QUERY, 0
            other, tri_format, n, own = _as_mesh(self.ctx, other, tri_format, vertices, indices, n, "instance=k")
        if n == 0:                                        # no queries: the empty answer, without a call
            return _no_queries(count_only, INSTANCE_TRI_HIT)
        if instance is None:
            qin = _build_input(tri_format, other, vertices, indices, n_vertices)
        r = float("inf") if radius is None else float(radius)
        flags = SCENE_RADIUS_TRIS_SORTED if sorted else 0
        self._sync_blas()
        return _count_fill(self.ctx, lambda off, out, cap, tot: lib().bvh_scene_radius_tris(self.handle, _ref(qin), n, mode, k, r, flags, off, out, cap, tot), n,
                           INSTANCE_TRI_HIT, count_only, capacity, "bvh_scene_radius_tris", own)

    def distance_to(self, other=None, instance: int | None = None, **mesh) -> float:
        """The distance between the scene and ``other`` (or, with ``instance=k``, between instance k and every other instance), query side and keyword
        arguments as closest_tris takes them: sqrt of the smallest dist2 of one unbounded "closest" call, inf when nothing answers (no query triangles, all
        of them with a NaN, no other active instance)"""
        rec = self.closest_tris(other, instance=instance, radius=None, query="closest", **mesh)
        hit = rec["prim"] != INVALID
        if not hit.any():
            return float("inf")
        return float(np.sqrt(np.float64(rec["dist2"][hit].min())))      # (a hit's dist2 is never a NaN)

    def collide(self, both: bool = False, sorted: bool = True, count_only: bool = False, capacity: int | None = None, row_capacity: int | None = None):
        """bvh_scene_collide: the crossing triangle pairs of all instances at once.  The rows are the triangles of all active instances in instance order;
        row r with row_first[k] <= r < row_first[k + 1] is triangle r - row_first[k] of instance k, and row_first[n_instances] is the number of rows.  Returns
        host arrays (row_first u32[n_instances + 1], offsets u32[row_capacity + 1], records INSTANCE_PRIM[total]): row r's partners {prim, instance} are
        records[offsets[r]:offsets[r + 1]] — the triangles of HIGHER instances that it properly crosses, so that every unordered pair appears once, or with
        ``both`` those of every other instance — in ascending (instance, prim) order when ``sorted`` (BVH_SCENE_COLLIDE_SORTED; quadratic in a slice's length),
        in no particular order otherwise.  ``count_only`` returns (row_first, offsets).  ``row_capacity`` None: the number of rows, computed from the host
        instance array the scene was last built or updated with; if that array lives on the device, the upper bound n_instances x the largest n_leaves among
        the BLASes.  Either way the call is then made with an upper bound (the host does not decide which instances are active) and the offsets returned are cut
        to the row_first[-1] rows that exist; a given ``row_capacity`` returns all its rows, those behind row_first[-1] empty, and one below the number of rows
        raises BvhError (BVH_E_TOO_LARGE).  ``capacity`` as for intersect_tris."""
        cut = row_capacity is None
        if row_capacity is None:
            host = getattr(self, "_host", None)
            if host is not None and getattr(self, "_host_current", False):
                bl = host["blas"].astype(np.int64)
                ok = (bl >= 0) & (bl < len(self._blas_leaves))
                row_capacity = int(self._blas_leaves[bl[ok]].sum())    # (an upper bound too: an instance may be inactive for its matrix alone)
            else:
                row_capacity = self.n_instances * getattr(self, "_max_leaves", 0)
        rows = int(row_capacity)
        flags = (SCENE_COLLIDE_SORTED if sorted else 0) | (SCENE_COLLIDE_BOTH if both else 0)
        first = self.ctx.alloc((self.n_instances + 1) * 4)
        n_rows = C.c_uint64()
        self._sync_blas()
        try:
            got = _count_fill(self.ctx, lambda off, out, cap, tot: lib().bvh_scene_collide(self.handle, flags, first.ptr, rows, off, out, cap, C.byref(n_rows), tot),
                              rows, INSTANCE_PRIM, count_only, capacity, "bvh_scene_collide")
            row_first = first.download(np.uint32, self.n_instances + 1)
        finally:
            first.free()
        off, recs = (got, None) if count_only else got
        if cut:
            off = off[: int(row_first[-1]) + 1]
        return (row_first, off) if count_only else (row_first, off, recs)

    def winding_prepare(self, keep_blas: bool = False) -> "Scene":
        """bvh_scene_winding_prepare: the BLAS moments (all BLASes in two launches), the per-instance maps and moments and the top-level moments, in memory the
        scene owns.  ``keep_blas`` (BVH_SCENE_WINDING_KEEP_BLAS) skips the BLAS moments when a prepare has succeeded since the last build: the cheap path
        after update() when no BLAS was refit."""
        self._sync_blas()
        _check(lib().bvh_scene_winding_prepare(self.handle, SCENE_WINDING_KEEP_BLAS if keep_blas else 0), "bvh_scene_winding_prepare")
        self._winding_ready = True
        return self

    def winding_moments(self, blas: int | None = None) -> np.ndarray:
        """the prepared WINDING_MOMENT records of BLAS ``blas``, or of the top-level tree (None), downloaded"""
        p, n = C.c_void_p(), C.c_uint32()
        _check(lib().bvh_scene_winding_moments(self.handle, INVALID if blas is None else int(blas), C.byref(p), C.byref(n)), "bvh_scene_winding_moments")
        out = np.empty(n.value, dtype=WINDING_MOMENT)
        if n.value:
            _check(lib().bvh_dev_download(self.ctx.handle, out.ctypes.data, p.value, out.nbytes), "bvh_dev_download")
        return out

    def winding_instances(self):
        """(instance moments WINDING_MOMENT[n_instances], maps WINDING_MAP[n_instances]) as prepared, downloaded"""
        pm, pc = C.c_void_p(), C.c_void_p()
        _check(lib().bvh_scene_winding_instances(self.handle, C.byref(pm), C.byref(pc)), "bvh_scene_winding_instances")
        mom, maps = np.empty(self.n_instances, dtype=WINDING_MOMENT), np.empty(self.n_instances, dtype=WINDING_MAP)
        _check(lib().bvh_dev_download(self.ctx.handle, mom.ctypes.data, pm.value, mom.nbytes), "bvh_dev_download")
        _check(lib().bvh_dev_download(self.ctx.handle, maps.ctypes.data, pc.value, maps.nbytes), "bvh_dev_download")
        return mom, maps

    def winding_number(self, points, beta: float = 2.0, n_points: int | None = None) -> np.ndarray:
        """bvh_scene_winding_number: ``points`` as for the builders' winding_number (a host (n, 3) float array, a host POINT_QUERY array whose radius is ignored,
        or a device buffer of POINT_QUERY records with ``n_points``) -> f32[n], summed over the world triangles of all active instances.  Prepares in full on
        first use and after build() or update(); call winding_prepare(keep_blas=True) after an update() that only moved instances to skip the BLAS moments."""
        if not getattr(self, "_winding_ready", False):
            self.winding_prepare()
        points, n_points, own = _as_points(self.ctx, points, None, n_points)      # (the radius is not read)
        if n_points == 0:
            return np.empty(0, dtype=np.float32)
        w = self.ctx.alloc(n_points * 4)
        self._sync_blas()
        try:
            _check(lib().bvh_scene_winding_number(self.handle, _ptr(points), n_points, float(beta), w.ptr), "bvh_scene_winding_number")
            return w.download(np.float32, n_points)
        finally:
            w.free()
            if own is not None:
                own.free()

    def signed_distance(self, points, beta: float = 2.0):
        """-> (sd f32[n], hits INSTANCE_POINT_HIT[n]): closest_point's world distance sqrt(dist2) (unbounded radius), negated where winding_number > 0.5 (inside
        the assembly).  ``points``: a host (n, 3) float array or POINT_QUERY records (their radius is replaced by +inf).  Plain composition of the two calls."""
        if isinstance(points, np.ndarray) and points.dtype == POINT_QUERY:
            points = np.ascontiguousarray(points["point"])
        xyz = np.asarray(points, dtype=np.float32)
        hits = self.closest_point(xyz)
        w = self.winding_number(xyz, beta=beta)
        with np.errstate(invalid="ignore"):
            d = np.sqrt(hits["dist2"])
            return np.where(w > np.float32(0.5), -d, d).astype(np.float32), hits

    def cull(self, planes, path="auto", count_only: bool = False, capacity: int | None = None):
        """bvh_scene_cull: every (instance, triangle) pair whose leaf box passes each WORLD-space convex volume of ``planes``, the instance judged by its stored
        world box and its leaves by the object planes of the volume under the instance's forward matrix.  ``planes`` and ``path`` as for the module's cull.
        Returns host arrays (offsets u32[n_volumes + 1], records SCENE_CULL_HIT[total]): volume i's records are records[offsets[i]:offsets[i + 1]], in no
        particular order; ``straddle == 0`` marks a leaf box wholly inside the volume.  ``count_only`` returns offsets alone.  ``capacity`` None: a
        count-only call first, then a call with the exact capacity; a given capacity that is too small is re-allocated with the total the call reported
        and the call repeated once."""
        pl = _as_volumes(planes)
        if path not in CULL_PATHS and path not in CULL_PATHS.values():
            raise BvhError('path must be "auto", "lane" or "group"')
        mode = CULL_PATHS.get(path, path)
        n, per = pl.shape[0], pl.shape[1]
        if n == 0:                                        # no volumes: the empty answer, without a call
            return _no_queries(count_only, SCENE_CULL_HIT)
        own = self.ctx.upload(pl)
        self._sync_blas()
        return _count_fill(self.ctx, lambda off, out, cap, tot: lib().bvh_scene_cull(self.handle, own.ptr, n, per, mode, off, out, cap, tot), n,
                           SCENE_CULL_HIT, count_only, capacity, "bvh_scene_cull", own)

    def cull_instances(self, planes, path="auto", count_only: bool = False, capacity: int | None = None):
        """bvh_cull on this scene's top-level tree (tlas()): which instances' world boxes pass each convex volume of ``planes``; the records' ``prim`` is the
        instance index (see the module's cull)."""
        return cull(self.ctx, self.tlas(), planes, path, count_only, capacity)

    def tlas(self) -> Result:
        r = Result()
        _check(lib().bvh_scene_tlas(self.handle, C.byref(r)), "bvh_scene_tlas")
        return r

    def close(self) -> None:
        if self.handle:
            if self.ctx.handle:                           # (a closed ctx has already destroyed its scenes: Context.close)
                lib().bvh_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
