/* bvh_mi355x.h — C ABI of the MI355X-native BVH build path (extent -> Morton -> radix sort -> hierarchy emit).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Each entry point names the
 * reference interface it replaces (paths relative to the reference repo root).  The C++ classes in
 * include/bvh/builders.hpp (same names/signatures as the reference's builders) are thin wrappers over these.
 *
 * Conventions
 *   - every function returns 0 on success, a negative value on failure (-(int)hipError_t, or BVH_E_*);
 *     nothing throws, nothing prints (the reference's CHECK_ORO logs and continues, src/Error.cpp:9-17).
 *   - a bvh_ctx is bound to one device and one HIP stream; calls on one ctx are serialised on its stream;
 *     different ctxs are independent (one ctx per GPU / per host thread for the batched builder).
 *   - "d_" pointers are device pointers on the ctx's device.  Layouts are those of include/bvh/types.h
 *     (= src/Common.h:310-441,574-578 of the reference).
 *   - there is NO CPU fallback: if the HIP runtime or a gfx950 device is missing, bvh_ctx_create fails.
 */
#ifndef BVH_MI355X_H
#define BVH_MI355X_H

#include <stdint.h>
#include "bvh/types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BVH_E_INVALID_ARG   (-10001)
#define BVH_E_TOO_LARGE     (-10002)   /* n >= 2^30 (status words of the one-sweep sort carry 30-bit counts) */
#define BVH_E_NOT_BUILT     (-10003)
#define BVH_E_INTERNAL      (-10004)   /* a device-side consistency check failed (e.g. HPLOC node count != n-1) */

typedef struct bvh_ctx bvh_ctx;

/* Replaces Context::Context() (src/Context.cpp:7-15: device 0 hard coded) — here any device, own stream.  The first context of a process on a device also
 * loads the build path's code objects (~2.6 ms, once), so that no build pays for it: the reference compiles its kernels at this point (hiprtc, seconds). */
int  bvh_ctx_create(int device, bvh_ctx** out);
/* Same, but work is enqueued on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int  bvh_ctx_create_on_stream(int device, void* hip_stream, bvh_ctx** out);
void bvh_ctx_destroy(bvh_ctx* ctx);
/* Pre-size the ctx's device arena for builds of up to n primitives (otherwise grown lazily, outside timed regions). */
int  bvh_ctx_reserve(bvh_ctx* ctx, uint32_t n);
int  bvh_ctx_device(const bvh_ctx* ctx);
void* bvh_ctx_stream(const bvh_ctx* ctx);

/* Per-context options.  The library never reads environment variables: which scheduler a builder uses is decided by the input size unless
 * the host says otherwise here (tests and A/B measurements do).  Unknown option or value: BVH_E_INVALID_ARG, nothing changes. */
typedef enum {
    BVH_OPT_HPLOC_SCHEDULER = 0,   /* 0 auto (by n; default), 1 one asynchronous launch (k_hploc), 2 tile kernel, then the external climb (k_hploc_block / k_hploc_ext).
                                      Same trees.  (3 was the overlapped schedule, removed: still accepted, means 2.) */
    BVH_OPT_LBVH_SCHEDULER  = 1,   /* 0 auto (by n; default), 1 one-launch kernels (k_lbvh_single / k_karras + k_refit), 2 tile scheduler (k_lbvh_block / k_lbvh_ext) */
    BVH_OPT_SORT_TEST_KNOBS = 2,   /* bit mask, default 0; results are identical for every value.  8: tiles are handed out in reverse order; 32: threads help at
                                      the first empty poll (both force the one-sweep sort's helping path, which in-order dispatch never takes) */
    BVH_OPT_PLOC_SCHEDULER  = 3    /* 0 auto (default): one launch per iteration (device-side loop, single-workgroup tail); iterations of at most 256 chunks take chunk =
                                      workgroup id, which assumes that the hardware dispatches a grid's workgroups in id order (it does).  1: chunk tickets in every
                                      iteration — no such assumption; for hosts that share the device between contexts (the batched builder sets it on its lanes).
                                      Same trees.  (2 was a cooperative launch, removed in round 5: still accepted, means 0.) */
} bvh_option;
int  bvh_ctx_set_option(bvh_ctx* ctx, bvh_option option, int64_t value);
int  bvh_ctx_get_option(const bvh_ctx* ctx, bvh_option option, int64_t* value_out);

/* Builder selection = the reference's compile-time switch in src/main.cpp:18-22. */
typedef enum {
    BVH_LBVH_TWOPASS    = 0,   /* TwoPassLbvh::build    src/TwoPassLbvh.cpp:17-197    */
    BVH_LBVH_SINGLEPASS = 1,   /* SinglePassLbvh::build src/SinglePassLbvh.cpp:17-188 */
    BVH_PLOCPP          = 2,   /* PLOCNew::build        src/PLOC++Bvh.cpp:16-196      */
    BVH_HPLOC           = 3    /* HPLOC::build          src/Hploc.cpp:16-165          */
} bvh_algo;

/* Per-stage times, same tokens as the reference's Timer (src/Common.h:418-427, src/Timer.h:31-73).
 * ms_total = extents + morton + sort + build  (the reference's "Total Time", src/TwoPassLbvh.cpp:308-309).
 * Filled only when profiling is enabled on the ctx (bvh_ctx_set_profiling); otherwise all zero. */
typedef struct {
    float    ms_extents, ms_morton, ms_sort, ms_build, ms_collapse, ms_total;
    uint32_t ploc_iterations;          /* PLOC++: NN/merge rounds executed on device */
    uint32_t sampled;                  /* 1: the ms_* fields of this build were recorded; 0: they are zero — profiling is off, or
                                          bvh_ctx_set_kernel_sampling(ctx, k) made this one of the k-1 un-instrumented builds (hosts that
                                          average ms_* over builds must skip those) */
    uint64_t bytes_algorithmic;        /* n x the NOMINAL per-primitive figure of SURVEY.md 8(d) (two-pass 384, single-pass 420, PLOC++ 438, HPLOC 386): mesh
                                          independent.  The exact figure of a PLOC-family build depends on the mesh's cluster loads / stores, which only the
                                          oracle counts (profiles/algorithmic_bytes.json, e.g. 387.98 for the 10 M uniform HPLOC build); bench.py prices its
                                          roofline with the exact figure when that file covers the workload and says which one it used */
} bvh_timings;
/* level 0: no events (bvh_build fully asynchronous where it can be); 1: one event per stage (the reference's Timer tokens);
 * 2: additionally one event pair around every kernel launch, summed by bvh_ctx_kernel_times. */
int  bvh_ctx_set_profiling(bvh_ctx* ctx, int level);
/* Per-kernel HIP-event times accumulated since the last bvh_ctx_set_profiling(ctx, 2): returns the number of distinct
 * kernels k; names_out receives k '\n'-separated names, ms_out[k] summed milliseconds, count_out[k] launch counts. */
/* With profiling level 2, record events for ONE kernel only (its name as reported by bvh_ctx_kernel_times; NULL or "" = all kernels):
 * two events per build instead of one per launch, so that measuring the dominant kernel inside a timed region does not stretch it. */
int  bvh_ctx_set_kernel_filter(bvh_ctx* ctx, const char* kernel_name);
/* Record events (stage events of level 1 AND per-kernel events of level 2) in every `every`-th build only (default 1 = every build).  An event
 * between two launches costs a few microseconds of launch gap and the stage times need a host wait at the end of the build; sampling keeps
 * the measurement inside a timed region without stretching it.  The other builds return bvh_timings with sampled = 0 and all ms_* zero. */
int  bvh_ctx_set_kernel_sampling(bvh_ctx* ctx, uint32_t every);
int  bvh_ctx_kernel_times(bvh_ctx* ctx, char* names_out, uint32_t names_cap, float* ms_out, uint32_t* count_out, uint32_t max_kernels);

/* Result of a build.  All pointers are device pointers owned by the ctx; they stay valid until the next
 * bvh_build on the same ctx or bvh_ctx_destroy.  Mirrors the public members of the reference builders
 * (src/TwoPassLbvh.h:19-31, src/PLOC++Bvh.h:19-32):
 *   LBVH layouts : d_nodes = Bvh2Node[2n-1], internal [0,n-1), leaf i at n-1+i {left=primIdx,right=INVALID}; d_leaves = NULL
 *   PLOC layouts : d_nodes = Bvh2Node[n-1], d_leaves = PrimRef[n] in Morton order, child >= n-1 -> leaves[child-(n-1)], root 0 */
typedef struct {
    void*    d_nodes;
    void*    d_leaves;
    void*    d_prim_aabbs;        /* Aabb[n] by original primitive index (d_triangleAabb) */
    void*    d_scene_extent;      /* Aabb[1] (d_sceneExtents) */
    void*    d_sorted_keys;       /* u32[n] (d_sortedMortonCodeKeys)   */
    void*    d_sorted_vals;       /* u32[n] (d_sortedMortonCodeValues) */
    uint32_t root;                /* BVH2 root index (m_rootNodeIdx; single-pass LBVH: data dependent) */
    uint32_t n_internal;          /* n - 1 (m_nInternalNodes) */
    uint32_t n_leaves;            /* n */
    uint32_t layout;              /* 0 = LBVH layout, 1 = PLOC layout */
    uint32_t key_bits;            /* 32: d_sorted_keys is u32[n] (30-bit codes, the reference); 64: u64[n] (60-bit codes, bvh_build_ex) */
    uint32_t reserved;
    const void* d_tris;           /* the triangles the build read, on the device (d_triangleBuff): the ctx's H2D copy of a host input, or the
                                     caller's own device buffer; format as given to the build (Triangle[n] for bvh_build) */
    void*    d_morton_keys;       /* unsorted Morton codes by primitive index, u32[n] / u64[n] (d_mortonCodeKeys).  d_mortonCodeValues is
                                     not materialised: value i = i (src/CommonBlocksKernel.h:384), produced inside the first sort pass */
} bvh_result;

/* X::build(Context&, std::vector<Triangle>&).  tris: Triangle[n], 64-byte stride, host (tris_on_device = 0: copied H2D
 * into the ctx arena, untimed, as src/TwoPassLbvh.cpp:19-20 does) or device (tris_on_device = 1: used in place). n >= 2. */
int  bvh_build(bvh_ctx* ctx, bvh_algo algo, const void* tris, uint32_t n, int tris_on_device,
               bvh_result* out, bvh_timings* timings /* may be NULL */);

/* ---- extended build (no counterpart in the reference) -----------------------------------
 * Input formats that do not pay for the reference's 64-byte padded Triangle records (stage E reads 36 or ~18 bytes per
 * triangle instead of 64), and 60-bit Morton codes in u64 keys (the same extended-code arithmetic as
 * computeExtendedMortonCode with a 60-bit budget; 8 one-sweep passes; the emitters compare 96-bit {key, position} words).
 * All pointers are DEVICE pointers.  Trees built from the same triangles are identical across input formats. */
typedef enum {
    BVH_TRI_PADDED64 = 0,   /* Triangle[n], 64-byte stride (src/Common.h:429-434) — the reference layout */
    BVH_TRI_PACKED36 = 1,   /* float[9n]: v1 v2 v3 per triangle, 36-byte stride; d_tris 16-byte aligned */
    BVH_TRI_INDEXED  = 2    /* float[3*n_vertices] + uint32[3n] */
} bvh_tri_format;
typedef struct {
    uint32_t    tri_format;      /* bvh_tri_format */
    uint32_t    morton_bits;     /* 30 (reference) or 60 */
    const void* d_tris;          /* PADDED64 / PACKED36 */
    const void* d_vertices;      /* INDEXED */
    const void* d_indices;       /* INDEXED */
    uint32_t    n_vertices;      /* INDEXED (indices >= n_vertices are read as vertex 0, never out of bounds) */
    uint32_t    reserved;
} bvh_build_input;
int  bvh_build_ex(bvh_ctx* ctx, bvh_algo algo, const bvh_build_input* in, uint32_t n, bvh_result* out, bvh_timings* timings /* may be NULL */);
/* Build over caller-supplied boxes instead of triangles (procedural primitives, particles; bvh_scene's top-level tree).  d_boxes: bvh_aabb[n] on the device, read
 * once (it may be the ctx's own d_prim_aabbs).  The pipeline of bvh_build_ex with only stage E replaced: the boxes are copied into the ctx's box array and unioned
 * into the scene extent.  Contract: given the boxes stage E writes for some triangles (a result's d_prim_aabbs), the tree is byte-identical to the one bvh_build_ex
 * builds from those triangles with the same algo and morton_bits (nodes, leaves, root, d_sorted_keys, d_sorted_vals), for every builder and scheduler option.
 * In the result d_tris is NULL: bvh_intersect / bvh_refit of it need an explicit `tris`.  Errors: those of bvh_build_ex (morton_bits 30 or 60), NULL d_boxes. */
int  bvh_build_boxes(bvh_ctx* ctx, bvh_algo algo, const void* d_boxes /* bvh_aabb[n], device */, uint32_t n, int morton_bits /* 30 or 60 */,
                     bvh_result* out, bvh_timings* timings /* may be NULL */);
/* stage E on any input format */
int  bvh_stage_extents_ex(bvh_ctx* ctx, const bvh_build_input* in, uint32_t n, void* d_prim_aabbs, void* d_scene_extent);
/* stage M with a total_bits budget (3..60) into u64 keys; total_bits = 30 reproduces bvh_stage_morton's codes.  The codes keep the reference's
 * interleave (X * 4 + Y * 2 + Z) at every budget: one that does not split evenly over the axes (not a multiple of 3 in 3-D, odd in 2-D) sets up to
 * two bits above total_bits, and degenerate extents wrap as in the reference, so sort the keys on [0, 64) as the builds do. */
int  bvh_stage_morton64(bvh_ctx* ctx, const void* d_prim_aabbs, uint32_t n, const void* d_scene_extent, uint64_t* d_keys, int total_bits);
/* The per-scene bit plan of stage M exactly as the device evaluates it (src/CommonBlocksKernel.h:162-275: axis order by extent, pre-bits from (int)log2f of the
 * extent ratios, the bit budget): plan_out = {axis[3], bits[3], pre[2], pre_sum, swap}.  total_bits 30 = bvh_stage_morton, <= 60 = bvh_stage_morton64.  A host
 * that must reproduce the codes bit for bit (an oracle, a CPU fallback of its own) takes the plan from here instead of evaluating log2f with another math
 * library: OCML and a host libm may truncate differently when a ratio sits within an ulp of a power of two.  Blocking (one small read-back). */
int  bvh_stage_morton_plan(bvh_ctx* ctx, const void* d_scene_extent, int total_bits, int32_t plan_out[10]);
/* stage S on u64 keys, key bits [start_bit, end_bit) with end_bit <= 64 */
int  bvh_sort_pairs64(bvh_ctx* ctx, const uint64_t* d_keys_in, const uint32_t* d_vals_in, uint32_t n,
                      uint64_t* d_keys_out, uint32_t* d_vals_out, int start_bit, int end_bit);

/* ---- many small meshes in one call (what the reference's BatchedBuildKernelLbvh, src/BatchedBuildKernel.h:218-312, was meant to be) ---------
 * The bottom-level trees of an instanced scene — thousands of meshes of tens to hundreds of triangles — built by one call instead of one bvh_build_ex each
 * (which costs ~0.1 ms of launch latency per mesh whatever its size).  Mesh m is triangles [first, first + count) of the input arrays; every mesh's arrays land
 * in a slice of six caller-owned device arrays.  out_off[m] = the sum of the counts of meshes 0 .. m-1, total = the sum of all counts (host arithmetic).
 * algo: BVH_LBVH_SINGLEPASS or BVH_LBVH_TWOPASS (two-pass: every root is 0, so a host can fill every bvh_result without a read-back); anything else is
 * BVH_E_INVALID_ARG — PLOC++ trees of a batch come from bvh_build_many_ploc below.  in->morton_bits must be 30.
 * Formats: all three.  PADDED64 / PACKED36: mesh m reads records first .. first+count of d_tris; INDEXED: index triples first .. first+count of d_indices over the
 * shared d_vertices.  Leaf primitive indices and d_sorted_vals are mesh-local, 0 .. count-1.
 * bvh_many_tree (host arithmetic only, no device work) describes mesh m's slice as a bvh_result (layout 0, key_bits 32, d_leaves / d_morton_keys NULL) plus the
 * bvh_build_input that names its triangles, ready for bvh_intersect / bvh_closest_point / bvh_refit_ex / a bvh_blas: PADDED64 tree_out->d_tris = d_tris + 64*first
 * (tris_out names the same); PACKED36 tree_out->d_tris NULL and tris_out->d_tris = d_tris + 36*first — consumers need that 16-byte aligned, so bvh_build_many
 * itself rejects first % 4 != 0 for this format; INDEXED tree_out->d_tris NULL and tris_out->d_indices = d_indices + 3*first over the same vertices.
 * Identity: for every mesh the bytes of its node slice, its d_prim_aabbs slice, its root and its d_sorted_keys / d_sorted_vals slices equal what
 * bvh_build_ex(ctx2, algo, tris_out, count) produces; its scene extent compares equal and is byte-equal unless a coordinate is a zero of mixed sign (as for
 * bvh_refit_subset).  The bytes depend on neither the internal path that served the mesh, nor the other meshes of the batch, nor the call: sorted order is ascending
 * {key, mesh-local index} (the pipeline's stable 32-bit sort, codes with bits 30 / 31 set included); an internal box is the fminf / fmaxf union of the leaf boxes of
 * its range (every union order gives the same bits, mixed-sign zeros apart); nodes are numbered as the LBVH builders number them.
 * Paths: count <= 64: one wave per mesh, several meshes per workgroup; 65 .. BVH_MANY_LDS_MAX_PRIMS: one workgroup per mesh, extent, codes, sort and emit in LDS;
 * larger: the ordinary bvh_build_ex on the ctx, one mesh after another, its arrays copied to the slice — ONLY then the call counts as a build on the ctx (it
 * invalidates results that live in the ctx's arena and may re-allocate it) and waits for what such a build waits for.  The host bins the meshes by size, which is
 * why the ranges are host memory; they are read before the call returns.  No kernel waits on another wave or workgroup.
 * Nothing but the slices is written; the arena is untouched unless the large-mesh path runs.  Asynchronous on the ctx's stream apart from that path and from what
 * the timings need (profiling on: ms_build = ms_total = the whole call).  bvh_ctx_kernel_times reports k_many_wave and k_many_block.
 * Errors (BVH_E_INVALID_ARG, nothing is written or enqueued): NULL ctx / in / h_meshes / out, NULL d_nodes / d_prim_aabbs / d_scene_extents / d_roots, a format error
 * as in bvh_build_ex, morton_bits != 30, n_meshes == 0, a count < 2, first + count > n_tris, total >= 2^30, a misaligned PACKED36 first, output arrays overlapping
 * each other or the input; bvh_many_tree: m >= n_meshes, NULL h_roots for single-pass, NULL tree_out / tris_out. */
#define BVH_MANY_LDS_MAX_PRIMS 512          /* meshes up to this size are built in LDS by the batched kernels */
typedef struct { uint32_t first, count; } bvh_mesh_range;   /* triangles [first, first+count) of the input arrays */
typedef struct {
    void*     d_nodes;          /* Bvh2Node[2*total - n_meshes]; mesh m's LBVH-layout array (2*count-1 records) starts at record 2*out_off[m] - m */
    void*     d_prim_aabbs;     /* bvh_aabb[total];   mesh m's at out_off[m], by mesh-local primitive index */
    void*     d_scene_extents;  /* bvh_aabb[n_meshes] */
    uint32_t* d_roots;          /* u32[n_meshes]: mesh-local root (two-pass: 0) */
    uint32_t* d_sorted_keys;    /* u32[total] or NULL */
    uint32_t* d_sorted_vals;    /* u32[total] or NULL (mesh-local indices) */
} bvh_many_out;
int  bvh_build_many(bvh_ctx* ctx, bvh_algo algo, const bvh_build_input* in, uint32_t n_tris,
                    const bvh_mesh_range* h_meshes /* host */, uint32_t n_meshes, const bvh_many_out* out, bvh_timings* timings /* may be NULL */);
/* host arithmetic only, no device work: mesh m's slice as a caller-filled bvh_result + the bvh_build_input that names its triangles */
int  bvh_many_tree(bvh_algo algo, const bvh_build_input* in, const bvh_mesh_range* h_meshes, uint32_t n_meshes, const bvh_many_out* out,
                   uint32_t m, const uint32_t* h_roots /* NULL allowed for BVH_LBVH_TWOPASS: root 0 */, bvh_result* tree_out, bvh_build_input* tris_out);

/* ---- many small meshes in one call, PLOC++ trees ------------------------------------------------------------------------------------------
 * bvh_build_many for trees of PLOC++ quality (bottom-level trees are built once and traced every frame): same input, ranges, out_off / total, formats (PACKED36
 * first % 4 == 0), morton_bits 30, host-side binning (one launch per size class), item table outside the arena, asynchrony on the ctx's stream and timings
 * (ploc_iterations stays 0) as bvh_build_many.  algo: BVH_PLOCPP only (HPLOC's parity bar is not byte identity; it is not served here).
 * Output: PLOC layout.  Mesh m's n-1 node records start at record out_off[m] - m of d_nodes, its root is local node 0, a child >= n-1 is leaf child-(n-1); its n
 * PrimRef leaves start at out_off[m] of d_leaves in sorted (Morton) order, prim_idx mesh-local.  bvh_many_ploc_tree (host arithmetic only) describes the slice as a
 * bvh_result: layout 1, root 0, n_internal = count-1, key_bits 32, d_leaves set, d_morton_keys NULL; d_tris and tris_out as bvh_many_tree.
 * Identity: for every mesh whose candidate areas are all finite — true whenever the f32 area of its extent is finite: every union of member boxes lies inside
 * the extent and the area expression is monotone — the bytes of its node slice, leaf slice, d_prim_aabbs slice and d_sorted_keys / d_sorted_vals slices equal what
 * bvh_build_ex(ctx2, BVH_PLOCPP, tris_out, count) produces; the extent compares equal and is byte-equal unless a coordinate is a zero of mixed sign.  The bytes depend
 * on neither the path, nor the other meshes of the batch, nor the call.  A mesh with an infinite or NaN candidate area (boxes at +-FLT_MAX from clamped inf / NaN
 * vertices) gets a valid tree over the same leaves in finite time — neighbour keys are compared as integers, so every round has a mutual pair — but not
 * necessarily the ordinary build's bytes: that build's emit is compiled without NaN semantics.
 * Paths: count <= 64: one wave per mesh, several meshes per workgroup; 65 .. BVH_MANY_LDS_MAX_PRIMS: one workgroup per mesh, all rounds in LDS, the last ones
 * (<= 64 clusters) by its first wave; larger: bvh_build_ex(BVH_PLOCPP) on the ctx, its arrays copied to the slice — ONLY then the call counts as a build on the ctx.
 * No kernel waits on another wave or workgroup.  Nothing but the slices is written.  bvh_ctx_kernel_times reports k_many_ploc_wave and k_many_ploc_block.
 * Errors (BVH_E_INVALID_ARG, nothing is written or enqueued): everything bvh_build_many rejects (d_roots does not exist here), NULL d_leaves, an algo other than
 * BVH_PLOCPP, any of the six output arrays overlapping each other or the input; bvh_many_ploc_tree: m >= n_meshes, another algo, NULL tree_out / tris_out. */
typedef struct {
    void*     d_nodes;          /* Bvh2Node[total - n_meshes]; mesh m's n-1 records start at record out_off[m] - m; root = local node 0 */
    void*     d_leaves;         /* PrimRef[total] (28-byte records); mesh m's at out_off[m], in sorted (Morton) order, prim_idx mesh-local */
    void*     d_prim_aabbs;     /* bvh_aabb[total], by mesh-local primitive index */
    void*     d_scene_extents;  /* bvh_aabb[n_meshes] */
    uint32_t* d_sorted_keys;    /* u32[total] or NULL */
    uint32_t* d_sorted_vals;    /* u32[total] or NULL (mesh-local indices) */
} bvh_many_ploc_out;
int  bvh_build_many_ploc(bvh_ctx* ctx, bvh_algo algo /* BVH_PLOCPP */, const bvh_build_input* in, uint32_t n_tris,
                         const bvh_mesh_range* h_meshes /* host */, uint32_t n_meshes, const bvh_many_ploc_out* out, bvh_timings* timings /* may be NULL */);
/* host arithmetic only, no device work: mesh m's slice as a caller-filled bvh_result + the bvh_build_input that names its triangles */
int  bvh_many_ploc_tree(bvh_algo algo, const bvh_build_input* in, const bvh_mesh_range* h_meshes, uint32_t n_meshes, const bvh_many_ploc_out* out,
                        uint32_t m, bvh_result* tree_out, bvh_build_input* tris_out);

/* ---- refit (no counterpart in the reference) ------------------------------------------------------------------------------------------
 * Recompute every box of an existing tree from new triangle positions, with the topology kept (deforming / animated meshes: vertices move, connectivity
 * and ordering stay).  Stage E, then the boxes are unioned bottom-up through the existing child links; Morton codes, sort and hierarchy search are skipped.
 * io: a result of bvh_build / bvh_build_ex on this ctx, or a caller-filled bvh_result whose arrays are device arrays on the ctx's device.
 * Written in place: leaf boxes (LBVH layout: nodes n-1 .. 2n-2; PLOC layout: d_leaves[j].aabb), every internal node's aabb, d_prim_aabbs, d_scene_extent;
 * io->d_tris is set to the triangles read.  Child links, leaf prim indices, root, d_sorted_* and d_morton_keys are not touched (the keys still describe the
 * mesh the tree was built from).  tris: Triangle[io->n_leaves], host or device, as in bvh_build.  timings: optional, same meaning and sampling rules as for a
 * build: ms_extents = stage E, ms_build = the refit proper (ms_morton / ms_sort are 0); bvh_ctx_kernel_times reports its kernels as k_refit_plan / k_refit_climb.
 * Contract: leaf boxes (and d_prim_aabbs) are bit-identical to what stage E writes for the same input; an internal box is the componentwise fminf / fmaxf union
 * of its two children's boxes, so a refit with the triangles the tree was built from reproduces the build's arrays.
 * The parent plan of the ctx's own tree is made once and kept until a build (or an emit) rewrites it; caller-owned arrays get a new plan on every call.
 * Errors (nothing is changed): NULL ctx / io / input, n_leaves < 2, layout not 0 or 1, NULL d_nodes / d_prim_aabbs / d_scene_extent, layout 1 with NULL
 * d_leaves, root not an internal node, an input format error: BVH_E_INVALID_ARG.  n_leaves larger than the ctx's capacity: BVH_E_INVALID_ARG — a refit
 * never re-allocates the arena (io may point into it); call bvh_ctx_reserve first.  Asynchronous like a build, except for what the timings need. */
int  bvh_refit(bvh_ctx* ctx, bvh_result* io, const void* tris, int tris_on_device, bvh_timings* timings /* may be NULL */);
/* the same on any bvh_tri_format (morton_bits is ignored) */
int  bvh_refit_ex(bvh_ctx* ctx, bvh_result* io, const bvh_build_input* in, bvh_timings* timings /* may be NULL */);
/* Partial refit: new boxes for the listed primitives' leaves and for the nodes on the paths from those leaves to the root — nothing else is written, and the work
 * is bounded by n_dirty x depth (a few moved triangles in a large static tree).  io: any tree bvh_refit accepts, either layout.  in: the COMPLETE triangle arrays with
 * the moved triangles already updated in place, any bvh_tri_format, validated as by bvh_refit_ex (NULL: io->d_tris is Triangle[n_leaves]).  d_prims: device array of
 * the primitive indices whose triangles changed; duplicates are allowed in any number, an index >= n_leaves is ignored.
 * For every distinct listed primitive p: d_prim_aabbs[p] and the box of the leaf record that holds p become the box stage E writes for triangle p (bit-identical,
 * NaN / infinity clamping included; a primitive no leaf holds gets only its d_prim_aabbs entry).  Every internal node on a path from such a leaf to the root gets the
 * componentwise fminf / fmaxf union of its two children's boxes as they are after the call: a child off every dirty path contributes the box it stores — it is read,
 * never recomputed.  d_scene_extent becomes the root's new box; io->d_tris is set as by bvh_refit_ex.  NOT written: node and leaf records off every dirty path,
 * d_prim_aabbs of unlisted primitives, child links, leaf prim indices, root, d_sorted_*, d_morton_keys.
 * If every unlisted triangle of `in` yields the box already stored for it, all arrays compare equal to those after bvh_refit_ex(ctx, io, in) (byte-identical when no
 * coordinate is a zero of mixed sign).  Arrays that are not a tree: the call ends in finite time with unspecified boxes and writes nothing outside the arrays.
 * The parent plan and the leaf map (which leaf holds which primitive) of the ctx's own tree are made once and kept as bvh_refit's plan is — bvh_optimize keeps
 * both valid —, caller-owned arrays get new ones on every call, and the call after one on caller-owned arrays first zeroes 8 bytes
 * per primitive of capacity: on caller-owned arrays the call costs O(capacity), not O(n_dirty x depth).  The first call on a ctx (and the first after its capacity grew) allocates 12 bytes per primitive
 * of capacity outside the arena; if that fails the HIP error is returned and nothing has changed.
 * timings: ms_extents = the box pass, ms_build = plan + map + mark + climb, sampling rules of a build.  bvh_ctx_kernel_times reports k_refit_subset_boxes /
 * k_refit_subset_mark / k_refit_subset_climb and, when they run, k_refit_plan / k_refit_leafmap.  Above some dirty fraction bvh_refit is the faster
 * call; where that lies has not been measured yet (tools/time_refit_subset.py writes it to profiles/refit_subset.md).
 * Errors (nothing is written or enqueued): those of bvh_refit_ex, NULL d_prims with n_dirty > 0, n_dirty >= 2^30, d_prims overlapping an array the call writes:
 * BVH_E_INVALID_ARG.  n_dirty == 0 returns 0 and touches nothing.  Asynchronous on the ctx's stream, except for what the timings need. */
int  bvh_refit_subset(bvh_ctx* ctx, bvh_result* io, const bvh_build_input* in /* NULL: io->d_tris is Triangle[n_leaves] */,
                      const uint32_t* d_prims /* device, [n_dirty] */, uint32_t n_dirty, bvh_timings* timings /* may be NULL */);

/* ---- ray queries (no counterpart in the reference) -----------------------------------------------------------------------------------
 * Which triangle does each ray hit first (BVH_QUERY_CLOSEST), or does it hit any (BVH_QUERY_ANY)?  One bvh_hit per ray: d_hits[i] answers d_rays[i].
 * tree: a result of bvh_build / bvh_build_ex / bvh_refit on this ctx, or a caller-filled bvh_result whose arrays are device arrays on the ctx's device (for instance a
 * tree read back with bvh_batch_download and uploaded again).  Both layouts are read as they are (no bvh_to_lbvh_layout copy): layout 0 = Bvh2Node[2n-1] with leaf j at
 * node n-1+j; layout 1 = Bvh2Node[n-1] + PrimRef[n], a child >= n-1 is leaf child-(n-1).  Read: root, n_leaves, layout, d_nodes, d_leaves, d_tris; nothing is written
 * to the tree.  The arrays must form a tree; a primitive or child index out of range is never followed (the primitive is skipped, the child treated as empty), and
 * arrays that are not a tree end in finite time with unspecified hits.  There is no depth limit: rays whose short stack would overflow are finished by a stackless pass.
 * tris: the triangles, any bvh_tri_format, validated as by bvh_build_ex (morton_bits is ignored; INDEXED indices >= n_vertices are read as vertex 0).  NULL:
 * tree->d_tris is read as Triangle[n_leaves] — a bvh_result does not record the format it was built from, so trees built from packed or indexed input pass `tris`.
 * Hit test: the reference's intersectTriangle (src/Common.h:516-531) without a transform, in f32 operation for operation: iu, iv, iw, it.  A hit is accepted iff
 * iu > 0 && iv > 0 && iw > 0 && tmin < it < tmax.  The test is two-sided (either winding is hit); a ray through an edge or a vertex exactly (an iu, iv or iw of 0)
 * misses.  Directions need not be normalised: t is measured in units of `direction`.
 * BVH_QUERY_CLOSEST: the accepted hit with the smallest (t, prim_idx), compared lexicographically — the answer does not depend on the builder, the layout, the
 * traversal order or the input format.  BVH_QUERY_ANY: some accepted hit (which one is unspecified; traversal stops at the first), t / u / v exactly as the
 * formula gives them for that primitive.  A hit is written as {it, iu, iv, prim_idx}; a miss as {t = ray.tmax, u = 0, v = 0, prim_idx = BVH_INVALID}.  Rays with a
 * NaN component, or with !(tmin < tmax), miss.  Zero direction components and origins on a box plane are handled.
 * Box tests are conservative: a subtree is culled only when it cannot hold an accepted hit of a well-conditioned ray (DESIGN.md §8b states the margins: every box
 * grows on every axis by 2^-16 times its largest |coordinate|, slab interval ends widen by 2^-20 relative; "well-conditioned": every accepted hit's point o + t*d
 * lies in its triangle's box grown by half that growth).
 * Errors (nothing is written): NULL ctx / tree / d_rays / d_hits, n_leaves < 2, layout not 0 or 1, NULL d_nodes, layout 1 with NULL d_leaves, root not an internal
 * node, no triangles (tris NULL and tree->d_tris NULL) or a tris format error, query not 0 or 1, overlapping d_rays / d_hits ranges: BVH_E_INVALID_ARG.  n_leaves
 * larger than the ctx's capacity: BVH_E_INVALID_ARG — a query never re-allocates the arena (the tree may live in it); call bvh_ctx_reserve first.  n_rays == 0: 0,
 * nothing is touched.
 * Asynchronous on the ctx's stream, no read-back.  bvh_ctx_kernel_times reports k_intersect, k_intersect_deep and, when the parent plan of the stackless pass is made,
 * k_refit_plan.  The plan of the ctx's own tree is made once and kept as for bvh_refit; caller-owned arrays get a new plan on every call. */
typedef enum { BVH_QUERY_CLOSEST = 0, BVH_QUERY_ANY = 1 } bvh_query_kind;
int  bvh_intersect(bvh_ctx* ctx, const bvh_result* tree, const bvh_build_input* tris /* NULL: tree->d_tris is Triangle[n_leaves] */,
                   const bvh_ray* d_rays, uint32_t n_rays, bvh_hit* d_hits, int query /* bvh_query_kind */);

/* ---- all-hits ray queries (no counterpart in the reference) ------------------------------------------------------------------------------
 * Which triangles does each ray cross, ALL of them?  Transparency and alpha layers, thickness and path-length integrals, crossing-number inside / outside
 * tests on closed meshes, CSG intervals, x-ray and attenuation renders, counting the shells a sensor ray passes through.  One call instead of re-issuing
 * bvh_intersect with tmin moved past the last hit, which costs a descent per layer and loses hits that share a t.
 * tree / tris: exactly as bvh_intersect — any bvh_result in either layout, read as it is (a build's, a refit's, an optimised or a caller-filled one on the
 * ctx's device), triangles in any bvh_tri_format validated as by bvh_build_ex (NULL: tree->d_tris is read as Triangle[n_leaves]); nothing in the tree is
 * written; a primitive or child index out of range is never followed, and arrays that are not a tree end in finite time with unspecified answers.
 * Hit test and acceptance: bvh_intersect's, word for word — the reference's intersectTriangle in f32, operation for operation; a hit is accepted iff
 * iu > 0 && iv > 0 && iw > 0 && tmin < it < tmax.  A ray with a NaN component, or with !(tmin < tmax), accepts nothing.
 * Answer: ray i's set is ALL its accepted hits, as {it, iu, iv, prim_idx} records in compressed-row form: d_hits[d_offsets[i] .. d_offsets[i+1]) is ray i's
 * slice, d_offsets[0] = 0, d_offsets[n_rays] = the total.  Each primitive appears at most once per slice.  There are no miss records: an empty slice is a
 * miss.  With d_hits == NULL the call only counts: d_offsets is then the rays' crossing numbers in scanned form.
 * Order inside a slice: without BVH_HITS_SORTED unspecified, but the same call on the same arrays gives the same bytes.  With BVH_HITS_SORTED each slice is in
 * ascending (t, prim_idx) order, compared lexicographically; the whole d_hits array then does not depend on the builder, the layout, the scheduler, the
 * triangle format or the traversal order.  Any other flag bit is an error.
 * Box tests are bvh_intersect's conservative test (boxes grow by 2^-16 times their largest |coordinate|, slab interval ends widen by 2^-20
 * relative) against [tmin, tmax] for the whole walk: the bound never shrinks.  §8b's argument needs only it < bound, which holds for every accepted hit, so on
 * a well-conditioned ray (§8b's definition, unchanged: every accepted hit's point o + t*d lies in its triangle's box grown by half that growth) no ancestor of
 * an accepted hit is culled and the set is exact.  On EVERY ray each reported record is an accepted hit of its primitive with bit-equal t / u / v, and the
 * slice is a subset of the true set.
 * Passes: the call always counts, then scans the counts into d_offsets, and keeps the 64-bit total in a device word.  It fills d_hits iff d_hits != NULL,
 * total <= capacity and total < 2^32; that decision is made ON THE DEVICE (the fill launch reads the total word and returns at once), so the call stays
 * asynchronous on the ctx's stream.  If the fill is skipped d_hits is not touched and d_offsets is still complete.  With total_out != NULL the call blocks on
 * an 8-byte read-back into pinned words and stores the total; a host that guessed too small a capacity re-allocates and calls again.  A total of 2^32 or more
 * saturates d_offsets at 0xFFFFFFFF; if total_out was given the call then returns BVH_E_TOO_LARGE (with *total_out set).  d_hits is never written outside
 * ray i's slice, nor past the total.
 * There is no depth limit: a ray whose short stack would overflow is finished by a stackless pass through bvh_refit's parent plan, cached for the ctx's own
 * tree as for bvh_intersect and made per call for caller-owned arrays.  Count and fill agree on every ray's set whichever pass served it.
 * Errors (nothing is written or enqueued, BVH_E_INVALID_ARG): bvh_intersect's (NULL ctx / tree / d_rays, n_leaves < 2, layout not 0 or 1, NULL d_nodes,
 * layout 1 with NULL d_leaves, root not an internal node, no triangles or a tris format error, n_leaves larger than the ctx's capacity: call bvh_ctx_reserve
 * first); NULL d_offsets; a flag bit other than BVH_HITS_SORTED; n_rays >= 2^30; d_offsets or d_hits (capacity records) overlapping d_rays or each other.
 * n_rays == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.
 * bvh_ctx_kernel_times reports k_hits_count, k_hits_deep (after each pass), k_overlap_scan (the scan is bvh_overlap's), k_hits_fill and, when the plan is
 * made, k_refit_plan. */
#define BVH_HITS_SORTED 1u
int  bvh_intersect_all(bvh_ctx* ctx, const bvh_result* tree, const bvh_build_input* tris /* NULL: tree->d_tris is Triangle[n_leaves] */,
                       const bvh_ray* d_rays, uint32_t n_rays, uint32_t flags /* 0 or BVH_HITS_SORTED */,
                       uint32_t* d_offsets /* u32[n_rays + 1], device */, bvh_hit* d_hits /* [capacity], device, or NULL: count only */,
                       uint64_t capacity, uint64_t* total_out /* host, may be NULL */);

/* ---- point queries (no counterpart in the reference) -----------------------------------------------------------------------------------
 * Which point of the mesh is nearest to each query point within its radius (BVH_QUERY_CLOSEST), or is any triangle within the radius (BVH_QUERY_ANY)?  One
 * bvh_point_hit per query: d_hits[i] answers d_points[i].  Unsigned distance fields (the sign is bvh_winding_number's), proximity tests, projection onto a surface, ICP correspondences.
 * tree / tris: exactly as bvh_intersect — any bvh_result in either layout (a build's, a refit's, an optimised or a caller-filled one on the ctx's device),
 * triangles in any bvh_tri_format (NULL: tree->d_tris is read as Triangle[n_leaves]); the same validation; arrays that are not a tree end in finite time.
 * Candidate: Ericson's ClosestPtPointTriangle (Real-Time Collision Detection, 5.1.5) in f32, operation for operation, no contraction, a = v1, b = v2, c = v3;
 * every dot product is (x*x' + y*y') + z*z'; regions tested in Ericson's order: A, B, edge AB, C, edge AC, edge BC, interior; denom = 1.0f / ((va + vb) + vc)
 * (correctly rounded division).  Point: a, b or c at a vertex; a_k + v*ab_k on AB; a_k + w*ac_k on AC; b_k + w*(c_k - b_k) on BC; (a_k + ab_k*v) + ac_k*w
 * inside.  (u, v) = the weights of v2 and v3: (0,0) at A, (1,0) at B, (0,1) at C, (v,0) on AB, (0,w) on AC, (1.0f - w, w) on BC, (v, w) inside.
 * dist2 = (dx*dx + dy*dy) + dz*dz with d = point - p.  (The formula is the contract even where it is inexact: on a collinear triangle, rounding noise in
 * va, vb, vc can select the interior branch, whose point then lies on the triangle's line but not necessarily on the triangle.)
 * Acceptance: a candidate is accepted iff dist2 <= r2, r2 = radius*radius in f32 (NaN is never accepted; an infinite radius is no bound).  Queries with a NaN
 * coordinate, a NaN radius or radius < 0 miss.
 * BVH_QUERY_CLOSEST: the accepted candidate with the smallest (dist2, prim_idx), compared lexicographically — the answer does not depend on the builder, the
 * layout, the traversal order or the input format.  BVH_QUERY_ANY: some accepted candidate (traversal stops at the first): "is anything within r".
 * A hit is written as {point, dist2, u, v, prim_idx, 0}; a miss as {0, 0, 0, r2, 0, 0, BVH_INVALID, 0}.
 * Box tests are conservative: every box grows on every axis by 2^-16 times its largest |coordinate|, its f32 squared distance to the point is
 * lb, and the subtree is kept iff lb * (1 - 2^-20) <= the best dist2 so far (r2 at the start).  Answers are exact on well-conditioned queries: the f64
 * squared distance from the point to the closest answer's triangle box grown by 2^-17 times its largest |coordinate| is <= that answer's dist2.  On every
 * query a reported hit is an accepted candidate, and a closest answer is never below the true best.
 * Errors (nothing is written): NULL ctx / tree / d_points / d_hits, n_leaves < 2, layout not 0 or 1, NULL d_nodes, layout 1 with NULL d_leaves, root not an
 * internal node, no triangles (tris NULL and tree->d_tris NULL) or a tris format error, query not 0 or 1, overlapping d_points / d_hits ranges:
 * BVH_E_INVALID_ARG.  n_leaves larger than the ctx's capacity: BVH_E_INVALID_ARG (the parent plan lives in the arena; call bvh_ctx_reserve first).
 * n_points == 0: 0, nothing is touched.
 * Asynchronous on the ctx's stream, no read-back.  There is no depth limit: queries whose short stack would overflow are finished by a stackless pass through
 * bvh_refit's parent plan, cached for the ctx's own tree as for bvh_intersect.  bvh_ctx_kernel_times reports k_closest_point, k_closest_point_deep and, when
 * the plan is made, k_refit_plan. */
int  bvh_closest_point(bvh_ctx* ctx, const bvh_result* tree, const bvh_build_input* tris /* NULL: tree->d_tris is Triangle[n_leaves] */,
                       const bvh_point_query* d_points, uint32_t n_points, bvh_point_hit* d_hits, int query /* bvh_query_kind */);

/* ---- winding numbers (no counterpart in the reference) -----------------------------------------------------------------------------------
 * Is each query point inside the mesh?  The generalized winding number w(q) = the sum over the triangles of their signed solid angle seen from q, over 4 pi: 1
 * inside a closed, outward-oriented mesh, 0 outside, and a smooth function in between on meshes with holes, on triangle soups and on open scans.  Point-in-mesh
 * (w > 0.5), the SIGN of a distance field (bvh_closest_point's distance, negated where w > 0.5), voxelisation and fill, repair of open scans.  Evaluated
 * hierarchically as in Barill et al., "Fast winding numbers for soups and clouds" (2018): a far subtree contributes one dipole term, a near one is opened.
 * On instanced scenes: bvh_scene_winding_number, below.  Two calls: bvh_winding_prepare once per tree, bvh_winding_number per batch of points.
 * tree / tris: exactly as bvh_closest_point — any bvh_result in either layout (a build's, a refit's, an optimised or a caller-filled one on the ctx's device),
 * triangles in any bvh_tri_format validated as by bvh_build_ex (NULL: tree->d_tris is read as Triangle[n_leaves]).  Nothing in the tree is written.  A
 * primitive or child index out of range is skipped (it contributes nothing); arrays that are not a tree end in finite time with unspecified answers.
 * All arithmetic below is f32 without contraction unless stated; every dot product is (x*x' + y*y') + z*z' and cross(u, v) = (uy*vz - uz*vy, uz*vx - ux*vz,
 * ux*vy - uy*vx); divisions and square roots are correctly rounded.
 *
 * bvh_winding_prepare writes one bvh_winding_moment per internal node: d_moments[i] belongs to node i, i in [0, n_leaves - 1).
 *   leaf (triangle a, b, c = v1, v2, v3): A = 0.5f * cross(b - a, c - a); area = sqrtf((Ax*Ax + Ay*Ay) + Az*Az); centroid c = ((a + b) + c) * (1.0f / 3.0f)
 *     per component; first moment M = area * c.
 *   internal node: A, area and M are the sums left + right of its children's values, componentwise, in that order.  The sums follow the tree and not the order
 *     in which the threads arrive, so the record is a function of the tree and the triangles alone and is bit-reproducible.
 *   p = M / area per component; if area is 0 or not finite, p = (lo + hi) * 0.5f per axis, the centre of the node's stored box.
 *   r = sqrtf((x*x + y*y) + z*z) with, per axis, the larger of |lo - p| and |hi - p| (a NaN side is ignored): the distance from p to the farthest corner of the box.
 *   The record is {Ax, Ay, Az, area, px, py, pz, r}.  d_moments is caller-owned device memory, 16-byte aligned.
 *   The moments describe the tree's topology, its boxes and the triangles at the time of the call: after a refit, an optimise or a rebuild they are STALE and
 *   the caller prepares again.  bvh_winding_number does not and cannot check this.
 *
 * bvh_winding_number answers d_points[i] (its radius is ignored) with d_w[i].  The walk starts at the root, which is always opened; an opened node's children
 * are taken left first:
 *   a leaf child adds the Van Oosterom–Strackee solid angle of its triangle: a, b, c = v1 - q, v2 - q, v3 - q; num = dot(a, cross(b, c)); la, lb, lc =
 *     sqrtf(dot(a, a)), ...; den = (((la*lb)*lc + dot(a, b)*lc) + dot(b, c)*la) + dot(c, a)*lb; term = (2.0f * atan2f(num, den)) / FOURPI, FOURPI = 4 pi
 *     rounded to f32.
 *   an internal child with record {A, area, p, r}: d = p - q; d2 = (dx*dx + dy*dy) + dz*dz; t = beta * r.  The child is APPROXIMATED iff d2 > t * t — false
 *     on NaN, so beta = +inf opens everything and the answer is then the plain sum over all triangles.  Its term is dot(A, d) / ((FOURPI * d2) * sqrtf(d2)).
 *     Otherwise the child is opened.
 *   The f32 terms are accumulated in f64 (the summation order is not part of the contract) and the sum is stored as f32.  A NaN answer is stored as the quiet NaN
 *   0x7FC00000.  A query with a NaN coordinate writes that NaN.
 * beta trades accuracy for speed: 2 is Barill et al.'s default; larger opens more (DESIGN.md §8s has measured errors).  The decision and every term are stated
 * above, so an answer depends on the tree, the triangles and the moments only — not on the scheduler — up to the rounding of the f64 sum and of atan2f.
 * Errors (nothing is written or enqueued, BVH_E_INVALID_ARG): NULL ctx / tree / d_moments (and, for the query, NULL d_points / d_w), n_leaves < 2, layout not 0 or
 * 1, NULL d_nodes, layout 1 with NULL d_leaves, root not an internal node, no triangles (tris NULL and tree->d_tris NULL) or a tris format error, n_leaves larger
 * than the ctx's capacity (the parent plan and the exchange words live in the arena; call bvh_ctx_reserve first), d_moments not 16-byte aligned, d_moments
 * overlapping a node, leaf, triangle, vertex or index array of the call; for the query also beta < 0 or NaN, d_moments overlapping d_points or d_w, and d_w
 * overlapping d_points or any tree or triangle array.  n_points == 0: 0, nothing is touched.
 * Asynchronous on the ctx's stream, no read-back.  There is no depth limit: queries whose short stack would overflow are finished by a stackless pass through
 * bvh_refit's parent plan, cached for the ctx's own tree as for bvh_intersect; the climb of bvh_winding_prepare uses the same plan.  bvh_ctx_kernel_times
 * reports k_winding_climb and k_winding_finish (prepare), k_winding and k_winding_deep (query) and, when the plan is made, k_refit_plan. */
int  bvh_winding_prepare(bvh_ctx* ctx, const bvh_result* tree, const bvh_build_input* tris /* NULL: tree->d_tris is Triangle[n_leaves] */,
                         bvh_winding_moment* d_moments /* [n_leaves - 1], device, caller-owned */);
int  bvh_winding_number(bvh_ctx* ctx, const bvh_result* tree, const bvh_build_input* tris /* NULL: tree->d_tris is Triangle[n_leaves] */,
                        const bvh_winding_moment* d_moments, const bvh_point_query* d_points /* radius ignored */, uint32_t n_points, float beta,
                        float* d_w /* f32[n_points], device */);

/* ---- k-nearest queries (no counterpart in the reference) -------------------------------------------------------------------------------
 * Which k triangles are nearest to each query point within its radius?  k (dist2, prim_idx) records per query: query i's list is d_hits[i*k .. i*k+k).
 * Point-cloud normals, kNN graphs, particle neighbourhoods, Chamfer-style losses, robust ICP.
 * tree / tris: exactly as bvh_closest_point — any bvh_result in either layout (a build's, a refit's, an optimised or a caller-filled one on the ctx's device),
 * triangles in any bvh_tri_format (NULL: tree->d_tris is read as Triangle[n_leaves]); the same validation; arrays that are not a tree end in finite time.
 * Candidate and acceptance are bvh_closest_point's, word for word: the candidate of a triangle is Ericson's ClosestPtPointTriangle in f32, operation for
 * operation as stated there, dist2 = (dx*dx + dy*dy) + dz*dz; it is accepted iff dist2 <= r2, r2 = radius*radius in f32 (an infinite radius is no bound).
 * Queries with a NaN coordinate, a NaN radius or radius < 0 are dead: they accept nothing.  A triangle with a NaN vertex is never accepted (its dist2 is NaN).
 * Answer: query i's list is the min(k, accepted) accepted candidates with the smallest (dist2, prim_idx), compared lexicographically, stored in ascending
 * order — it does not depend on the builder, the layout, the scheduler, the input format or the traversal order.  Slots past the list are
 * {r2, BVH_INVALID}; for a dead query that is all k of them.  d_counts[i], when d_counts is given, is the list's length.
 * With k == 1 the record equals (dist2, prim_idx) of bvh_closest_point BVH_QUERY_CLOSEST bit for bit, on every query.  A tree with fewer than k triangles is
 * fine: the lists are short.
 * Point clouds are served by degenerate triangles v1 == v2 == v3: region A of the formula then gives dist2 = |p - v1|^2 exactly as (dx*dx + dy*dy) + dz*dz
 * with d = v1 - p, and prim_idx is the point's index.  BVH_TRI_PACKED36 (nine floats per point) is the cheap input for it.
 * Box tests are bvh_closest_point's: every box grows on every axis by 2^-16 times its largest |coordinate|, its f32 squared distance to
 * the point is lb, and the subtree is kept iff lb * (1 - 2^-20) <= the current bound: the dist2 of the list's last entry once the list holds k entries, r2
 * before that.  The <= keeps a candidate of equal dist2 and smaller prim_idx reachable.  A query is well-conditioned when every entry of its true list
 * satisfies §8e's condition: the f64 squared distance from the point to that triangle's box, grown by 2^-17 times its largest |coordinate|, is <= its dist2.
 * The bound never drops below the true k-th dist2, so on such queries no ancestor of a true answer is culled and the list is exact.  On every query each
 * reported entry is an accepted candidate of its prim with a bit-equal dist2, the entries are strictly ascending in (dist2, prim_idx), and no list is
 * lexicographically below the true one.
 * Errors (nothing is written or enqueued, BVH_E_INVALID_ARG): bvh_closest_point's (NULL ctx / tree / d_points / d_hits, n_leaves < 2, layout not 0 or 1, NULL
 * d_nodes, layout 1 with NULL d_leaves, root not an internal node, no triangles or a tris format error, n_leaves larger than the ctx's capacity); k == 0 or
 * k > BVH_KNN_MAX_K; the d_points / d_hits / d_counts ranges overlapping each other; n_points * k >= 2^32.  n_points == 0: 0, nothing is touched.
 * Asynchronous on the ctx's stream, no read-back.  There is no depth limit: queries whose short stack would overflow are finished by a stackless pass through
 * bvh_refit's parent plan, cached for the ctx's own tree as for bvh_intersect.  bvh_ctx_kernel_times reports k_knn, k_knn_deep and, when the plan is made,
 * k_refit_plan. */
#define BVH_KNN_MAX_K 32
int  bvh_knn(bvh_ctx* ctx, const bvh_result* tree, const bvh_build_input* tris /* NULL: tree->d_tris is Triangle[n_leaves] */,
             const bvh_point_query* d_points, uint32_t n_points, uint32_t k, bvh_knn_hit* d_hits /* [n_points * k], query i's list at d_hits[i*k .. i*k+k) */,
             uint32_t* d_counts /* [n_points] or NULL */);

/* ---- radius searches (no counterpart in the reference) ---------------------------------------------------------------------------------
 * Which triangles lie within the radius of each query point, ALL of them?  The fixed-radius range search: SPH and particle neighbourhoods on point clouds,
 * contact and proximity detection with a margin, narrow-band distance fields where more than the nearest triangle matters, brush spheres of mesh painting and
 * selection, density estimates.  One call instead of bvh_knn with a k that may be too small (its lists are capped at BVH_KNN_MAX_K), or bvh_overlap with the
 * sphere's box and an exact-distance filter on the host.
 * tree / tris: exactly as bvh_closest_point — any bvh_result in either layout, read as it is (a build's, a refit's, an optimised or a caller-filled one on the
 * ctx's device), triangles in any bvh_tri_format validated as by bvh_build_ex (NULL: tree->d_tris is read as Triangle[n_leaves]); nothing in the tree is
 * written; a primitive or child index out of range is never followed, and arrays that are not a tree end in finite time with unspecified answers.
 * Candidate and acceptance are bvh_closest_point's, word for word: the candidate of a triangle is Ericson's ClosestPtPointTriangle in f32, operation for
 * operation as stated there, dist2 = (dx*dx + dy*dy) + dz*dz; it is accepted iff dist2 <= r2, r2 = radius*radius in f32.  An infinite radius accepts every
 * triangle whose dist2 is not NaN (a triangle with a NaN vertex is never accepted).  Queries with a NaN coordinate, a NaN radius or radius < 0 are dead: they
 * accept nothing.  radius 0 (or -0) accepts the triangles at dist2 == 0.
 * Answer: query i's set is ALL its accepted candidates, as {dist2, prim_idx} records (bvh_knn_hit) in compressed-row form: d_hits[d_offsets[i] ..
 * d_offsets[i+1]) is query i's slice, d_offsets[0] = 0, d_offsets[n_points] = the total.  Each primitive appears at most once per slice.  There is no padding
 * and there are no miss records: an empty slice is "nothing within r".  With d_hits == NULL the call only counts: d_offsets is then the queries' neighbour
 * counts in scanned form.
 * Point clouds are served by degenerate triangles v1 == v2 == v3, as for bvh_knn: dist2 = |p - v1|^2 as (dx*dx + dy*dy) + dz*dz, prim_idx the point's index.
 * Order inside a slice: without BVH_RADIUS_SORTED unspecified, but the same call on the same arrays gives the same bytes.  With BVH_RADIUS_SORTED each slice is
 * in ascending (dist2, prim_idx) order, compared lexicographically; the whole d_hits array then does not depend on the builder, the layout, the scheduler, the
 * triangle format or the traversal order, and the first min(k, count) records of a slice are bvh_knn's list.  Any other flag bit is an error.  The sorted fill
 * inserts each record into its slice as it is found, which is quadratic in the slice's length: very long sorted slices (thousands of neighbours per query)
 * are the caller's to avoid, or to fill unsorted and sort themselves.
 * Box tests are bvh_closest_point's conservative test (every box grows on every axis by 2^-16 times its largest |coordinate|, its f32 squared
 * distance to the point is lb, the subtree is kept iff lb * (1 - 2^-20) <= the bound) against r2 for the whole walk: the bound never shrinks.  A query is
 * well-conditioned when every accepted triangle satisfies §8e's condition: the f64 squared distance from the point to that triangle's box, grown by 2^-17
 * times its largest |coordinate|, is <= its dist2.  On such queries no ancestor of an accepted triangle is culled and the set is exact.  On
 * EVERY query each reported record is an accepted candidate of its primitive with a bit-equal dist2, and the slice is a subset of the true set.
 * Passes: the call always counts, then scans the counts into d_offsets, and keeps the 64-bit total in a device word.  It fills d_hits iff d_hits != NULL,
 * total <= capacity and total < 2^32; that decision is made ON THE DEVICE (the fill launch reads the total word and returns at once), so the call stays
 * asynchronous on the ctx's stream.  If the fill is skipped d_hits is not touched and d_offsets is still complete.  With total_out != NULL the call blocks on
 * an 8-byte read-back into pinned words and stores the total; a host that guessed too small a capacity re-allocates and calls again.  A total of 2^32 or more
 * saturates d_offsets at 0xFFFFFFFF; if total_out was given the call then returns BVH_E_TOO_LARGE (with *total_out set).  d_hits is never written outside
 * query i's slice, nor past the total.
 * There is no depth limit: a query whose short stack would overflow, or whose walk exceeds the node count, is redone by a stackless pass through bvh_refit's
 * parent plan, cached for the ctx's own tree as for bvh_intersect and made per call for caller-owned arrays.  Count and fill agree on every query's set
 * whichever pass served it.
 * Errors (nothing is written or enqueued, BVH_E_INVALID_ARG): bvh_closest_point's (NULL ctx / tree / d_points, n_leaves < 2, layout not 0 or 1, NULL d_nodes,
 * layout 1 with NULL d_leaves, root not an internal node, no triangles or a tris format error, n_leaves larger than the ctx's capacity: call bvh_ctx_reserve
 * first); NULL d_offsets; a flag bit other than BVH_RADIUS_SORTED; n_points >= 2^30; d_offsets or d_hits (capacity records) overlapping d_points or each other.
 * n_points == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.
 * bvh_ctx_kernel_times reports k_radius_count, k_radius_deep (after each pass), k_overlap_scan (the scan is bvh_overlap's), k_radius_fill and, when the plan is
 * made, k_refit_plan. */
#define BVH_RADIUS_SORTED 1u
int  bvh_radius_search(bvh_ctx* ctx, const bvh_result* tree, const bvh_build_input* tris /* NULL: tree->d_tris is Triangle[n_leaves] */,
                       const bvh_point_query* d_points, uint32_t n_points, uint32_t flags /* 0 or BVH_RADIUS_SORTED */,
                       uint32_t* d_offsets /* u32[n_points + 1], device */, bvh_knn_hit* d_hits /* [capacity], device, or NULL: count only */,
                       uint64_t capacity, uint64_t* total_out /* host, may be NULL */);

/* ---- box queries (no counterpart in the reference) -------------------------------------------------------------------------------------
 * Which primitives does each box touch?  The broad phase of collision detection, region selection, culling against an axis-aligned volume, neighbour gathering
 * on a bvh_build_boxes tree, "which instances does this volume touch" on a scene's top-level tree.
 * tree: any bvh_result bvh_intersect accepts, in either layout, read as it is — a build's, a refit's, an optimised one, a bvh_build_boxes tree, a
 * bvh_scene_tlas result, or caller-filled device arrays.  Only root, n_leaves, layout, d_nodes and d_leaves are read; no triangles are needed; nothing in the
 * tree is written.  A primitive's box is its leaf record's box (layout 0: node n-1+j; layout 1: d_leaves[j].aabb).
 * Overlap test: closed, non-empty boxes, IEEE f32 comparisons only, no arithmetic.  q overlaps b iff, for k = x, y, z,
 *   q.min.k <= b.max.k && b.min.k <= q.max.k && q.min.k <= q.max.k && b.min.k <= b.max.k.
 * Touching boxes (a shared face, edge or corner) overlap.  A NaN anywhere makes the test false.  An inverted box (a min above its max: the empty set, such as
 * the reset box) overlaps nothing — for boxes that are not inverted the last two comparisons hold and the test is the usual six.  -0 equals +0.
 * Answer: query i's set is every primitive whose leaf box overlaps d_boxes[i], in compressed-row form: d_prims[d_offsets[i] .. d_offsets[i+1]) is query i's
 * slice, d_offsets[0] = 0, d_offsets[n_boxes] = the total.  The set is exact for EVERY query and does not depend on the builder, the layout or the scheduler.
 * The order inside a slice is unspecified, but the same call on the same arrays gives the same bytes.  Each primitive appears at most once per slice.
 * Exactness condition: every internal box contains its children's boxes (then a box that a leaf's box passes is passed by every box above it).  All trees this
 * library produces satisfy it bitwise: an internal box is the fminf / fmaxf union of its children's.  On caller-filled trees that violate it every reported
 * primitive still overlaps its query, but some may be left out.  Arrays that are not a tree end in finite time with unspecified answers (d_prims is never
 * written outside query i's slice).  A child or primitive index out of range is never followed or reported.
 * BVH_OVERLAP_SELF: n_boxes must equal n_leaves; d_boxes[i] is taken as primitive i's box (typically tree->d_prim_aabbs) and only primitives j > i are
 * reported, so every unordered overlapping pair {i, j} appears exactly once, as j in i's slice, and no primitive pairs with itself.
 * Passes: the call always counts, then scans the counts into d_offsets, and keeps the 64-bit total in a device word.  It fills d_prims iff d_prims != NULL,
 * total <= capacity and total < 2^32; that decision is made ON THE DEVICE (the fill launch reads the total word and returns at once), so the call stays
 * asynchronous on the ctx's stream.  If the fill is skipped d_prims is not touched and d_offsets is still complete.  With total_out != NULL the call blocks on
 * an 8-byte read-back into pinned words and stores the total; a host that guessed too small a capacity re-allocates and calls again.  A total of 2^32 or more
 * saturates d_offsets at 0xFFFFFFFF; if total_out was given the call then returns BVH_E_TOO_LARGE (with *total_out set).
 * There is no depth limit: a query whose short stack would overflow is finished by a stackless pass through bvh_refit's parent plan, cached for the ctx's own
 * tree as for bvh_intersect and made per call for caller-owned arrays.  Count and fill agree on every query's set whichever pass served it.
 * Errors (nothing is written or enqueued, BVH_E_INVALID_ARG): NULL ctx / tree / d_boxes / d_offsets, n_leaves < 2, layout not 0 or 1, NULL d_nodes, layout 1
 * with NULL d_leaves, root not an internal node, mode not 0 or 1, BVH_OVERLAP_SELF with n_boxes != n_leaves, n_boxes >= 2^30, n_leaves larger than the ctx's
 * capacity (the parent plan lives in the arena; call bvh_ctx_reserve first), d_offsets or d_prims (capacity words) overlapping d_boxes or each other.
 * n_boxes == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.
 * bvh_ctx_kernel_times reports k_overlap_count, k_overlap_deep (after each pass), k_overlap_scan, k_overlap_fill and, when the plan is made, k_refit_plan. */
typedef enum { BVH_OVERLAP_BOXES = 0, BVH_OVERLAP_SELF = 1 } bvh_overlap_mode;
int  bvh_overlap(bvh_ctx* ctx, const bvh_result* tree, const bvh_aabb* d_boxes, uint32_t n_boxes, int mode /* bvh_overlap_mode */,
                 uint32_t* d_offsets /* u32[n_boxes + 1], device */, uint32_t* d_prims /* u32[capacity], device, or NULL: count only */,
                 uint64_t capacity, uint64_t* total_out /* host, may be NULL */);

/* ---- convex-volume and frustum queries (no counterpart in the reference) ---------------------------------------------------------------
 * Which primitives lie inside or across each convex volume?  View-frustum culling, the tile and cluster volumes of a light-culling pass, shadow cascades,
 * "which instances are in view" on a scene's top-level tree.  bvh_overlap with a frustum's bounding box answers a superset that the caller must filter; this
 * call takes the planes themselves.
 * tree: anything bvh_overlap accepts, read as it is — a build's, a refit's, an optimised one, a bvh_build_boxes tree, a bvh_scene_tlas result (the answers are
 * then instance indices), or caller-filled device arrays.  Only root, n_leaves, layout, d_nodes and d_leaves are read; no triangles are needed; nothing in the
 * tree is written.  A primitive's box is its leaf record's box, as in bvh_overlap.
 * Planes and volumes: d_planes[i][k] = (a, b, c, d) is plane k of volume i; its inside is a x + b y + c z + d >= 0; it need not be normalised.  A volume is the
 * intersection of its planes_per_volume (1 .. BVH_CULL_MAX_PLANES) half-spaces; a caller with fewer real planes pads with (0, 0, 0, 1).
 * The test, for a plane with n = (a, b, c) and a box [lo, hi] with lo.k <= hi.k on every axis (bvh_overlap's validity test), in IEEE f32:
 *   p-vertex: p.k = (n.k >= 0) ? hi.k : lo.k (so -0.0 selects hi); the n-vertex takes the other choice on every axis;
 *   s(v) = fadd(fadd(fadd(t(a, v.x), t(b, v.y)), t(c, v.z)), d), every product and sum ONE round-to-nearest f32 operation (never an FMA), with
 *   t(coef, x) = fmul(coef, x) for a coefficient that is not zero and a zero for a coefficient of +0 or -0, WHATEVER x is (never 0 * inf = NaN; the sign of
 *   that zero is not specified and cannot change an `s >= 0`): the padding plane and axis-aligned planes are immune to box planes at +-inf;
 *   the box passes the plane iff s(p) >= 0 — a NaN fails —, and passes the volume iff it passes every plane.  A NaN comes only from inf - inf between terms
 *   whose coefficients are not zero (a product that overflows against an infinite d, a box with infinite planes on two axes), or from a NaN in the input;
 *   bit k of straddle = !(s(n-vertex of plane k) >= 0): the box is not wholly inside plane k.  straddle == 0: the box lies wholly inside the volume (a
 *   renderer then skips clipping).  An invalid box (inverted, or with a NaN) passes nothing.
 * This is the standard conservative box test: a box beyond a corner or an edge of the volume can pass every plane without touching the volume.  That is the
 * defined answer, not an error.
 * Answer: volume i's slice d_hits[d_offsets[i] .. d_offsets[i+1]) holds one record per primitive whose leaf box passes volume i, with that leaf box's straddle
 * mask (always worked out from the leaf's own box against all planes); compressed rows as bvh_overlap's, d_offsets[0] = 0, d_offsets[n_volumes] = the total.
 * Each primitive appears at most once per slice.  The order inside a slice is unspecified, but the same call on the same arrays with the same path gives the
 * same bytes.
 * Exactness condition: every internal box contains its children's boxes — true bitwise of every tree this library makes —, and no evaluation of s produces a
 * NaN — true of finite planes whose products and sums do not overflow, on finite boxes and, for the terms with a zero coefficient, on boxes with infinite
 * planes as well (a mesh with one vertex at +inf is answered exactly by every volume of axis-aligned or padded planes).  The test is monotone under containment in rounded f32 (products by a fixed
 * factor and sums are monotone, and the p-vertex takes the larger coordinate of every product), so every box above a passing leaf passes: the set is exact for
 * EVERY volume and does not depend on the builder, the layout or the path.  Outside that condition every reported primitive still passes its own leaf test,
 * but some may be left out.  A walk may drop plane k below a node whose n-vertex has s >= 0 (s(n_parent) <= s(n_child) <= s(p_child)): result-preserving under
 * the same condition.  Arrays that are not a tree end in finite time with unspecified answers (d_hits is never written outside volume i's slice); a child or
 * primitive index out of range is never followed or reported.
 * path: BVH_CULL_LANE walks one volume per lane (thousands of small volumes); BVH_CULL_GROUP gives each volume a workgroup of 256 threads and a work stack of
 * BVH_CULL_GROUP_STACK node indices in LDS (one camera frustum on a large tree); BVH_CULL_AUTO takes the group walk iff n_volumes <= 65536 and n_leaves >= 1024.
 * The group walk's schedule is fixed: each round takes the m = min(top, 256) entries at the top of the stack, thread t entry top - m + t, tests both children,
 * and emits leaf survivors / pushes internal survivors in thread order, left child before right — so its slice bytes are deterministic too.
 * Passes, capacity, total_out, saturation and BVH_E_TOO_LARGE: bvh_overlap's, word for word.  The call always counts, then scans the counts into d_offsets, and
 * fills d_hits iff d_hits != NULL, total <= capacity and total < 2^32, decided ON THE DEVICE; if the fill is skipped d_hits is not touched and d_offsets is
 * still complete.  With total_out != NULL the call blocks on an 8-byte read-back.
 * There is no depth or size limit: a volume whose short stack (lane walk) or work stack (group walk) would overflow is finished by a stackless pass through
 * bvh_refit's parent plan, as in bvh_overlap.  Count and fill agree on every volume's set whichever walk served it.
 * Errors (nothing is written or enqueued, BVH_E_INVALID_ARG): NULL ctx / tree / d_planes / d_offsets, the tree errors of bvh_overlap, planes_per_volume
 * outside 1 .. 8, path outside 0 .. 2, n_volumes >= 2^30, n_leaves larger than the ctx's capacity (bvh_ctx_reserve first), d_offsets or d_hits (capacity
 * records) overlapping d_planes or each other.
 * n_volumes == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.
 * bvh_ctx_kernel_times reports k_cull_walk or k_cull_group (count and fill), k_cull_deep (after each pass), k_overlap_scan (the scan is bvh_overlap's) and,
 * when the plan is made, k_refit_plan. */
typedef struct { uint32_t prim; uint32_t straddle; } bvh_cull_hit;          /* 8 bytes */
typedef enum { BVH_CULL_AUTO = 0, BVH_CULL_LANE = 1, BVH_CULL_GROUP = 2 } bvh_cull_path;
#define BVH_CULL_MAX_PLANES   8
#define BVH_CULL_GROUP_STACK  8192       /* entries of the group walk's LDS work stack (32 KiB: four workgroups still fit a CU's 160 KiB) */
int  bvh_cull(bvh_ctx* ctx, const bvh_result* tree, const float* d_planes /* float[n_volumes][planes_per_volume][4], device */,
              uint32_t n_volumes, uint32_t planes_per_volume /* 1 .. 8 */, int path /* bvh_cull_path */,
              uint32_t* d_offsets /* u32[n_volumes + 1], device */, bvh_cull_hit* d_hits /* [capacity], device, or NULL: count only */,
              uint64_t capacity, uint64_t* total_out /* host, may be NULL */);

/* ---- crossing triangle pairs (no counterpart in the reference) ---------------------------------------------------------------------------
 * Which triangles of the tree does each triangle of another mesh cut — or, with BVH_TRIS_SELF, which triangles of the tree's own mesh cut each other?  Contact
 * detection, self-intersection checks before meshing or booleans, mesh validation before a winding-number field.  bvh_overlap's broad phase and the exact narrow
 * phase in one walk: no pair list goes through memory.
 * tree, tris: as for bvh_intersect (tris NULL: tree->d_tris is Triangle[n_leaves]); nothing in the tree is written.  queries: the other mesh's n_queries
 * triangles, device pointers, in any bvh_tri_format, independent of tris' (morton_bits is ignored); NULL with BVH_TRIS_SELF.
 * The predicate.  All arithmetic is IEEE f64 on the f32 coordinates widened exactly, without contraction or reassociation.
 *   orient(a, b, c, d), with ad = a - d, bd = b - d, cd = c - d:
 *     ad.x * (bd.y * cd.z - bd.z * cd.y)  +  ad.y * (bd.z * cd.x - bd.x * cd.z)  +  ad.z * (bd.x * cd.y - bd.y * cd.x),   the three terms summed left to right.
 *   edge_crosses(p, q; a, b, c), with sp = orient(a, b, c, p) and sq = orient(a, b, c, q), is true iff both
 *     (sp > 0 && sq < 0) || (sp < 0 && sq > 0), and
 *     orient(p, q, a, b), orient(p, q, b, c) and orient(p, q, c, a) are all > 0 or all < 0.
 *   proper(T) is true iff none of T's nine coordinates is a NaN and, with u = v2 - v1, w = v3 - v1, one of u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z,
 *     u.x * w.y - u.y * w.x is > 0 or < 0 (T has an area).
 *   crosses(X, Y) is true iff X and Y are proper and one of the 3 edges of X, taken as (v1, v2), (v2, v3), (v3, v1), crosses Y = (v1, v2, v3), or one of Y's
 *   crosses X.  Each plane side orient(a, b, c, p) is computed once per vertex with the arguments in exactly this order.
 * (The determinants alone would report an edge of a zero-area triangle, or an edge between the two clean vertices of a triangle whose third holds a NaN, that
 * passes through the other triangle's interior: such an edge is still a segment.  proper() is what keeps those two kinds out.)
 * The comparisons are strict, a zero row gives an exact 0 and a NaN compares false; so
 *   - only PROPER crossings are reported: an edge of one triangle passes through the interior of the other;
 *   - touching is not a crossing: a vertex or an edge lying in the other's plane or on its boundary;
 *   - coplanar overlap is not a crossing;
 *   - identical triangles, zero-area triangles and triangles with a NaN are not a crossing;
 *   - two triangles that share a vertex bitwise are reported only when an edge that does not contain the shared vertex crosses the other's interior;
 *   - two triangles that share an edge are never reported;
 *   - so a closed manifold mesh has an empty self set, without any adjacency test or index comparison, in all three triangle formats.
 * tests/test_intersect_tris.py restates the predicate in numpy f64 (bit for bit) and in exact rational arithmetic; on this project's meshes and on triangles
 * built to lie within an f32 ulp of touching the two agree on every pair.
 * Answer: the pair (query triangle i, tree primitive j) is reported iff box_overlap(B(i), leafbox(j)) — bvh_overlap's test; B(i) is stage E's box of query
 * triangle i (bvh_stage_extents_ex's expression, clamps against the reset box included), leafbox(j) the leaf record's box as bvh_overlap reads it — and
 * crosses(query_i, tri_j).  Compressed-row form, as bvh_overlap's: d_prims[d_offsets[i] .. d_offsets[i+1]) holds the tree primitives that query triangle i
 * crosses, i the query mesh's own triangle index; d_offsets[0] = 0, d_offsets[n_queries] = the total.  The order inside a slice is unspecified, but the same call
 * on the same arrays gives the same bytes.  The set does not depend on the builder, the layout or the scheduler.
 * Completeness condition: (1) every internal box contains its children's boxes — all of this library's trees satisfy that; (2) each leaf box is stage E's box
 * of the triangle passed for it — that holds for a build, and for a refit with the same triangles that are passed to the query.  Two triangles that cross share
 * a point, so their stage-E boxes overlap, and under (1) and (2) the walk reaches the pair.  On other arrays every reported pair still satisfies both tests,
 * but pairs may be missing.  Arrays that are not a tree end in finite time with unspecified answers (d_prims is never written outside query i's slice).  A
 * child or primitive index out of range is never followed or reported; a vertex index out of range reads vertex 0, as in bvh_build_ex.  On a tree relabelled by
 * bvh_remap_leaves (BVH_TRIS_QUERY only, see below) a pair can appear once per reference reached; this is not deduplicated.
 * BVH_TRIS_SELF: the queries are the tree's own triangles (tris), n_queries must equal n_leaves, and only j > i is reported: each unordered pair once, as j in
 * i's slice, and no triangle with itself.  The call reads triangle i of tris for EVERY i < n_leaves, so tris must hold n_leaves triangles (an indexed tris:
 * n_leaves index triples).  That is a requirement on the caller which the call cannot check: BVH_TRIS_SELF is NOT usable on a tree with more leaves than
 * triangles — a tree over bvh_split_refs references relabelled by bvh_remap_leaves — where it would read past the end of the triangle array.  For such a tree
 * pass the mesh itself as queries with BVH_TRIS_QUERY (the Python binding refuses self_pairs on a build_split tree).
 * Passes, capacity, total_out, saturation and BVH_E_TOO_LARGE: bvh_overlap's, word for word.  The call always counts, then scans the counts into d_offsets, and
 * keeps the 64-bit total in a device word.  It fills d_prims iff d_prims != NULL, total <= capacity and total < 2^32; that decision is made ON THE DEVICE (the
 * fill launch reads the total word and returns at once), so the call stays asynchronous on the ctx's stream.  If the fill is skipped d_prims is not touched
 * and d_offsets is still complete.  With total_out != NULL the call blocks on an 8-byte read-back into pinned words and stores the total.  A total of 2^32 or
 * more saturates d_offsets at 0xFFFFFFFF; if total_out was given the call then returns BVH_E_TOO_LARGE (with *total_out set).
 * There is no depth limit: a query whose short stack would overflow is finished by a stackless pass through bvh_refit's parent plan, cached for the ctx's own
 * tree as for bvh_overlap and made per call for caller-owned arrays.  Count and fill agree on every query's set whichever pass served it.
 * Errors (nothing is written or enqueued, BVH_E_INVALID_ARG): NULL ctx / tree / d_offsets, n_leaves < 2, layout not 0 or 1, NULL d_nodes, layout 1 with NULL
 * d_leaves, root not an internal node, no triangles (tris NULL and tree->d_tris NULL), a format error in tris or queries (an unknown tri_format, a NULL or — for
 * PACKED36 — misaligned d_tris, INDEXED with a NULL vertex or index pointer or n_vertices == 0), mode not 0 or 1, NULL queries without BVH_TRIS_SELF, queries
 * given with BVH_TRIS_SELF, BVH_TRIS_SELF with n_queries != n_leaves, n_queries >= 2^30, n_leaves larger than the ctx's capacity (the parent plan lives in the
 * arena; call bvh_ctx_reserve first), d_offsets or d_prims (capacity words) overlapping each other or a node, leaf, triangle, vertex or index array of the call.
 * n_queries == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.
 * bvh_ctx_kernel_times reports k_tris_count, k_tris_deep (after each pass), k_overlap_scan (the scan is bvh_overlap's), k_tris_fill and, when the plan is
 * made, k_refit_plan. */
typedef enum { BVH_TRIS_QUERY = 0, BVH_TRIS_SELF = 1 } bvh_tris_mode;
int  bvh_intersect_tris(bvh_ctx* ctx, const bvh_result* tree, const bvh_build_input* tris /* NULL: tree->d_tris is Triangle[n_leaves] */,
                        const bvh_build_input* queries /* the other mesh, device; any bvh_tri_format, independent of tris'; NULL with BVH_TRIS_SELF */,
                        uint32_t n_queries, int mode /* bvh_tris_mode */, uint32_t* d_offsets /* u32[n_queries + 1], device */,
                        uint32_t* d_prims /* u32[capacity], device, or NULL: count only */, uint64_t capacity, uint64_t* total_out /* host, may be NULL */);

/* ---- mesh-to-mesh distance (no counterpart in the reference) -----------------------------------------------------------------------------
 * Which triangle of the tree is nearest to each triangle of another mesh, and how far apart are the two (BVH_QUERY_CLOSEST) — or is any tree triangle within the
 * radius of it (BVH_QUERY_ANY)?  One bvh_tri_hit per query triangle: d_hits[i] answers triangle i of `queries`.  Clearance and tolerance checks between parts,
 * contact generation with a margin (bodies that do not touch yet have an empty bvh_intersect_tris set), penetration-free stepping, mesh-to-mesh distance for
 * registration.  bvh_closest_point on the other mesh's vertices misses every edge-edge and face-vertex minimum; this query does not.
 * tree / tris: exactly as bvh_closest_point — any bvh_result in either layout (a build's, a refit's, an optimised or a caller-filled one on the ctx's device),
 * triangles in any bvh_tri_format (NULL: tree->d_tris is read as Triangle[n_leaves]); nothing in the tree is written.  queries: as bvh_intersect_tris's with
 * BVH_TRIS_QUERY — the other mesh's n_queries triangles, device pointers, any bvh_tri_format, independent of tris' (morton_bits is ignored).
 * radius: ONE bound for the whole call; r2 = radius * radius in f32; +inf is no bound; a NaN or negative radius makes every query miss.
 * The candidate of a pair: X = the query triangle, Y = the tree triangle, vertices v1, v2, v3.  Everything is f32 without contraction except the crossing
 * test; every dot product is (x*x' + y*y') + z*z'; divisions are correctly rounded.  dist2(X, Y) and feature, in this order:
 *   0. NaN.  If one of Y's nine coordinates is a NaN, dist2 = NaN and feature = 0: never accepted.  (A query triangle with a NaN coordinate misses, below.)
 *   1. Crossing (feature 15).  If the stage-E boxes of X and Y overlap (bvh_overlap's box_overlap on bvh_stage_extents_ex's expression of either triangle,
 *      clamps included) and proper(X) && proper(Y) && crosses(X, Y) — bvh_intersect_tris's predicate word for word, IEEE f64 on the f32 coordinates — then
 *      dist2 = 0.0f and feature = 15.  Two triangles that cross share a point, which lies between the f32 minimum and maximum of either triangle's coordinates
 *      on every axis: their stage-E boxes overlap exactly, so skipping the determinants where the boxes are disjoint changes no answer.
 *   2. Vertices of X against Y (features 0, 1, 2): term k = tri_closest(Y.v1, Y.v2, Y.v3, X.v(k+1)), bvh_closest_point's formula word for word (its dist2).
 *   3. Vertices of Y against X (features 3, 4, 5): term 3 + k = tri_closest(X.v1, X.v2, X.v3, Y.v(k+1)).
 *   4. Edge i of X against edge j of Y (feature 6 + 3*i + j, i, j in 0..2), edges taken as (v1,v2), (v2,v3), (v3,v1): Ericson's ClosestPtSegmentSegment
 *      (Real-Time Collision Detection, 5.1.9) for the segments (p1, q1) of X and (p2, q2) of Y, operation for operation:
 *        d1 = q1 - p1;  d2 = q2 - p2;  r = p1 - p2;  a = dot(d1, d1);  e = dot(d2, d2);  f = dot(d2, r);   clamp(x) = x < 0 ? 0 : (x > 1 ? 1 : x)
 *        if (a <= 0 && e <= 0)  s = 0, t = 0;
 *        else if (a <= 0)       s = 0, t = clamp(f / e);
 *        else { c = dot(d1, r);
 *          if (e <= 0)          t = 0, s = clamp((-c) / a);
 *          else { b = dot(d1, d2);  denom = a*e - b*b;
 *                 s = denom != 0 ? clamp((b*f - c*e) / denom) : 0;
 *                 t = (b*s + f) / e;
 *                 if (t < 0)      t = 0, s = clamp((-c) / a);
 *                 else if (t > 1) t = 1, s = clamp((b - c) / a); } }
 *        w_k = (p1_k + d1_k*s) - (p2_k + d2_k*t);   term = (w.x*w.x + w.y*w.y) + w.z*w.z
 *      (the book's EPSILON tests as exact tests against 0; a NaN passes through clamp).
 *   Without a crossing, dist2 = the smallest of the 15 terms and feature = the LOWEST index that attains it: the minimum starts at +inf with feature 0 and a
 *   term replaces it only when it is strictly smaller, in index order, so a NaN term never wins (if no term is below +inf, dist2 = +inf, feature 0).
 * The 15 terms cover every closest pair of two disjoint triangles (the minimum is attained at a vertex of one, or between two edges); where two edges are nearly
 * parallel and the segment formula's denom is weak, the end points' vertex terms hold the minimum.  Touching and coplanar overlap give a zero (or
 * rounding-sized) vertex or edge term; only a proper crossing, whose 15 terms can all be positive, needs step 1.  `feature` lets a caller recompute the witness
 * points with one evaluation of the stated term; the points themselves are not returned.
 * Acceptance and answer: bvh_closest_point's, word for word.  A candidate is accepted iff dist2 <= r2.  BVH_QUERY_CLOSEST: the accepted candidate with the
 * smallest (dist2, prim_idx), compared lexicographically — independent of the builder, the layout, the formats and the traversal order.  BVH_QUERY_ANY: some
 * accepted candidate (the walk stops at the first); its record is that candidate's full dist2(X, Y) and feature.  A hit is written as {dist2, prim_idx, feature,
 * 0}; a miss as {r2, BVH_INVALID, 0, 0}.  A query triangle with a NaN coordinate misses.  Degenerate query or tree triangles (points, segments) are ordinary
 * candidates of steps 2-4; they cross nothing.
 * Box tests are conservative: every node box grows on every axis by 2^-16 times its largest |coordinate|, the query triangle's stage-E box once
 * the same way; the per-axis gap is fmaxf(fmaxf(lo_b - hi_q, lo_q - hi_b), 0) (a NaN plane is dropped), lb = (gx*gx + gy*gy) + gz*gz, and a subtree is kept
 * iff lb * (1 - 2^-20) <= the best dist2 so far (r2 at the start).  A leaf pair whose own two stage-E boxes fail the same test is skipped.  Answers are exact
 * on well-conditioned queries: the f64 squared distance between the two stage-E boxes of the true answer's pair, each grown by 2^-17 times its largest
 * |coordinate|, is <= that answer's dist2.  On every query a reported hit is an accepted candidate of its prim with exactly its dist2 and feature, and a closest
 * answer is never below the true best.
 * Errors (nothing is written or enqueued, BVH_E_INVALID_ARG): bvh_closest_point's (NULL ctx / tree / d_hits, n_leaves < 2, layout not 0 or 1, NULL d_nodes,
 * layout 1 with NULL d_leaves, root not an internal node, no triangles or a tris format error, query not 0 or 1, n_leaves larger than the ctx's capacity), NULL
 * queries or a format error in it, n_queries >= 2^30, d_hits overlapping any node, leaf, triangle, vertex or index array of the call, the queries' included.
 * n_queries == 0: 0, nothing is touched.
 * Asynchronous on the ctx's stream, no read-back.  There is no depth limit: queries whose short stack would overflow are finished by a stackless pass through
 * bvh_refit's parent plan, cached for the ctx's own tree and made per call for caller-owned arrays.  bvh_ctx_kernel_times reports k_closest_tris,
 * k_closest_tris_deep and, when the plan is made, k_refit_plan. */
int  bvh_closest_tris(bvh_ctx* ctx, const bvh_result* tree, const bvh_build_input* tris /* NULL: tree->d_tris is Triangle[n_leaves] */,
                      const bvh_build_input* queries /* the other mesh, device; any bvh_tri_format, independent of tris' */, uint32_t n_queries,
                      float radius, bvh_tri_hit* d_hits /* [n_queries], device */, int query /* bvh_query_kind */);

/* ---- every triangle within a radius, mesh to mesh (no counterpart in the reference) ------------------------------------------------------
 * Which triangles of the tree lie within the radius of each triangle of another mesh, ALL of them, how far away, and between which two features — or, with
 * BVH_RADIUS_TRIS_SELF, which pairs of the tree's own mesh?  The third proximity answer of the triangle queries, beside bvh_intersect_tris (every crossing
 * pair) and bvh_closest_tris (the one nearest): cloth and shell contact with a thickness, barrier and penalty methods that need every vertex-face and
 * edge-edge pair closer than a distance, clearance reports that list every violating pair, proximity constraints between parts.  One walk instead of
 * bvh_overlap with inflated boxes and an exact filter on the host, which sends the whole box-pair list through memory.
 * tree / tris / queries: exactly as bvh_closest_tris — any bvh_result in either layout (a build's, a refit's, an optimised or a caller-filled one on the ctx's
 * device), triangles in any bvh_tri_format (NULL: tree->d_tris is read as Triangle[n_leaves]); nothing in the tree is written.  queries: the other mesh's
 * n_queries triangles, device pointers, any bvh_tri_format, independent of tris' (morton_bits is ignored); NULL with BVH_RADIUS_TRIS_SELF.
 * Candidate: dist2(X, Y) and feature are bvh_closest_tris's, steps 0-4 word for word, X = the query triangle, Y = the tree triangle (one device function
 * serves both calls).
 * Acceptance: dist2 <= r2, r2 = radius * radius in f32; radius is ONE bound for the whole call.  An infinite radius accepts every pair whose dist2 is not NaN
 * (a tree triangle with a NaN vertex is never accepted).  A NaN or negative radius makes every query dead, and so does a NaN coordinate in the query triangle:
 * a dead query accepts nothing.  radius 0 (or -0) accepts the pairs at dist2 == 0, proper crossings (feature 15) among them.
 * Answer: query triangle i's set is ALL its accepted candidates, as {dist2, prim_idx, feature, 0} records (bvh_tri_hit) in compressed-row form, as
 * bvh_radius_search's: d_hits[d_offsets[i] .. d_offsets[i+1]) is query i's slice, d_offsets[0] = 0, d_offsets[n_queries] = the total.  Each primitive appears
 * at most once per slice.  There is no padding and there are no miss records: an empty slice is "nothing within r".  With d_hits == NULL the call only counts:
 * d_offsets is then the queries' partner counts in scanned form.
 * Order inside a slice: without BVH_RADIUS_TRIS_SORTED unspecified, but the same call on the same arrays gives the same bytes.  With BVH_RADIUS_TRIS_SORTED
 * each slice is in ascending (dist2, prim_idx) order, compared lexicographically (an accepted dist2 is never NaN or negative); the whole d_hits array then does
 * not depend on the builder, the layout, the scheduler, the triangle formats or the traversal order, and the first record of a non-empty slice is
 * bvh_closest_tris(BVH_QUERY_CLOSEST)'s record for the same radius, bit for bit.  The sorted fill inserts each record into its slice as it is found, which is
 * quadratic in the slice's length: very long sorted slices (thousands of partners per query) are the caller's to avoid, or to fill unsorted and sort themselves.
 * Box tests are bvh_closest_tris's conservative test (every node box grows on every axis by 2^-16 times its largest |coordinate|, the query
 * triangle's stage-E box once the same way, lb = the f32 sum of the squared per-axis gaps, the subtree is kept iff lb * (1 - 2^-20) <= the bound) against r2
 * for the whole walk: the bound never shrinks.  A leaf pair whose own two stage-E boxes fail the same test is skipped before any term is computed.  A query is
 * well-conditioned when every accepted pair satisfies bvh_closest_tris's condition: the f64 squared distance between the pair's two stage-E boxes, each grown by
 * 2^-17 times its largest |coordinate|, is <= the pair's dist2.  On such queries no ancestor of an accepted triangle is culled and the set is exact (DESIGN.md
 * 8z).  On EVERY query each reported record is an accepted candidate of its primitive with a bit-equal dist2 and feature, and the slice is a subset of the true
 * set.
 * BVH_RADIUS_TRIS_SELF: the queries are the tree's own triangles (tris), queries must be NULL, n_queries must equal n_leaves, and only j > i is reported: each
 * unordered pair once, as j in i's slice, and no triangle with itself.  The call reads triangle i of tris for EVERY i < n_leaves, so tris must hold n_leaves
 * triangles: as BVH_TRIS_SELF, it is NOT usable on a tree with more leaves than triangles (a tree over bvh_split_refs references relabelled by
 * bvh_remap_leaves); pass the mesh itself as queries there (the Python binding refuses self_pairs on a build_split tree).  On such a tree a pair can appear
 * once per reference reached; this is not deduplicated.
 * BVH_RADIUS_TRIS_SKIP_SHARED (only together with SELF): on one mesh every topological neighbour is at distance 0, which is not contact.  A pair is skipped
 * when any vertex of X equals any vertex of Y on all three coordinates under IEEE == — so -0 equals +0 and a NaN equals nothing.  No adjacency input and no
 * index comparison: it works in all three triangle formats.  It is evaluated at the leaf before the terms, identically in count and fill.
 * Passes: the call always counts, then scans the counts into d_offsets, and keeps the 64-bit total in a device word.  It fills d_hits iff d_hits != NULL,
 * total <= capacity and total < 2^32; that decision is made ON THE DEVICE (the fill launch reads the total word and returns at once), so the call stays
 * asynchronous on the ctx's stream.  If the fill is skipped d_hits is not touched and d_offsets is still complete.  With total_out != NULL the call blocks on
 * an 8-byte read-back into pinned words and stores the total; a host that guessed too small a capacity re-allocates and calls again.  A total of 2^32 or more
 * saturates d_offsets at 0xFFFFFFFF; if total_out was given the call then returns BVH_E_TOO_LARGE (with *total_out set).  d_hits is never written outside
 * query i's slice, nor past the total.
 * There is no depth limit: a query whose short stack would overflow, or whose walk exceeds the node count, is redone by a stackless pass through bvh_refit's
 * parent plan, cached for the ctx's own tree as for bvh_intersect and made per call for caller-owned arrays.  Count and fill agree on every query's set
 * whichever pass served it.
 * Errors (nothing is written or enqueued, BVH_E_INVALID_ARG): bvh_closest_tris's without the query kind (NULL ctx / tree, n_leaves < 2, layout not 0 or 1,
 * NULL d_nodes, layout 1 with NULL d_leaves, root not an internal node, no triangles or a tris format error, a format error in queries, n_leaves larger than the
 * ctx's capacity: call bvh_ctx_reserve first); NULL d_offsets; a flag bit other than the three below; BVH_RADIUS_TRIS_SKIP_SHARED without BVH_RADIUS_TRIS_SELF;
 * NULL queries without BVH_RADIUS_TRIS_SELF; queries given with BVH_RADIUS_TRIS_SELF; BVH_RADIUS_TRIS_SELF with n_queries != n_leaves; n_queries >= 2^30;
 * d_offsets or d_hits (capacity records) overlapping each other or a node, leaf, triangle, vertex or index array of the call.
 * n_queries == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.
 * bvh_ctx_kernel_times reports k_radius_tris_walk (count and fill), k_radius_tris_deep (after each pass), k_overlap_scan (the scan is bvh_overlap's) and, when
 * the plan is made, k_refit_plan. */
#define BVH_RADIUS_TRIS_SORTED       1u
#define BVH_RADIUS_TRIS_SELF         2u
#define BVH_RADIUS_TRIS_SKIP_SHARED  4u   /* only together with BVH_RADIUS_TRIS_SELF */
int  bvh_radius_tris(bvh_ctx* ctx, const bvh_result* tree, const bvh_build_input* tris /* NULL: tree->d_tris is Triangle[n_leaves] */,
                     const bvh_build_input* queries /* the other mesh, device; any bvh_tri_format, independent of tris'; NULL with BVH_RADIUS_TRIS_SELF */,
                     uint32_t n_queries, float radius, uint32_t flags /* BVH_RADIUS_TRIS_* */, uint32_t* d_offsets /* u32[n_queries + 1], device */,
                     bvh_tri_hit* d_hits /* [capacity], device, or NULL: count only */, uint64_t capacity, uint64_t* total_out /* host, may be NULL */);

/* ---- early split clipping (Utility::doEarlySplitClipping, src/Utility.cpp:456-538: the PrimRef[] front end of the reference's LBVH builders) -------------
 * Large triangles become several REFERENCES {box, triangle index}: a box whose surface area exceeds sa_max is halved at its centre on its longest axis until
 * every piece is small enough, and the tree is then built over the pieces (bvh_build_boxes), so a wall that spans the scene no longer owns a scene-sized leaf.
 * Several leaves refer to one triangle.  The reference does this on the host, one queue item at a time; here it is a count -> scan -> fill device pass.
 * Input: any bvh_tri_format (in->morton_bits is not read), n triangles, device pointers.
 * Root box: triangle p's root box is exactly the box stage E writes for it (bvh_stage_extents_ex; the same device function), NaN / infinity clamping included;
 * for finite triangles that is the reference's Aabb::grow of the three vertices.
 * refs(box, depth) — f32 throughout, operation for operation, no contraction; ext = max - min:
 *   area = 2 * (ext.x * ext.y + ext.x * ext.z + ext.y * ext.z)                     (Aabb::area, src/Common.h:361-365, same association)
 *   dim  = 0 if ext.x > ext.y && ext.x > ext.z, else 1 if ext.y > ext.z, else 2    (Aabb::maximumExtentDim, :351-359)
 *   c    = (max[dim] + min[dim]) * 0.5f                                            (Aabb::center, :347)
 *   EMIT the box as one reference if !(area > sa_max) (a NaN area emits at once), or depth == max_depth, or !(min[dim] < c && c < max[dim]) (the cut would make
 *   no progress); OTHERWISE L = the box with max[dim] = c, R = the box with min[dim] = c, and the result is refs(L, depth + 1) followed by refs(R, depth + 1).
 *   The last two emit rules are this library's: the reference has neither and does not terminate where they would fire.  Where neither fires the set of
 *   references equals the reference's (tests/golden/split_*.primref), which it produces in breadth-first order.
 * Output order (canonical): triangles in index order, and within a triangle the depth-first, left-first order above.  d_ref_boxes[d_offsets[p] ..
 * d_offsets[p+1]) are triangle p's references and d_ref_prims holds p there; d_offsets[0] = 0, d_offsets[n] = the total.  The bytes depend neither on the
 * triangle format nor on which internal path served a triangle (one lane per triangle, or one wave for a triangle with more than 64 references), and are the same
 * on every call.  A triangle has at most 2^max_depth references.
 * Passes: the call always counts, scans the counts into d_offsets and keeps the 64-bit total in a device word.  It fills iff both output pointers are non-NULL,
 * total <= capacity and total < 2^32; that decision is made ON THE DEVICE, so the call stays asynchronous on the ctx's stream.  If the fill is skipped the output
 * arrays are not touched and d_offsets is still complete.  With total_out != NULL the call blocks on an 8-byte read-back and stores the total; a total of 2^32 or
 * more saturates d_offsets at 0xFFFFFFFF and the call then returns BVH_E_TOO_LARGE (with *total_out set).
 * Identity: max_depth == 0 gives one reference per triangle — stage E's boxes and prims 0 .. n-1 — and so does sa_max = FLT_MAX for finite triangles (the
 * reference's default saMax).  bvh_build_boxes over that output is byte-identical to bvh_build_ex on the triangles.
 * Errors (nothing is written or enqueued, BVH_E_INVALID_ARG): NULL ctx / in / d_offsets, an input format error as in bvh_build_ex, n == 0 or n >= 2^30, sa_max
 * NaN or < 0, max_depth > BVH_SPLIT_MAX_DEPTH, exactly one of d_ref_boxes / d_ref_prims NULL, output ranges (capacity records) that overlap each other,
 * d_offsets or the input arrays.
 * Memory: the ctx keeps 4 bytes per triangle plus 8 KiB outside the arena (the list of wave-filled triangles, the scan's sums, the total word), grown when n
 * grows; the arena and every bvh_result in it are untouched.  bvh_ctx_kernel_times reports k_split_count, k_overlap_scan, k_split_fill and k_split_heavy.
 *
 * bvh_remap_leaves: every leaf's primitive index q becomes d_map[q] (layout 0: nodes[n-1+j].left; layout 1: d_leaves[j].prim_idx); a q >= n_map stays as it
 * is; nothing else is written.  After bvh_build_boxes over d_ref_boxes, d_map = d_ref_prims makes the leaves name the ORIGINAL triangles.  Topology and boxes
 * are untouched, so the ctx's cached parent plan stays valid; the cached leaf map of bvh_refit_subset is dropped.  Asynchronous on the ctx's stream.
 * Errors (nothing written, BVH_E_INVALID_ARG): NULL ctx / io / d_map, a tree bvh_refit would reject, d_map (n_map words) overlapping the leaf records.
 * Who accepts a relabelled tree (n_leaves references, primitive indices below the triangle count, several leaves per triangle) — always pass the ORIGINAL
 * triangles explicitly as `tris` (the tree's own d_tris is NULL after bvh_build_boxes):
 *   bvh_intersect, bvh_closest_point: answers as on the unsplit tree.  Records are ordered by (t, prim) / (dist2, prim) and a triangle reached through two leaves
 *     gives the same record twice, so the answer does not change; a primitive index is only followed while it is < n_leaves, which every triangle index is.
 *     Conservative culling carries over: a triangle's references tile its root box with closed halves.
 *   bvh_scene_build: as a BLAS, with the original triangles as bvh_blas.tris.  bvh_download, bvh_checksum, bvh_to_lbvh_layout, bvh_trace (with the original
 *     Triangle array), bvh_collapse4: read the arrays as any tree.
 *   bvh_intersect_all, bvh_knn, bvh_radius_search, bvh_overlap: valid, but they report a triangle ONCE PER REFERENCE REACHED (duplicates within a slice; a
 *     bvh_knn list can fill with one triangle's references).  BVH_OVERLAP_SELF compares reference positions before and triangle indices after a relabelling;
 *     run it before.
 *   bvh_intersect_tris: BVH_TRIS_QUERY is valid after the relabelling, with the original triangles as `tris`, and likewise reports a triangle once per
 *     reference reached; deduplicated, the set equals the unsplit tree's (a crossing point lies in one of the references, which tile the triangle's box).
 *     BVH_TRIS_SELF is NOT valid on such a tree, before or after: it reads triangle i of `tris` for every i < n_leaves, and there are fewer triangles.
 *   bvh_sah_cost needs nothing but the tree and may run at any time; bvh_optimize likewise (it moves no leaf).  bvh_bvh4_cost indexes d_prim_aabbs by the
 *     leaves' primitive index: run it BEFORE the relabelling, while d_prim_aabbs (the reference boxes) still matches the leaves.
 *   bvh_refit, bvh_refit_ex, bvh_refit_subset: NOT applicable to a tree over references, relabelled or not — they would read Triangle[n_leaves] and give leaf j
 *     the whole box of triangle j.  After the triangles move, split and build again. */
#define BVH_SPLIT_MAX_DEPTH 16
int  bvh_split_refs(bvh_ctx* ctx, const bvh_build_input* in, uint32_t n, float sa_max, uint32_t max_depth /* 0 .. BVH_SPLIT_MAX_DEPTH */,
                    uint32_t* d_offsets /* u32[n + 1], device */, bvh_aabb* d_ref_boxes /* [capacity], device, or NULL: count only */,
                    uint32_t* d_ref_prims /* u32[capacity], device, or NULL: count only */, uint64_t capacity, uint64_t* total_out /* host, may be NULL */);
int  bvh_remap_leaves(bvh_ctx* ctx, bvh_result* io, const uint32_t* d_map /* u32[n_map], device */, uint32_t n_map);

/* ---- tree optimisation (no counterpart in the reference) ---------------------------------------------------------------------------------
 * Lower a built tree's SAH by treelet restructuring (Karras & Aila, HPG 2013): bottom-up, every treelet of 7 entries whose root holds enough leaves is replaced
 * by its SAH-optimal topology over the same entries.  The fast LBVH builds come out close to HPLOC quality; PLOC++ / HPLOC trees gain a few percent.
 * io: any tree bvh_refit / bvh_intersect accept — a result of bvh_build / bvh_build_ex / bvh_refit / bvh_optimize on this ctx, or a caller-filled bvh_result of
 * device arrays on the ctx's device.  Read: root, n_leaves, layout, d_nodes, d_leaves.  Written in place: only the child links and boxes of internal nodes
 * [0, n-1).  Not written: leaf records (layout 0: nodes n-1 .. 2n-2; layout 1: d_leaves), root, d_prim_aabbs, d_scene_extent, d_sorted_*, d_morton_keys,
 * d_tris.  The set of internal node indices is unchanged; the root's box keeps its value.  After an optimise an LBVH-layout internal node no longer
 * corresponds to a split position of d_sorted_keys.
 * Algorithm (f32 throughout, area = Aabb::area without contraction, unions fminf / fmaxf, comparisons IEEE <).  Round r = 0 .. rounds-1,
 * gamma = 7 << r; a node is processed after every internal node of its subtree; an internal node N whose subtree holds >= gamma leaves is a treelet root:
 *   formation: T = [left(N), right(N)]; while |T| < 7, the internal entry of T with the largest stored-box area (the first internal entry starts the scan, a
 *     later one wins only if strictly larger: ties go to the earliest position) is replaced in place by its left child and its right child is appended; the
 *     picked nodes are E (expansion order).
 *   current cost: c_cur(x) = area(x) + (c_cur(left x) + c_cur(right x)) over N and E, 0 for the entries of T.
 *   DP over the subsets S of {0..6}: B(S) = union of the entries' boxes in increasing bit order; c(S) = 0 for a singleton, else area(B(S)) + the smallest
 *     c(P) + c(S \ P) over the proper subsets P of S that hold S's lowest bit, in increasing mask order (the first P starts, a later one wins only if strictly smaller).
 *   decision: restructure iff c(all) < c_cur(N) — NaN or infinite costs keep the treelet byte for byte.
 *   rebuild: preorder from N (which keeps its index and its box); for the recorded partition {P, Q = S \ P}, P first, a singleton is its entry and a larger
 *     subset takes the next unused index of E in ascending order; node = {left = node(P), right = node(Q), box B(S)}.
 * What a treelet becomes depends only on its subtree, which is final when its root is processed: the result does not depend on scheduling, and a tree's SAH
 * never rises.  Trees with fewer than 7 leaves come back unchanged.  With NaN boxes the output is still a tree over the same leaves.
 * rounds: 1 .. 8 (3 is the usual choice).  timings: optional, sampled as for a build; ms_build = the optimise, the other stage times are 0; bvh_ctx_kernel_times
 * reports k_optimize (one launch per round whose gamma is <= n_leaves) and, when the parent plan is made, k_refit_plan.
 * The ctx's own tree keeps the parent plan of bvh_refit / bvh_intersect valid (the rounds rewrite parent[] as they move nodes); caller-owned arrays get a new
 * plan on every call.  A later bvh_refit refits the new topology; bvh_intersect closest hits do not change; bvh_collapse4, bvh_to_lbvh_layout, bvh_sah_cost
 * and bvh_checksum read the result as any tree.
 * Errors (nothing is written or enqueued): NULL ctx / io, n_leaves < 2, layout not 0 or 1, NULL d_nodes, layout 1 with NULL d_leaves, root not an internal
 * node, rounds outside [1, 8]: BVH_E_INVALID_ARG.  n_leaves larger than the ctx's capacity: BVH_E_INVALID_ARG — an optimise never re-allocates the arena (io
 * may point into it); call bvh_ctx_reserve first.  Asynchronous on the ctx's stream, except for what the timings need. */
int  bvh_optimize(bvh_ctx* ctx, bvh_result* io, uint32_t rounds, bvh_timings* timings /* may be NULL */);

/* ---- instanced scenes (two levels; no counterpart in the reference beyond one Transformation, src/Common.h:541-548) ------------------------------------
 * A scene places bottom-level trees (BLASes) by 3x4 transforms (bvh_instance) under a top-level tree over the instances' world boxes, and answers ray queries
 * against all of them: the same mesh placed many times is stored once, and moving an instance costs a refit of the top-level tree, not a rebuild.
 * Bottom level: bvh_blas = a tree (any bvh_result bvh_intersect accepts, either layout) + its triangles (any bvh_tri_format; tri_format PADDED64 with d_tris
 * NULL reads tree.d_tris as Triangle[n_leaves]).  Arrays are REFERENCED, not copied: they must stay valid and keep their topology while the scene is used.
 * Ordering: the scene reads a BLAS's arrays on ITS ctx's stream (bvh_scene_build: the plan and the root box; bvh_scene_update: the root box; queries: everything),
 * and nothing orders those reads after work enqueued on other streams.  All work that writes a BLAS's arrays (its build, bvh_refit, bvh_optimize, copies) must
 * be complete before bvh_scene_build, bvh_scene_update and bvh_scene_intersect are called — e.g. bvh_ctx_synchronize on the ctx that built or refit it.
 * Ownership: a scene is bound to one ctx and enqueues on its stream.  It owns device memory (outside the ctx's arena) for the BLAS table (device copies of the
 * descriptors), the instance array, the per-instance world-to-object matrices and world boxes, the top-level tree's nodes and leaves, and the parent plans
 * (k_refit_plan, 4 bytes x (2n-1) per tree, the top level and every BLAS) of the stackless pass: scene queries have no depth limit at either level.  The top-level
 * tree is built in the ctx's arena with bvh_build_boxes and copied out, so bvh_scene_build counts as a build on the ctx: it invalidates earlier bvh_results that
 * point into the arena.  Scenes stay valid across later builds on the ctx.  Destroy scenes before their ctx.
 * A BLAS whose d_nodes, d_leaves or triangle arrays overlap the scene's ctx's arena or its triangle staging buffer (what bvh_build of a host input copies to) is
 * rejected (BVH_E_INVALID_ARG): the scene build would overwrite it.  Build BLASes on other contexts, keep bvh_batch trees (their triangles uploaded by the caller),
 * or copy them out with bvh_dev_copy.
 * Instance maths (f32 unless stated, no contraction; tests/test_scene.py restates it in numpy):
 *   world_to_object = inverse of M = [A | t]: in f64 from the f32 entries, a_ij = M[4i + j]; cofactors c00 = a11 a22 - a12 a21, c01 = a12 a20 - a10 a22,
 *     c02 = a10 a21 - a11 a20; det = (a00 c00 + a01 c01) + a02 c02; A^-1 = adj(A) / det with adj row 0 = {c00, a02 a21 - a01 a22, a01 a12 - a02 a11},
 *     row 1 = {c01, a00 a22 - a02 a20, a02 a10 - a00 a12}, row 2 = {c02, a01 a20 - a00 a21, a00 a11 - a01 a10} (each entry divided by det); translation
 *     w_i3 = -((A^-1_i0 t0 + A^-1_i1 t1) + A^-1_i2 t2) with the unrounded f64 A^-1; every entry then rounded once to f32.
 *   object-space ray: o'_i = ((w_i0 ox + w_i1 oy) + w_i2 oz) + w_i3, d'_i = (w_i0 dx + w_i1 dy) + w_i2 dz; tmin / tmax unchanged.  d' is not normalised: t means
 *     the same in both frames and is compared across instances.
 *   world box: componentwise fminf / fmaxf over the 8 corners of the BLAS root box (nodes[root].aabb in both layouts; corner k takes max x if k & 1, max y if
 *     k & 2, max z if k & 4), each mapped by M in the order of o'.
 *   inactive instance: blas >= n_blas, a non-finite entry of M, det 0 or not finite, or a non-finite rounded inverse entry.  Its world box is the reset box
 *     {+FLT_MAX, -FLT_MAX}; it is never hit.
 * n_instances == 1 is supported: there is no top-level tree (bvh_scene_tlas reports n_leaves = 1 and d_nodes = NULL); a query tests the instance's world box
 * and enters it.  With n_instances >= 2 the top-level tree is built by any algo.
 * Queries: bvh_intersect's hit test (tri_hit, same acceptance rule) on the object-space ray.  BVH_QUERY_CLOSEST: the accepted hit with the smallest
 * (t, instance_idx, prim_idx), compared lexicographically — independent of the top-level builder, the BLAS builders, layouts and formats, and traversal order.
 * BVH_QUERY_ANY: some accepted hit.  Hit = {t, u, v, prim_idx, instance_idx, 0, 0, 0}; miss = {tmax, 0, 0, BVH_INVALID, BVH_INVALID, 0, 0, 0}; NaN rays and rays
 * with !(tmin < tmax) miss.  Box tests are bvh_intersect's at both levels.  Well-conditioned (answers exact): the object-space ray is
 * well-conditioned for its BLAS (§8b), and every accepted hit's world point o + t d (f64) lies in its instance's world box grown by half the box test's growth.
 * Asynchronous on the ctx's stream, no read-back.  bvh_ctx_kernel_times reports k_scene_intersect and k_scene_intersect_deep.
 * Errors write nothing (BVH_E_INVALID_ARG): bvh_intersect's checks, a NULL or unbuilt scene, overlapping d_rays / d_hits ranges.  n_rays == 0: nothing is touched.
 * Update: bvh_scene_update takes n_instances records as the build did; every field may change, blas included.  It recomputes the inverses and world boxes from the
 * BLAS root boxes as they are now (bvh_refit a BLAS, then update: correct) and refits the top-level tree in place (k_refit_climb), topology kept.  A BLAS whose
 * topology changed (a rebuild, bvh_optimize) needs a new bvh_scene_build: its parent plan is stale.  Asynchronous with device instances; host instances are
 * read before the call returns.
 * bvh_scene_build: blas[n_blas] host descriptors (n_blas >= 1), instances[n_instances] (1 <= n_instances < 2^30) on the host or (instances_on_device) the device.
 * Errors (BVH_E_INVALID_ARG, the scene unchanged): NULL arguments, algo out of range, a BLAS bvh_intersect would reject, a BLAS in the ctx's arena.  A HIP error
 * after validation leaves the scene unbuilt (queries and updates then return BVH_E_INVALID_ARG until a build succeeds).  timings: the top-level build's
 * (bvh_build_boxes; all zero with one instance).  Blocking (the descriptors are copied from host memory before any kernel is enqueued).
 * bvh_scene_tlas: the top-level tree as a bvh_result — layout by algo, d_prim_aabbs = the world boxes by instance index, d_tris / d_scene_extent / d_sorted_* /
 * d_morton_keys NULL — readable by bvh_sah_cost, bvh_checksum and bvh_download (nodes and leaves).  Valid until the next bvh_scene_build or bvh_scene_destroy.
 * Point queries: bvh_scene_closest_point answers d_points[i] (bvh_point_query, as bvh_closest_point reads it) with d_hits[i]: the nearest surface point over
 * all active instances, in world space.  Everything is f32 with no contraction in the stated order (tests/test_scene_point.py restates it in numpy).
 *   candidate of (instance k, primitive j): the world triangle V_i = M_k v_i, V_i.r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 (the order of the world box), and
 *     bvh_closest_point's formula tri_closest(V1, V2, V3, p) word for word: point and dist2 are world-space values that do not depend on how the tree is walked.
 *     Accepted iff dist2 <= r2 = radius * radius (NaN never; an infinite radius is no bound).  Queries with a NaN coordinate, a NaN radius or radius < 0 miss.
 *     Inactive instances never answer.
 *   BVH_QUERY_CLOSEST: the accepted candidate with the smallest (dist2, instance_idx, prim_idx), compared lexicographically.  BVH_QUERY_ANY: some accepted
 *     candidate (the walk stops at the first).  Hit = {point, dist2, u, v, prim_idx, instance_idx}; miss = {0, 0, 0, r2, 0, 0, BVH_INVALID, BVH_INVALID}.
 *   scale bound s2 of an instance (0 if inactive; recomputed by bvh_scene_update): from the rounded f32 world_to_object entries w_ij taken as f64,
 *     S_ij = (w_i0 w_j0 + w_i1 w_j1) + w_i2 w_j2, lambda = max_i (|S_i0| + |S_i1|) + |S_i2|, s2 = (float)((1 - 2^-10) / lambda).  lambda >= sigma_max(W)^2
 *     (Gershgorin), so |M x - p|^2 >= s2 |x - W p|^2 for every object point x: tight for rotation x uniform scale, within 3x otherwise.
 *   box tests.  Top level: bvh_closest_point's (box_dist_pass) on the instances' world boxes with the world point.  Inside instance k: the point
 *     p' = W_k p in the order of o' above, the slack e = 2^-20 max_i(((|w_i0||px| + |w_i1||py|) + |w_i2||pz|) + |w_i3|); a node box grows on every axis by
 *     2^-16 * (its largest |coordinate|) + e, lb' is its f32 squared distance to p' as in box_dist_pass, and the subtree is culled iff
 *     s2 * lb' * (1 - 2^-20) > best (a NaN product never culls), best being the world-space dist2 so far (r2 at the start), carried across instances.
 *   well-conditioned (answers exact): for the true answer (k, j), (1) with p* = W_k p in f64 from the stored f32 entries, s2_k times the f64
 *     squared distance from p* to triangle j's object box grown by 2^-17 * (its largest |coordinate|) + e / 2 is <= the answer's dist2, and (2) the f64 squared
 *     distance from p to instance k's world box grown by 2^-17 * (its largest |coordinate|) is <= that dist2.  On every query a reported hit is an accepted
 *     candidate of its (instance, prim) with bit-equal point, dist2, u, v, and a closest answer is never lexicographically below the true one.
 * Asynchronous on the ctx's stream, no read-back; no depth limit at either level.  bvh_ctx_kernel_times reports k_scene_closest_point and
 * k_scene_closest_point_deep.  Errors write and enqueue nothing (BVH_E_INVALID_ARG): a NULL or unbuilt scene, NULL d_points or d_hits, a query other than 0 or 1,
 * overlapping d_points / d_hits ranges.  n_points == 0 returns 0 and touches nothing.  BLAS ordering as for bvh_scene_intersect.
 * k nearest: bvh_scene_knn is bvh_knn on a scene — the k nearest triangles of each point within its radius, over all active instances.  Its contract is the
 * union of bvh_scene_closest_point's and bvh_knn's; nothing in it is new arithmetic (tests/test_scene_knn.py restates it in numpy).
 *   candidate and acceptance: bvh_scene_closest_point's, word for word — the world triangle V_i = M_k v_i in the stated order, dist2 = tri_closest(V1, V2, V3, p),
 *     accepted iff dist2 <= r2 = radius * radius in f32.  A query with a NaN coordinate, a NaN radius or radius < 0 accepts nothing.  Inactive instances never
 *     answer; a triangle with a NaN world vertex is never accepted.
 *   answer: query i's list, d_hits[i*k .. i*k+k), is the min(k, accepted) accepted candidates with the smallest (dist2, instance_idx, prim_idx), compared
 *     lexicographically and stored in ascending order as {dist2, prim_idx, instance_idx, 0} records; each (instance, prim) pair appears at most once.  The list
 *     depends on none of the top-level builder, the BLAS builders, the layouts, the formats, the traversal order.  Slots past the list are
 *     {r2, BVH_INVALID, BVH_INVALID, 0}: all k of them for a query that accepts nothing.  d_counts[i], when given, is the list's length.  1 <= k <= BVH_KNN_MAX_K.
 *   relation to the other queries: with k == 1, (dist2, prim_idx, instance_idx) are bvh_scene_closest_point's BVH_QUERY_CLOSEST fields bit for bit, on every
 *     query (the walk is the same: near child first by lower bound at both levels, equal bounds go left).  With one identity instance, (dist2, prim_idx) are
 *     bvh_knn's on the BLAS, on well-conditioned queries.
 *   box tests: bvh_scene_closest_point's, unchanged — box_dist_pass on the world boxes at the top level; inside instance k the mapped point p' = W_k p, the
 *     slack e, boxes grown by 2^-16 * (their largest |coordinate|) + e, a subtree culled iff s2 * lb' * (1 - 2^-20) > bound (a NaN product never culls).  bound
 *     is the dist2 of the list's last entry once the list holds k entries and r2 before that; it is carried across instances and level changes.
 *   well-conditioned (lists exact): every entry of the query's true list meets bvh_scene_closest_point's conditions (1) and (2) against that
 *     entry's own dist2.  The bound never drops below the true k-th dist2, so no ancestor of a true entry is culled at either level.  On EVERY query each
 *     reported entry is an accepted candidate of its (instance, prim) with bit-equal dist2, the entries strictly ascend, and no list is lexicographically
 *     below the true one.
 *   no depth limit at either level: a query whose push would overflow the short stack, or whose walk exceeds the node count, is finished by a stackless pass
 *     through the plans the scene owns.  Asynchronous on the ctx's stream, no read-back.  bvh_ctx_kernel_times reports k_scene_knn and k_scene_knn_deep.
 *   errors write and enqueue nothing (BVH_E_INVALID_ARG): a NULL or unbuilt scene; NULL d_points or d_hits; k == 0 or k > BVH_KNN_MAX_K; n_points * k >= 2^32;
 *     the d_points / d_hits / d_counts ranges overlapping each other.  n_points == 0 returns 0 and touches nothing.  BLAS ordering as for bvh_scene_intersect.
 * All hits: bvh_scene_intersect_all is bvh_intersect_all on a scene — which triangles of which instances does each ray cross, ALL of them?  Its contract is the
 * union of bvh_scene_intersect's and bvh_intersect_all's; nothing in it is new arithmetic.
 *   hit test and acceptance: bvh_scene_intersect's, word for word — tri_hit on the object-space ray made by the instance maths above, accepted iff
 *     iu > 0 && iv > 0 && iw > 0 && tmin < it < tmax; t is not rescaled.  Inactive instances never answer.  A ray with a NaN component, or with
 *     !(tmin < tmax), accepts nothing.
 *   answer: ray i's set is ALL its accepted hits over all active instances, in compressed-row form: d_hits[d_offsets[i] .. d_offsets[i+1]) is ray i's slice,
 *     d_offsets[0] = 0, d_offsets[n_rays] = the total.  A record is {it, iu, iv, prim_idx, instance_idx, 0, 0, 0}.  Each (instance, prim) pair appears at most
 *     once per slice.  There are no miss records: an empty slice is a miss.  With d_hits == NULL the call only counts.
 *   order inside a slice: without BVH_HITS_SORTED unspecified, but the same call on the same arrays gives the same bytes.  With BVH_HITS_SORTED each slice is
 *     ascending in (t, instance_idx, prim_idx), compared lexicographically — the scene's closest-hit order, so a slice's first record is the BVH_QUERY_CLOSEST
 *     answer; the whole d_hits array then depends on none of the top-level builder, the BLAS builders, the layouts, the formats, the traversal order.
 *   box tests: bvh_intersect's conservative test at both levels, against [tmin, tmax] for the whole walk: the bound never shrinks.
 *   well-conditioned: bvh_scene_intersect's definition applied to EVERY accepted hit of the ray — the object-space ray is well-conditioned for its BLAS for
 *     that hit (§8b), and the hit's world point o + t d (f64) lies in its instance's world box grown by half the box test's growth.  On such rays the set is
 *     exact.  On EVERY ray each record is an accepted hit of its (instance, prim) with bit-equal t / u / v, and the slice is a subset of the true set.
 *   passes, capacity, total_out, saturation, asynchrony: exactly bvh_intersect_all's.  The call always counts and scans; the fill decides ON THE DEVICE whether
 *     it runs (d_hits != NULL, total <= capacity and total < 2^32); a skipped fill leaves d_hits untouched and d_offsets complete; total_out != NULL is the
 *     only host wait (an 8-byte read-back); a total of 2^32 or more saturates d_offsets at 0xFFFFFFFF and returns BVH_E_TOO_LARGE when total_out was given
 *     (with *total_out set); d_hits is never written outside ray i's slice nor past the total.  The scratch words are the ctx's, as for bvh_intersect_all; on
 *     a ctx that has no arena yet (a one-instance scene on a fresh ctx) the first call reserves the smallest one, as bvh_ctx_reserve(ctx, 2) would.
 *   per-ray counter: a scene ray's count is not bounded by 2^30 (it can cross many instances of one BLAS), so the per-ray counter saturates at 0xFFFFFFFD
 *     (one below the internal mark 0xFFFFFFFE of a ray left to the stackless pass): the mark is never a count.
 *   no depth limit at either level: a ray whose short stack would overflow is finished by a stackless pass through the plans the scene owns.  Both passes
 *     test the same boxes (every record below a root; neither the top-level root's own box nor a BLAS root's, for which the instance's world box stands), so
 *     count and fill agree on every ray's set whichever pass served it.
 *   errors enqueue and write nothing (BVH_E_INVALID_ARG): a NULL or unbuilt scene; NULL d_rays or d_offsets; a flag bit other than BVH_HITS_SORTED;
 *     n_rays >= 2^30; d_offsets or d_hits (capacity records, clamped to 2^32 - 1) overlapping d_rays or each other.
 *   n_rays == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.  BLAS ordering as for bvh_scene_intersect.
 *   bvh_ctx_kernel_times reports k_scene_hits_count, k_scene_hits_fill, k_scene_hits_deep (after each pass) and k_overlap_scan.
 * Radius search: bvh_scene_radius_search is bvh_radius_search on a scene — EVERY triangle of every active instance within the radius of each point.  Its
 * contract is the union of bvh_scene_closest_point's and bvh_radius_search's; nothing in it is new arithmetic (tests/test_scene_radius.py restates it in numpy).
 *   candidate and acceptance: bvh_scene_closest_point's, word for word — the world triangle V_i = M_k v_i in the stated order, dist2 = tri_closest(V1, V2, V3, p),
 *     accepted iff dist2 <= r2 = radius * radius in f32.  A query with a NaN coordinate, a NaN radius or radius < 0 accepts nothing.  Radius 0 (or -0) accepts
 *     the candidates at dist2 == 0; an infinite radius accepts every triangle of every active instance whose dist2 is not NaN.  Inactive instances never answer.
 *   answer: query i's set is ALL its accepted candidates over all active instances, in compressed-row form: d_hits[d_offsets[i] .. d_offsets[i+1]) is query
 *     i's slice, d_offsets[0] = 0, d_offsets[n_points] = the total.  A record is a bvh_instance_knn_hit {dist2, prim_idx, instance_idx, 0}.  Each
 *     (instance, prim) pair appears at most once per slice.  There is no padding and there are no miss records: an empty slice is a miss.  With d_hits == NULL
 *     the call only counts.
 *   order inside a slice: without BVH_RADIUS_SORTED unspecified, but the same call on the same arrays gives the same bytes.  With BVH_RADIUS_SORTED each slice
 *     is ascending in (dist2, instance_idx, prim_idx), compared lexicographically — bvh_scene_knn's order; the whole d_hits array then depends on none of the
 *     top-level builder, the BLAS builders, the layouts, the formats, the traversal order.  Any other flag bit is an error.  The sorted insertion is quadratic
 *     in the slice's length, as for bvh_radius_search: sort long slices on the caller's side.
 *   box tests: bvh_scene_closest_point's at both levels, against r2 for the whole walk: the bound never shrinks.  Top level: box_dist_pass on the world boxes.
 *     Inside instance k: the mapped point p' = W_k p and the slack e, boxes grown by 2^-16 * (their largest |coordinate|) + e, a subtree culled iff
 *     s2 * lb' * (1 - 2^-20) > r2 (a NaN product never culls).
 *   well-conditioned (set exact): every accepted candidate of the query meets bvh_scene_closest_point's conditions (1) and (2) against its own
 *     dist2.  On EVERY query each record is an accepted candidate of its (instance, prim) with bit-equal dist2, and the slice is a subset of the true set.
 *   relation to the other queries: on well-conditioned queries the first min(k, count) records of a sorted slice are bvh_scene_knn's list for the same point
 *     and k, bit for bit.  With one identity instance, (dist2, prim_idx) are bvh_radius_search's on the BLAS.
 *   passes, capacity, total_out, saturation, asynchrony: exactly bvh_scene_intersect_all's.  The call always counts and scans; the fill decides ON THE DEVICE
 *     whether it runs (d_hits != NULL, total <= capacity and total < 2^32); a skipped fill leaves d_hits untouched and d_offsets complete; total_out != NULL is
 *     the only host wait (an 8-byte read-back); a total of 2^32 or more saturates d_offsets at 0xFFFFFFFF and returns BVH_E_TOO_LARGE when total_out was given
 *     (with *total_out set); d_hits is never written outside query i's slice nor past the total.  The per-query counter saturates at 0xFFFFFFFD, so the
 *     internal mark 0xFFFFFFFE is never a count.  The scratch words are the ctx's, the same as bvh_scene_intersect_all's; on a ctx that has no arena yet (a
 *     one-instance scene on a fresh ctx) the first call reserves the smallest one, as bvh_ctx_reserve(ctx, 2) would.
 *   no depth limit at either level: a query whose short stack would overflow is finished by a stackless pass through the plans the scene owns.  Both passes
 *     test the same boxes (every record below a root; neither the top-level root's own box nor a BLAS root's, for which the instance's world box stands), so
 *     count and fill agree on every query's set whichever pass served it.
 *   errors enqueue and write nothing (BVH_E_INVALID_ARG): a NULL or unbuilt scene; NULL d_points or d_offsets; a flag bit other than BVH_RADIUS_SORTED;
 *     n_points >= 2^30; d_offsets or d_hits (capacity records, clamped to 2^32 - 1) overlapping d_points or each other.
 *   n_points == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.  BLAS ordering as for bvh_scene_intersect.
 *   bvh_ctx_kernel_times reports k_scene_radius_count, k_scene_radius_fill, k_scene_radius_deep (after each pass) and k_overlap_scan.
 * Box queries: bvh_scene_overlap is bvh_overlap on a scene — which triangles' leaf boxes of which active instances does each WORLD-space query box touch.
 * bvh_overlap(bvh_scene_tlas) alone is the broad phase (which instances); this is both phases in one call, and like bvh_overlap it is exact on EVERY query
 * (tests/test_scene_overlap.py restates the contract in numpy).
 *   mapped box: the mapped box of object box {lo, hi} under instance matrix M, with m_rc = object_to_world[4r + c], all in f32 without contraction; for row r
 *     a_c = m_rc * lo.c and b_c = m_rc * hi.c (c = 0, 1, 2),
 *     min.r = ((fminf(a_0, b_0) + fminf(a_1, b_1)) + fminf(a_2, b_2)) + m_r3,   max.r = ((fmaxf(a_0, b_0) + fmaxf(a_1, b_1)) + fmaxf(a_2, b_2)) + m_r3.
 *     For finite values this is, as values, the componentwise fminf / fmaxf over the box's 8 corners, each mapped in the order of the scene's world box
 *     (((m_r0 x + m_r1 y) + m_r2 z) + m_r3); it differs at most in the sign of a zero.
 *   test: pair (instance k, primitive j) passes query box q iff instance k is active, primitive j's leaf box b is valid (b.min <= b.max on every axis; the leaf
 *     box is layout 0's node n-1+j or layout 1's d_leaves[j].aabb, as bvh_overlap defines it) and box_overlap(q, mapped(M_k, b)) with bvh_overlap's closed,
 *     comparisons-only test: touching boxes overlap, a NaN anywhere fails, an inverted q overlaps nothing.
 *   answer: query i's set is EVERY passing pair, in compressed-row form: d_prims[d_offsets[i] .. d_offsets[i+1]) is query i's slice, d_offsets[0] = 0,
 *     d_offsets[n_boxes] = the total.  A record is a bvh_instance_prim {prim_idx, instance_idx}.  Each pair appears at most once per slice.  There are no miss
 *     records: an empty slice is a miss.  With d_prims == NULL the call only counts.
 *   order inside a slice: without BVH_SCENE_OVERLAP_SORTED unspecified, but the same call on the same arrays gives the same bytes.  With
 *     BVH_SCENE_OVERLAP_SORTED each slice is ascending in (instance_idx, prim_idx); the whole d_prims array then depends on none of the top-level builder, the
 *     BLAS builders, the layouts, the traversal order.  Any other flag bit is an error.  The sorted insertion is quadratic in the slice's length, as for the
 *     siblings: sort long slices on the caller's side.
 *   exactness: the set is exact for EVERY query — there is no well-conditioned share — whenever (1) every internal box of every BLAS contains its children's
 *     boxes (true bitwise of every tree the library makes, and after bvh_refit and bvh_optimize) and (2) every mapped value is finite.  Rounded f32
 *     multiplication by a fixed factor and rounded addition are monotone, so min.r / max.r are monotone in lo / hi, so a parent's mapped box contains its
 *     children's mapped boxes as values, so the instance's stored world box (the 8 mapped corners of the BLAS root box) contains everything below it; the
 *     top-level tree's containment is bitwise as before.  When (1) or (2) fails, every reported pair still passes its own test and the
 *     slice is a subset of the true set.
 *   walk tests: the top level uses box_overlap on the top-level nodes and the world boxes (one instance: its world box).  Inside an instance the test above —
 *     validity of the object box, then box_overlap against its mapped box — is applied to every record below the BLAS root; the BLAS root's own box is not
 *     tested: the world box stands for it.
 *   relation to the other queries: with one identity instance the prim sets equal bvh_overlap's on the BLAS for every query (((1 x + 0 y) + 0 z) + 0 == x as a
 *     value).  The instances that appear in query i's slice are a subset of slice i of bvh_overlap on bvh_scene_tlas.
 *   passes, capacity, total_out, saturation, asynchrony: exactly bvh_scene_radius_search's.  The call always counts and scans; the fill decides ON THE DEVICE
 *     whether it runs (d_prims != NULL, total <= capacity and total < 2^32); a skipped fill leaves d_prims untouched and d_offsets complete; total_out != NULL
 *     is the only host wait (an 8-byte read-back); a total of 2^32 or more saturates d_offsets at 0xFFFFFFFF and returns BVH_E_TOO_LARGE when total_out was
 *     given (with *total_out set); d_prims is never written outside query i's slice nor past the total.  The per-query counter saturates at 0xFFFFFFFD, so the
 *     internal mark 0xFFFFFFFE is never a count.  The scratch words are the ctx's, the same as bvh_scene_radius_search's; on a ctx that has no arena yet (a
 *     one-instance scene on a fresh ctx) the first call reserves the smallest one, as bvh_ctx_reserve(ctx, 2) would.
 *   no depth limit at either level: a query whose short stack would overflow is finished by a stackless pass through the plans the scene owns.  Both passes
 *     test the same boxes, so count and fill agree on every query's set whichever pass served it.
 *   errors enqueue and write nothing (BVH_E_INVALID_ARG): a NULL or unbuilt scene; NULL d_boxes or d_offsets; a flag bit other than
 *     BVH_SCENE_OVERLAP_SORTED; n_boxes >= 2^30; d_offsets or d_prims (capacity records, clamped to 2^32 - 1) overlapping d_boxes or each other.
 *   n_boxes == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.  BLAS ordering as for bvh_scene_intersect.
 *   bvh_ctx_kernel_times reports k_scene_overlap_count, k_scene_overlap_fill, k_scene_overlap_deep (after each pass) and k_overlap_scan.
 * Crossing triangle pairs: bvh_scene_intersect_tris is bvh_intersect_tris on a scene — which triangles of which active instances does each query triangle
 * properly cross?  Collision between the rigid bodies a scene models, without flattening it and after bvh_scene_update alone.  bvh_scene_overlap's two-level
 * broad phase and bvh_intersect_tris's exact narrow phase in one walk; like both it is exact on EVERY query (tests/test_scene_intersect_tris.py restates the
 * contract in numpy).
 *   tree-side triangle (k, j): the WORLD TRIANGLE of primitive j of instance k's BLAS, bvh_scene_closest_point's: with m_rc = object_to_world[4r + c],
 *     V.r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 for each of the three vertices (x, y, z), in f32 without contraction, in exactly this order.  It is a value
 *     that depends on the instance record and the BLAS triangle alone, not on the walk.
 *   query triangle i: BVH_SCENE_TRIS_QUERY — triangle i of `queries`, n_queries triangles already in world space, device pointers, any bvh_tri_format
 *     (morton_bits is ignored); query_instance must be 0.  BVH_SCENE_TRIS_INSTANCE — `queries` must be NULL and the rows are the triangles of instance
 *     query_instance: if i < n_leaves of that instance's BLAS, query i is the world triangle (query_instance, i); a row at or beyond n_leaves has an empty
 *     slice; an inactive query instance gives all-empty slices.  The device reads the BLAS index from the scene's instance array: there is no host read-back
 *     and the call stays asynchronous, also after a bvh_scene_update from device memory.  Instance query_instance itself is skipped BY INDEX; a second
 *     instance of the same BLAS is a different instance and answers.  As for BVH_TRIS_SELF the call reads triangle i of the BLAS's triangle array for every
 *     i < n_leaves, so that array must hold n_leaves triangles: this mode is NOT usable on a BLAS over bvh_split_refs references relabelled by
 *     bvh_remap_leaves, which the call cannot check.
 *   answer: pair (i; k, j) is reported iff (a) instance k is active (and, in INSTANCE mode, k != query_instance), (b) primitive j's leaf box b is valid on
 *     the OBJECT box, as for bvh_scene_overlap, (c) box_overlap(B(i), mapped(M_k, b)), where B(i) is stage E's box of query triangle i's three vertices, as in
 *     bvh_intersect_tris (clamps against the reset box included), and mapped is bvh_scene_overlap's expression above, and (d) crosses(query_i, worldtri(k, j)),
 *     bvh_intersect_tris's predicate word for word: IEEE f64 on the f32 world coordinates widened exactly, strict comparisons, proper() on both triangles.
 *     Compressed-row form: d_prims[d_offsets[i] .. d_offsets[i+1]) is query i's slice of bvh_instance_prim {prim_idx, instance_idx} records, d_offsets[0] = 0,
 *     d_offsets[n_queries] = the total.  Each pair appears at most once per slice.  There are no miss records: an empty slice crosses nothing.  With
 *     d_prims == NULL the call only counts.
 *   order inside a slice: without BVH_SCENE_TRIS_SORTED unspecified, but the same call on the same arrays gives the same bytes.  With BVH_SCENE_TRIS_SORTED
 *     each slice is ascending in (instance_idx, prim_idx); the whole d_prims array then depends on none of the top-level builder, the BLAS builders, the
 *     layouts, the formats, the traversal order.  Any other flag bit is an error.  The sorted insertion is quadratic in the slice's length.
 *   exactness: the set is exact for EVERY query — there is no well-conditioned share — whenever every mapped value and every world coordinate is finite, every
 *     internal box of every BLAS contains its children's boxes, and each leaf box is stage E's box of the BLAS triangle passed for it (true of a build, and
 *     of a refit with the same triangles).  The argument: (1) if a vertex v lies in an object box {lo, hi}, its world vertex lies in
 *     mapped(M, {lo, hi}) as values — each product m_rc * v.c lies between fminf and fmaxf of m_rc * lo.c and m_rc * hi.c because rounded multiplication by a
 *     fixed factor is monotone, and the three rounded sums and the translation are added in the same association in V.r and in min.r / max.r, and rounded
 *     addition is monotone; (2) stage E's leaf box contains its triangle's vertices (its clamps against the reset box leave every finite value as it is), so the mapped leaf box contains the world triangle; (3) two triangles
 *     that cross share a point, which lies in B(i) and in the world triangle's box, so B(i) overlaps the mapped leaf box; (4) bvh_scene_overlap's argument
 *     carries the pair up through the BLAS, the instance's world box and the top-level tree.  When a premise fails, every reported pair still passes its own
 *     four tests and the slice is a subset of the true set.
 *   relation to the other queries: with one identity instance, BVH_SCENE_TRIS_QUERY returns bvh_intersect_tris's prim sets on the BLAS
 *     (((1 x + 0 y) + 0 z) + 0 == x as a value).  Slice i's (instance, prim) pairs are a subset of bvh_scene_overlap's slice for the box B(i).  crosses() is
 *     symmetric, so (l, j) is in row i of INSTANCE(k) iff (k, i) is in row j of INSTANCE(l).
 *   passes, capacity, total_out, saturation, asynchrony, scratch words: exactly bvh_scene_overlap's — the call always counts and scans; the fill decides ON
 *     THE DEVICE whether it runs (d_prims != NULL, total <= capacity and total < 2^32); a skipped fill leaves d_prims untouched and d_offsets complete;
 *     total_out != NULL is the only host wait; a total of 2^32 or more saturates d_offsets at 0xFFFFFFFF and returns BVH_E_TOO_LARGE when total_out was given
 *     (with *total_out set); d_prims is never written outside query i's slice nor past the total; the per-query counter saturates at 0xFFFFFFFD; a
 *     one-instance scene on a fresh ctx reserves the smallest arena at the first call.
 *   no depth limit at either level: a query whose short stack would overflow is finished by a stackless pass through the plans the scene owns.  Both passes
 *     test the same boxes and the same triangles, so count and fill agree on every query's set whichever pass served it.
 *   errors enqueue and write nothing (BVH_E_INVALID_ARG): a NULL or unbuilt scene; NULL d_offsets; a flag bit other than BVH_SCENE_TRIS_SORTED;
 *     n_queries >= 2^30; mode not 0 or 1; NULL queries with BVH_SCENE_TRIS_QUERY; queries given with BVH_SCENE_TRIS_INSTANCE; query_instance >= n_instances
 *     with BVH_SCENE_TRIS_INSTANCE, query_instance != 0 with BVH_SCENE_TRIS_QUERY; a format error in queries (an unknown tri_format, a NULL or — for
 *     PACKED36 — misaligned d_tris, INDEXED with a NULL vertex or index pointer or n_vertices == 0); d_offsets or d_prims (capacity records, clamped to
 *     2^32 - 1) overlapping each other or the query mesh's triangle, vertex or index array.
 *   n_queries == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.  BLAS ordering as for bvh_scene_intersect.
 *   bvh_ctx_kernel_times reports k_scene_tris_count, k_scene_tris_fill, k_scene_tris_deep (after each pass) and k_overlap_scan.
 * All instances at once: bvh_scene_collide is BVH_SCENE_TRIS_INSTANCE asked for every instance in one call — the crossing triangle pairs between the bodies
 * of a scene, each unordered pair once, without a loop over instances on the host and without the host knowing which BLAS an instance places
 * (tests/test_scene_collide.py restates the contract in numpy).
 *   rows: the triangles of all instances, in instance order.  d_row_first[k] is the exclusive sum of n_leaves(BLAS of instance j) over the ACTIVE instances
 *     j < k — an inactive instance has no rows — and d_row_first[n_instances] = n_rows.  Row r with d_row_first[k] <= r < d_row_first[k+1] is query triangle
 *     (k, r - d_row_first[k]): the world triangle of that primitive of instance k, defined word for word as in BVH_SCENE_TRIS_INSTANCE.  Rows at or beyond
 *     n_rows, up to row_capacity, are empty.
 *   the table is made ON THE DEVICE from the scene's own instance array: there is no read-back, it follows a bvh_scene_update from device memory (also one that
 *     hands an instance another BLAS), and d_row_first is written on every successful call.  An n_rows of 2^32 or more saturates d_row_first at 0xFFFFFFFF.
 *   answer: pair (k, i; l, j) is in row (k, i) iff instance l is active; l > k — or, with BVH_SCENE_COLLIDE_BOTH, l != k —; and bvh_scene_intersect_tris's
 *     conditions (b), (c) and (d) hold unchanged: primitive j's leaf box b of instance l's BLAS is valid, box_overlap(B(k, i), mapped(M_l, b)), and
 *     crosses(worldtri(k, i), worldtri(l, j)) in f64 on the f32 world triangles with proper() on both.  So by default every unordered pair of triangles from
 *     two DIFFERENT instances appears exactly once, in the row of the lower instance; with BVH_SCENE_COLLIDE_BOTH every row holds all its partners.  Pairs
 *     inside one instance are never reported (that is BVH_TRIS_SELF on the BLAS); a second instance of the same BLAS is another instance and answers.
 *   output: compressed-row form over row_capacity rows: d_prims[d_offsets[r] .. d_offsets[r+1]) is row r's slice of bvh_instance_prim
 *     {prim_idx = j, instance_idx = l} records, d_offsets[0] = 0, d_offsets[row_capacity] = the total.  Without BVH_SCENE_COLLIDE_SORTED the order inside a
 *     slice is unspecified, but the same call on the same arrays gives the same bytes; with it each slice is ascending in (instance_idx, prim_idx), and the
 *     arrays then depend on no builder, layout or format.  The sorted insertion is quadratic in the slice's length.  With d_prims == NULL the call only counts.
 *   exactness: bvh_scene_intersect_tris's, on every row and under its premises (every mapped value and world coordinate finite, nested BLAS boxes, leaf boxes
 *     that are stage E's boxes of their triangles).  Under them the box test removes no crossing pair in either direction and crosses() is symmetric, so
 *     (1) the default answer is the BVH_SCENE_COLLIDE_BOTH answer filtered to instance_idx > k, (2) total(BOTH) == 2 * total(default), and (3) with
 *     SORTED | BOTH the rows of instance k equal the first n_leaves slices of bvh_scene_intersect_tris(BVH_SCENE_TRIS_INSTANCE, k, SORTED) byte for byte.
 *   too many rows: if n_rows > row_capacity nothing is walked, every offset is 0 and d_prims is untouched; d_row_first is still complete, so
 *     d_row_first[n_instances] tells a device-side caller; if rows_out was given, *rows_out = n_rows and the call returns BVH_E_TOO_LARGE.
 *   passes, capacity, total_out, saturation, scratch words, row_capacity == 0: exactly bvh_scene_overlap's over the row_capacity rows — count, scan, then a
 *     fill that decides ON THE DEVICE whether it runs (d_prims != NULL, total <= capacity and total < 2^32); a skipped fill leaves d_prims untouched and
 *     d_offsets complete; a total of 2^32 or more saturates d_offsets and returns BVH_E_TOO_LARGE when total_out was given.  rows_out and total_out are the
 *     only host waits (an 8-byte read-back each).  row_capacity == 0 writes d_offsets[0] = 0, *total_out = 0 and the table.
 *   like BVH_SCENE_TRIS_INSTANCE the call reads triangle i of each BLAS's triangle array for every i < n_leaves: it is NOT usable on a BLAS over
 *     bvh_split_refs references relabelled by bvh_remap_leaves, which the call cannot check.
 *   no depth limit at either level: a row whose short stack would overflow is finished by a stackless pass that tests the same boxes and triangles.
 *   errors enqueue and write nothing (BVH_E_INVALID_ARG): a NULL or unbuilt scene; NULL d_row_first or NULL d_offsets; a flag bit other than
 *     BVH_SCENE_COLLIDE_SORTED and BVH_SCENE_COLLIDE_BOTH; row_capacity >= 2^30; any two of d_row_first (n_instances + 1 words), d_offsets
 *     (row_capacity + 1 words) and d_prims (capacity records, clamped to 2^32 - 1) overlapping.
 *   bvh_ctx_kernel_times reports k_scene_collide_rows, k_scene_collide_count, k_scene_collide_fill, k_scene_collide_deep (after each pass) and
 *     k_overlap_scan.
 * Mesh-to-scene distance: bvh_scene_closest_tris is bvh_closest_tris on a scene — which triangle of which active instance is nearest to each query triangle,
 * and how far apart are the two (BVH_QUERY_CLOSEST), or is any within the radius (BVH_QUERY_ANY)?  Clearance of one body against the rest of an assembly,
 * contact generation with a margin (bodies that do not touch yet have an empty bvh_scene_intersect_tris / bvh_scene_collide set), penetration-free stepping,
 * tool-to-fixture distance, without flattening the scene and after bvh_scene_update alone.  One bvh_instance_tri_hit per query triangle.  The contract is the
 * union of bvh_closest_tris's and bvh_scene_closest_point's; nothing in it is new arithmetic (tests/test_scene_closest_tris.py restates it in numpy).
 *   tree-side triangle (k, j): the WORLD TRIANGLE of primitive j of instance k's BLAS, bvh_scene_closest_point's: with m_rc = object_to_world[4r + c],
 *     V.r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 for each of the three vertices, in f32 without contraction, in exactly this order.  Inactive instances never
 *     answer.
 *   query triangle i: bvh_scene_intersect_tris's, word for word.  BVH_SCENE_TRIS_QUERY — triangle i of `queries`, n_queries triangles already in world space,
 *     device pointers, any bvh_tri_format (morton_bits is ignored); query_instance must be 0.  BVH_SCENE_TRIS_INSTANCE — `queries` must be NULL and query i is
 *     the world triangle (query_instance, i); the instance is looked up ON THE DEVICE (no read-back; it follows a bvh_scene_update from device memory); a row at
 *     or beyond that BLAS's n_leaves misses, every row of an inactive query instance misses; the walk skips instance query_instance BY INDEX, a second
 *     instance of the same BLAS is another instance and answers.  As there, this mode reads triangle i of the BLAS's triangle array for every i < n_leaves and
 *     is NOT usable on a BLAS over bvh_split_refs references relabelled by bvh_remap_leaves, which the call cannot check.
 *   candidate of (i; k, j): bvh_closest_tris's dist2(X, Y) and feature with X = query triangle i and Y = the world triangle (k, j), all five steps word for
 *     word: the NaN rule on Y; a proper crossing (feature 15, dist2 0) only where the two WORLD stage-E boxes overlap; the three vertex terms of X against Y;
 *     the three of Y against X; the nine edge terms; the lowest index that attains the minimum wins.  The value does not depend on how the scene is walked.
 *   acceptance and answer: r2 = radius * radius in f32, ONE bound for the whole call (+inf: no bound).  A candidate is accepted iff dist2 <= r2.  A NaN or
 *     negative radius makes every query miss; a query triangle with a NaN coordinate misses.  BVH_QUERY_CLOSEST: the accepted candidate with the smallest
 *     (dist2, instance_idx, prim_idx), compared lexicographically — independent of the top-level builder, the BLAS builders, the layouts, the formats and the
 *     traversal order.  BVH_QUERY_ANY: some accepted candidate (the walk stops at the first); its record is that candidate's full dist2 and feature.
 *     Hit = {dist2, prim_idx, feature, instance_idx}; miss = {r2, BVH_INVALID, 0, BVH_INVALID}.
 *   box tests.  Top level: bvh_closest_tris's box_box_dist_pass on the instances' world boxes (each grown by 2^-16 * its largest |coordinate|) against the
 *     query's world stage-E box grown once the same way; with n_instances == 1 the one world box is tested, then the instance entered.  Inside instance k: the
 *     three query vertices x'_i = W_k x_i in the order of o' above; e = the largest over the three vertices of bvh_scene_closest_point's slack
 *     2^-20 max_r(((|w_r0||x| + |w_r1||y|) + |w_r2||z|) + |w_r3|); the object query box is the componentwise min / max of the x'_i, grown on every axis by
 *     2^-16 * (its largest |coordinate|) + e; a node box grows by 2^-16 * (its largest |coordinate|); the per-axis gap is
 *     fmaxf(fmaxf(lo_b - hi_q, lo_q - hi_b), 0) (a NaN plane is dropped), lb' = (gx*gx + gy*gy) + gz*gz, and the subtree is culled iff
 *     s2_k * lb' * (1 - 2^-20) > best (a NaN product never culls), s2_k being bvh_scene_closest_point's scale bound and best the world dist2 so far (r2 at the
 *     start), carried across instances.  A leaf pair whose two WORLD stage-E boxes fail bvh_closest_tris's rule against best is skipped before any term is
 *     computed.  (W_k is affine, so W_k x lies in the box of the W_k x_i for every point x of the query triangle, and
 *     |M y - x|^2 >= s2 |y - W x|^2.)
 *   well-conditioned (answers exact): for the true answer (k, j), (1) with x*_i = W_k x_i in f64 from the stored f32 entries, s2_k times the f64 squared gap
 *     between the box of the x*_i grown by 2^-17 * (its largest |coordinate|) + e / 2 and triangle j's object box grown by 2^-17 * (its largest |coordinate|) is
 *     <= the answer's dist2, and (2) the f64 squared gap between the query's world stage-E box and instance k's world box, each grown by 2^-17 * (its largest
 *     |coordinate|), is <= that dist2.  On every query a reported hit is an accepted candidate of its (instance, prim) with bit-equal dist2 and feature, and a
 *     closest answer is never lexicographically below the true one.
 *   relation to the other queries: with one identity instance the hit records are bvh_closest_tris's on the BLAS byte for byte (its reserved 0 is instance 0),
 *     misses equal but for the last word.  A row whose closest answer has feature 15 is a non-empty row of bvh_scene_intersect_tris; a non-empty row answers
 *     dist2 = 0, with feature 15 unless a candidate that touches the query at exactly 0 by a vertex or edge term has the lower (instance_idx, prim_idx).
 *   errors enqueue and write nothing (BVH_E_INVALID_ARG): a NULL or unbuilt scene; NULL d_hits; query not 0 or 1; mode not 0 or 1; NULL queries with
 *     BVH_SCENE_TRIS_QUERY; queries given with BVH_SCENE_TRIS_INSTANCE; query_instance >= n_instances with BVH_SCENE_TRIS_INSTANCE, query_instance != 0 with
 *     BVH_SCENE_TRIS_QUERY; n_queries >= 2^30; a format error in queries (as for bvh_scene_intersect_tris); d_hits overlapping the query mesh's triangle,
 *     vertex or index array.  n_queries == 0: returns 0 and touches nothing.  BLAS ordering as for bvh_scene_intersect.
 *   asynchronous on the ctx's stream, no read-back, no depth limit at either level (queries whose short stack would overflow are finished by a stackless pass
 *     through the top-level plan and the BLAS plans, with the same boxes and candidates).  bvh_ctx_kernel_times reports k_scene_closest_tris and
 *     k_scene_closest_tris_deep.
 * Every triangle within a radius, on scenes: bvh_scene_radius_tris is bvh_radius_tris on a scene — ALL triangles of all active instances within a distance
 * of each query triangle, with the squared distance and the feature pair.  Contact generation between the rigid bodies of a scene: barrier and penalty
 * methods want every vertex-face and edge-edge pair closer than a distance BEFORE the bodies touch (bvh_scene_intersect_tris and bvh_scene_collide are still
 * empty then), after bvh_scene_update alone and without flattening the scene.  The contract is the union of bvh_scene_closest_tris's and bvh_radius_tris's;
 * nothing in it is new arithmetic (tests/test_scene_radius_tris.py restates it in numpy).
 *   query triangle i: bvh_scene_closest_tris's, word for word.  BVH_SCENE_TRIS_QUERY — triangle i of `queries`, n_queries triangles already in world space,
 *     device pointers, any bvh_tri_format (morton_bits is ignored); query_instance must be 0.  BVH_SCENE_TRIS_INSTANCE — `queries` must be NULL and row i is
 *     the world triangle (query_instance, i); the instance is looked up ON THE DEVICE (no read-back; it follows a bvh_scene_update from device memory); a row at
 *     or beyond that BLAS's n_leaves is empty, every row of an inactive query instance is empty; the walk skips instance query_instance BY INDEX, a second
 *     instance of the same BLAS is another instance and answers.  This mode reads triangle i of the BLAS's triangle array for every i < n_leaves and is NOT
 *     usable on a BLAS over bvh_split_refs references relabelled by bvh_remap_leaves, which the call cannot check.
 *   candidate of (i; k, j): bvh_closest_tris's dist2(X, Y) and feature, steps 0-4 word for word, with X = query triangle i and Y = the WORLD triangle (k, j):
 *     V.r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 with m_rc = object_to_world[4r + c], in f32 without contraction, in exactly this order.  The crossing test
 *     (feature 15, dist2 0) runs only where the two world stage-E boxes overlap.  The value does not depend on how the scene is walked.
 *   acceptance: r2 = radius * radius in f32, ONE bound for the whole call.  A candidate is accepted iff dist2 <= r2.  A NaN or negative radius, or a query
 *     triangle with a NaN coordinate, makes the query dead: it accepts nothing.  Radius 0 accepts dist2 == 0, feature-15 crossings among them.  +inf accepts
 *     every non-NaN candidate of every active instance.  Inactive instances never answer.
 *   answer: ALL accepted candidates, in compressed-row form as bvh_scene_radius_search's: d_hits[d_offsets[i] .. d_offsets[i+1]) is query i's slice of
 *     bvh_instance_tri_hit {dist2, prim_idx, feature, instance_idx} records, d_offsets[0] = 0, d_offsets[n_queries] = the total.  Each (instance, prim) pair
 *     appears at most once per slice.  There are no miss records: an empty slice has nothing within the radius.  With d_hits == NULL the call only counts.
 *   order inside a slice: without BVH_SCENE_RADIUS_TRIS_SORTED unspecified, but the same call on the same arrays gives the same bytes.  With it each slice is
 *     ascending in (dist2, instance_idx, prim_idx), compared lexicographically; the arrays then depend on no builder, layout, format or traversal order, and
 *     the first record of a non-empty slice is bvh_scene_closest_tris(BVH_QUERY_CLOSEST)'s record for the same radius, bit for bit.  The sorted insertion is
 *     quadratic in the slice's length.
 *   box tests: bvh_scene_closest_tris's at both levels, against r2 for the WHOLE walk — the bound never shrinks.  Top level: box_box_dist_pass on the
 *     instances' world boxes (each grown by 2^-16 * its largest |coordinate|) against the query's world stage-E box grown once the same way.  Inside instance
 *     k: the object box of the three mapped vertices x'_i = W_k x_i, grown on every axis by 2^-16 * (its largest |coordinate|) + e with e as there; a node box
 *     grows by 2^-16 * (its largest |coordinate|); lb' = (gx*gx + gy*gy) + gz*gz over the per-axis gaps, and the subtree is culled iff
 *     s2_k * lb' * (1 - 2^-20) > r2 (a NaN product never culls).  A leaf pair whose two WORLD stage-E boxes fail bvh_closest_tris's rule against r2 is skipped
 *     before any term is computed.  Neither the top-level root's own box nor a BLAS root's own box is tested: the instance's world box stands for the BLAS root
 *     (with n_instances == 1 the one world box is tested, then the instance entered).  This holds in both passes.
 *   well-conditioned (the set exact): every accepted pair (i; k, j) meets bvh_scene_closest_tris's conditions (1) and (2) against its OWN dist2.  Then the
 *     slice is the full set (8y's argument with a constant bound).  On every query each record is an accepted candidate of its (instance, prim)
 *     with bit-equal dist2 and feature, and the slice is a subset of the true set.
 *   relation to the other queries: with one identity instance, offsets and records equal bvh_radius_tris's on the BLAS byte for byte (its reserved 0 is
 *     instance 0).  The feature-15 records at radius 0 are bvh_scene_intersect_tris's set.  Row i of INSTANCE(k) is NOT promised to mirror row j of
 *     INSTANCE(l) bit for bit: dist2(X, Y) and dist2(Y, X) run their f32 terms in different roles.
 *   passes, capacity, total_out, saturation, asynchrony, scratch words: exactly bvh_scene_radius_search's — the call always counts and scans; the fill decides
 *     ON THE DEVICE whether it runs (d_hits != NULL, total <= capacity and total < 2^32); a skipped fill leaves d_hits untouched and d_offsets complete;
 *     total_out != NULL is the only host wait; a total of 2^32 or more saturates d_offsets at 0xFFFFFFFF and returns BVH_E_TOO_LARGE when total_out was given
 *     (with *total_out set); d_hits is never written outside query i's slice nor past the total; the per-query counter saturates at 0xFFFFFFFD; a
 *     one-instance scene on a fresh ctx reserves the smallest arena at the first call.
 *   no depth limit at either level: a query whose short stack would overflow is finished by a stackless pass through the plans the scene owns.  Both passes
 *     test the same boxes and the same candidates, so count and fill agree on every query's set whichever pass served it.
 *   errors enqueue and write nothing (BVH_E_INVALID_ARG), bvh_scene_intersect_tris's in its order: a NULL or unbuilt scene; NULL d_offsets; a flag bit other
 *     than BVH_SCENE_RADIUS_TRIS_SORTED; mode not 0 or 1; NULL queries with BVH_SCENE_TRIS_QUERY; queries given with BVH_SCENE_TRIS_INSTANCE;
 *     query_instance >= n_instances with BVH_SCENE_TRIS_INSTANCE, query_instance != 0 with BVH_SCENE_TRIS_QUERY; n_queries >= 2^30; a format error in queries
 *     (as for bvh_scene_intersect_tris); d_offsets or d_hits (capacity records, clamped to 2^32 - 1) overlapping each other or the query mesh's triangle,
 *     vertex or index array.
 *   n_queries == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.  BLAS ordering as for bvh_scene_intersect.
 *   bvh_ctx_kernel_times reports k_scene_radius_tris_walk (count and fill), k_scene_radius_tris_deep (after each pass) and k_overlap_scan.
 * Convex volumes: bvh_scene_cull is bvh_cull on a scene — which triangles' leaf boxes of which active instances pass each WORLD-space convex volume (a view
 * frustum, the tile frusta of a view, shadow cascades against thousands of placed bodies), without flattening the scene and after bvh_scene_update alone.  It
 * answers both phases in one call and tighter than bvh_cull on bvh_scene_tlas followed by a flat test: a plane maps to a plane under an affine map, so each
 * instance is tested as its oriented box, not as the world box around it (tests/test_scene_cull.py restates the contract in numpy).
 *   planes, volumes, p-vertex, n-vertex, s(v) with its rule for zero coefficients, "passes", straddle: bvh_cull's, word for word; d_planes is in WORLD space.
 *     The rule applies to the numbers each test multiplies: the world coefficients against the world boxes, the OBJECT coefficients a', b', c' below against
 *     the leaf boxes (the object planes themselves are plain products and sums: an infinite matrix entry times a zero coefficient is still a NaN).  A NaN
 *     s or s' then comes only from inf - inf between terms whose coefficients are not zero, or from a NaN in the input.
 *   object planes of world plane (a, b, c, d) of volume i in instance k, with m_rc = object_to_world[4r + c] — the caller's forward matrix; no inverse is used:
 *     a' = fadd(fadd(fmul(a, m00), fmul(b, m10)), fmul(c, m20)), b' and c' the same with columns 1 and 2,
 *     d' = fadd(fadd(fadd(fmul(a, m03), fmul(b, m13)), fmul(c, m23)), d), each fmul / fadd ONE round-to-nearest f32 operation, never an FMA.  In exact
 *     arithmetic a'x + b'y + c'z + d' is the world plane evaluated at M x + t.
 *   test: pair (instance k, primitive j) passes volume i iff (1) instance k is active, (2) the scene's stored world box of k passes bvh_cull's test against
 *     the WORLD planes — exactly what bvh_cull on bvh_scene_tlas tests —, (3) primitive j's leaf box, as bvh_overlap defines it in both layouts, is valid, and
 *     (4) that leaf box passes bvh_cull's p-vertex test against the OBJECT planes of (i, k).  straddle bit p = !(s'(n-vertex of object plane p) >= 0), from
 *     the leaf's own object box against all planes; zero is written 0.
 *   answer: compressed rows as bvh_cull's, d_offsets[0] = 0, d_offsets[n_volumes] = the total; each pair appears at most once per slice; the order inside a
 *     slice is unspecified, but the same call on the same arrays with the same path gives the same bytes (slots never come from atomics).
 *   exactness: inside an instance the object planes are fixed numbers, so bvh_cull's argument (monotone products and sums) holds verbatim below the BLAS
 *     root, and top-level containment is bitwise, as before: every box above a passing leaf passes.  The set is exact for EVERY volume and independent of
 *     builders, layouts and path whenever every BLAS's boxes nest (true of every tree the library makes) and no s or s' is a NaN.  Outside that condition
 *     every reported pair still passes its own test and the slice is a subset.  The BLAS root's own box and the top-level root's own box are not tested, as
 *     in bvh_scene_overlap (the world box stands for the former).  A one-instance scene has no top-level tree: its world box is tested, then the instance is
 *     entered.
 *   relations: one identity instance gives bvh_cull's {prim, straddle} set on the BLAS for every volume with finite planes (((a 1 + b 0) + c 0) == a as a
 *     value; a zero's sign does not change n.k >= 0).  The instances occurring in slice i are a subset of slice i of bvh_cull on bvh_scene_tlas.  A slice
 *     never contains an inactive instance.
 *   path: bvh_cull_path.  BVH_CULL_LANE walks one volume per lane on both levels; BVH_CULL_GROUP gives each volume a workgroup of 256 threads and a work stack
 *     of BVH_SCENE_CULL_GROUP_STACK {instance, node} entries in LDS, on bvh_cull's fixed schedule (each round the m = min(top, 256) entries at the top, thread
 *     t entry top - m + t; a passing top-level leaf whose instance is active is pushed as that BLAS's root; emits and pushes in thread order, left before
 *     right); BVH_CULL_AUTO takes the group walk iff n_volumes <= 65536 and n_instances + the largest registered BLAS's n_leaves >= 1024.
 *   passes, capacity, total_out, saturation, BVH_E_TOO_LARGE, asynchrony, scratch words: exactly bvh_scene_overlap's — the call always counts and scans; the
 *     fill decides ON THE DEVICE whether it runs (d_hits != NULL, total <= capacity, total < 2^32) and otherwise leaves d_hits untouched with d_offsets
 *     complete; the 8-byte read-back happens only with total_out != NULL; a volume's counter saturates at 0xFFFFFFFD.  No depth or size limit at either
 *     level: a volume whose short stack or work stack would overflow is finished by a stackless pass through the top-level plan and the BLAS plans.
 *   errors (nothing is written or enqueued, BVH_E_INVALID_ARG): NULL or unbuilt scene, NULL d_planes or d_offsets, planes_per_volume outside 1 .. 8, path
 *     outside 0 .. 2, n_volumes >= 2^30, d_offsets or d_hits (capacity records) overlapping d_planes or each other.
 *   n_volumes == 0: returns 0, writes d_offsets[0] = 0 and *total_out = 0, touches nothing else.  BLAS ordering as for bvh_scene_intersect.
 *   bvh_ctx_kernel_times reports k_scene_cull_walk or k_scene_cull_group (count and fill), k_scene_cull_deep (after each pass) and k_overlap_scan.
 * Winding numbers: bvh_scene_winding_number is bvh_winding_number on a scene — inside / outside against an assembly of bodies, the sign for
 * bvh_scene_closest_point's distance, voxelisation and point-in-union over thousands of bvh_build_many bodies — without flattening the scene.  Two calls:
 * bvh_scene_winding_prepare after a build or an update, bvh_scene_winding_number per batch of points (tests/test_scene_winding.py restates both in numpy).
 * All f32 without contraction in the stated order unless marked f64; dot and cross products as in the bvh_winding_number section.
 *   world triangle of (instance k, primitive j): V_i = M_k v_i, V_i.r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 — bvh_scene_closest_point's, in its order.
 *   exact value: w(q) = the sum over the ACTIVE instances k and their primitives j of Omega(V1, V2, V3; q) / 4 pi, Omega being bvh_winding_number's leaf term
 *     word for word on the world triangle and the world point.  The value is stated on world triangles because the solid angle of ONE triangle is not
 *     invariant under a general 3x4 map; only the total over a closed surface is, so an object-space evaluation answers another function on open meshes under
 *     shear or non-uniform scale.  A reflecting instance (det < 0) therefore contributes -1 inside: no sign rule is added.  Inactive instances
 *     contribute nothing.  With beta = +inf the answer is this plain sum.
 *   per instance (active; bvh_winding_map, written by prepare), with M = [A | t]: c = the cofactor matrix C of A, row-major: row 0 = {c00, c01, c02} of the
 *     instance maths above, row 1 = {a02 a21 - a01 a22, a00 a22 - a02 a20, a01 a20 - a00 a21}, row 2 = {a01 a12 - a02 a11, a02 a10 - a00 a12,
 *     a00 a11 - a01 a10}, in f64 from the f32 entries, each rounded once to f32.  It maps area vectors: cross(A u, A v) = C (u x v).
 *     smax = (float)sqrt(lambda), lambda = max_i (|S_i0| + |S_i1|) + |S_i2| with S_ij = (a_i0 a_j0 + a_i1 a_j1) + a_i2 a_j2 in f64: a Gershgorin bound on the
 *     largest singular value of A, with no guard factor on purpose (the identity gives exactly 1).  An inactive instance's record is all zero.
 *   a BLAS node seen from the world: a BLAS node has the object record {A, area, p, r} — bvh_winding_prepare's, unchanged, made once per BLAS.  In instance k:
 *     A_w.i = (C_i0 Ax + C_i1 Ay) + C_i2 Az; p_w = M_k p (the order above); r_w = smax * r; d = p_w - q; d2 = (dx*dx + dy*dy) + dz*dz; t = beta * r_w.  The
 *     node is APPROXIMATED iff d2 > t * t (false on NaN); its term is dot(A_w, d) / ((FOURPI * d2) * sqrtf(d2)).  Every object point within r of p maps to
 *     within sigma_max(A) r <= r_w of p_w, so the far-field condition of the flat walk holds in world space.
 *   instance moment (a bvh_winding_moment, one per instance), from the BLAS root's record: A_k = C A in the order of A_w; area a_k = (smax * smax) * area;
 *     p = c_k = M_k p; r_k = the distance from c_k to the farthest corner of the instance's world box, by bvh_winding_prepare's formula for r.  Inactive: all zero.
 *   top-level moments: bvh_winding_moment[n_instances - 1], record i for top-level node i: bvh_winding_prepare's climb on the top-level tree with the leaf sums
 *     {A_k, a_k, a_k * c_k} of the leaf's instance; an internal node's sums are left + right, following the tree, bit-reproducible; then p = M / a, or the
 *     centre of the node's stored box if a is 0 or not finite, and r from the node's stored box, exactly as bvh_winding_prepare.
 *   walk: with n_instances >= 2 the top-level root is always opened.  An internal top-level child follows bvh_winding_number's rule on its top-level record.
 *     A top-level leaf child is instance k: it contributes its instance dipole (d = c_k - q with A_k and r_k) iff approximated, otherwise it is entered: its
 *     BLAS root is opened, below it internal children use the world-mapped rule and leaf children add the world-triangle term.  With n_instances == 1 the
 *     instance is always entered.  Children are taken left first.  The f32 terms go into one f64 sum carried across levels, stored as f32; a NaN answer is
 *     stored as 0x7FC00000, a query with a NaN coordinate writes that NaN, the radius is ignored.
 *   consequences: one identity instance opens exactly the nodes bvh_winding_number opens on the BLAS and adds bit-equal terms; any similarity transform gives
 *     the flat answer at the mapped point, up to rounding.
 *   bvh_scene_winding_prepare(scene, flags): the scene owns the memory (allocated by the first prepare after a build, outside the ctx's arena, freed by the
 *     next build): the per-BLAS moments, one exchange word per BLAS leaf (kept all-INVALID), the per-instance maps, the instance moments and the top-level
 *     moments.  The moments of ALL BLASes are made by one climb launch and one finish launch, whatever n_blas is (one thread per (BLAS, sorted leaf), the
 *     BLAS found in a prefix table made from the descriptors): byte for byte bvh_winding_prepare's records of each BLAS.  BVH_SCENE_WINDING_KEEP_BLAS skips
 *     them when a prepare has succeeded since the last bvh_scene_build: the cheap path after bvh_scene_update, which only moves instances.  A caller who
 *     refits a BLAS prepares without the flag; the scene cannot detect a refit.  bvh_scene_build discards everything; bvh_scene_update makes the instance and
 *     top-level part stale.  Asynchronous on the ctx's stream (the first prepare after a build allocates and copies the table, which blocks).  Errors
 *     (BVH_E_INVALID_ARG): a NULL or unbuilt scene, a flag bit other than BVH_SCENE_WINDING_KEEP_BLAS; BVH_E_TOO_LARGE: 2^32 or more BLAS leaves in all.
 *   bvh_scene_winding_number(scene, d_points, n_points, beta, d_w): asynchronous, no read-back, no depth limit at either level (queries whose short stack
 *     would overflow are finished by a stackless pass through the top-level plan and the BLAS plans).  Returns BVH_E_INVALID_ARG and writes nothing for a
 *     NULL or unbuilt scene, moments missing or stale (no prepare since the last build or update), NULL d_points or d_w, beta < 0 or NaN, overlapping
 *     d_points / d_w ranges.  n_points == 0 returns 0 and touches nothing.  BLAS ordering as for bvh_scene_intersect.
 *   accessors (read-only device pointers, valid until the next bvh_scene_build or bvh_scene_destroy; BVH_E_INVALID_ARG while the part asked for is missing or
 *     stale): bvh_scene_winding_moments(scene, blas, ...) gives BLAS blas's n_leaves - 1 records or, with blas == BVH_INVALID, the top-level tree's
 *     n_instances - 1 (NULL and 0 with one instance); bvh_scene_winding_instances gives the instance moments and the maps (either pointer may be NULL).
 *   bvh_ctx_kernel_times reports k_scene_winding_climb and k_scene_winding_finish (both levels), k_scene_winding_inst, k_scene_winding and
 *     k_scene_winding_deep. */
typedef struct { bvh_result tree; bvh_build_input tris; } bvh_blas;   /* tris.tri_format PADDED64 with d_tris NULL: tree.d_tris is Triangle[n_leaves] */
typedef struct bvh_scene bvh_scene;
int  bvh_scene_create(bvh_ctx* ctx, bvh_scene** out);
void bvh_scene_destroy(bvh_scene* scene);
int  bvh_scene_build(bvh_scene* scene, bvh_algo algo, const bvh_blas* blas /* host [n_blas] */, uint32_t n_blas,
                     const bvh_instance* instances, uint32_t n_instances, int instances_on_device, bvh_timings* timings /* may be NULL */);
int  bvh_scene_update(bvh_scene* scene, const bvh_instance* instances, int instances_on_device, bvh_timings* timings /* may be NULL */);
int  bvh_scene_intersect(bvh_scene* scene, const bvh_ray* d_rays, uint32_t n_rays, bvh_instance_hit* d_hits, int query /* bvh_query_kind */);
int  bvh_scene_closest_point(bvh_scene* scene, const bvh_point_query* d_points, uint32_t n_points, bvh_instance_point_hit* d_hits, int query /* bvh_query_kind */);
int  bvh_scene_knn(bvh_scene* scene, const bvh_point_query* d_points, uint32_t n_points, uint32_t k,
                   bvh_instance_knn_hit* d_hits /* [n_points * k], query i's list at d_hits[i*k .. i*k+k) */, uint32_t* d_counts /* [n_points] or NULL */);
int  bvh_scene_intersect_all(bvh_scene* scene, const bvh_ray* d_rays, uint32_t n_rays, uint32_t flags /* 0 or BVH_HITS_SORTED */,
                             uint32_t* d_offsets /* u32[n_rays + 1], device */, bvh_instance_hit* d_hits /* [capacity], device, or NULL: count only */,
                             uint64_t capacity, uint64_t* total_out /* host, may be NULL */);
int  bvh_scene_radius_search(bvh_scene* scene, const bvh_point_query* d_points, uint32_t n_points, uint32_t flags /* 0 or BVH_RADIUS_SORTED */,
                             uint32_t* d_offsets /* u32[n_points + 1], device */, bvh_instance_knn_hit* d_hits /* [capacity], device, or NULL: count only */,
                             uint64_t capacity, uint64_t* total_out /* host, may be NULL */);
#define BVH_SCENE_OVERLAP_SORTED 1u
int  bvh_scene_overlap(bvh_scene* scene, const bvh_aabb* d_boxes, uint32_t n_boxes, uint32_t flags /* 0 or BVH_SCENE_OVERLAP_SORTED */,
                       uint32_t* d_offsets /* u32[n_boxes + 1], device */, bvh_instance_prim* d_prims /* [capacity], device, or NULL: count only */,
                       uint64_t capacity, uint64_t* total_out /* host, may be NULL */);
typedef struct { uint32_t prim; uint32_t instance; uint32_t straddle; uint32_t zero; } bvh_scene_cull_hit;   /* 16 bytes, one store */
#define BVH_SCENE_CULL_GROUP_STACK 8192   /* entries {instance, node} of the group walk's LDS work stack: 64 KiB, two workgroups per CU */
int  bvh_scene_cull(bvh_scene* scene, const float* d_planes /* float[n_volumes][planes_per_volume][4], device, WORLD space */,
                    uint32_t n_volumes, uint32_t planes_per_volume /* 1 .. BVH_CULL_MAX_PLANES */, int path /* bvh_cull_path */,
                    uint32_t* d_offsets /* u32[n_volumes + 1], device */, bvh_scene_cull_hit* d_hits /* [capacity], device, or NULL: count only */,
                    uint64_t capacity, uint64_t* total_out /* host, may be NULL */);
typedef enum { BVH_SCENE_TRIS_QUERY = 0, BVH_SCENE_TRIS_INSTANCE = 1 } bvh_scene_tris_mode;
#define BVH_SCENE_TRIS_SORTED 1u
int  bvh_scene_intersect_tris(bvh_scene* scene, const bvh_build_input* queries /* world-space mesh, device, any bvh_tri_format; NULL with BVH_SCENE_TRIS_INSTANCE */,
                              uint32_t n_queries, int mode /* bvh_scene_tris_mode */, uint32_t query_instance /* BVH_SCENE_TRIS_INSTANCE only, else 0 */,
                              uint32_t flags /* 0 or BVH_SCENE_TRIS_SORTED */, uint32_t* d_offsets /* u32[n_queries + 1], device */,
                              bvh_instance_prim* d_prims /* [capacity], device, or NULL: count only */, uint64_t capacity,
                              uint64_t* total_out /* host, may be NULL */);
#define BVH_SCENE_COLLIDE_SORTED 1u
#define BVH_SCENE_COLLIDE_BOTH   2u
int  bvh_scene_collide(bvh_scene* scene, uint32_t flags /* BVH_SCENE_COLLIDE_SORTED | BVH_SCENE_COLLIDE_BOTH */,
                       uint32_t* d_row_first /* u32[n_instances + 1], device */, uint32_t row_capacity,
                       uint32_t* d_offsets /* u32[row_capacity + 1], device */, bvh_instance_prim* d_prims /* [capacity], device, or NULL: count only */,
                       uint64_t capacity, uint64_t* rows_out /* host, may be NULL */, uint64_t* total_out /* host, may be NULL */);
int  bvh_scene_closest_tris(bvh_scene* scene, const bvh_build_input* queries /* world-space mesh, device, any bvh_tri_format; NULL with BVH_SCENE_TRIS_INSTANCE */,
                            uint32_t n_queries, int mode /* bvh_scene_tris_mode */, uint32_t query_instance /* BVH_SCENE_TRIS_INSTANCE only, else 0 */,
                            float radius, bvh_instance_tri_hit* d_hits /* [n_queries], device */, int query /* bvh_query_kind */);
#define BVH_SCENE_RADIUS_TRIS_SORTED 1u
int  bvh_scene_radius_tris(bvh_scene* scene, const bvh_build_input* queries /* world-space mesh, device, any bvh_tri_format; NULL with BVH_SCENE_TRIS_INSTANCE */,
                           uint32_t n_queries, int mode /* bvh_scene_tris_mode */, uint32_t query_instance /* BVH_SCENE_TRIS_INSTANCE only, else 0 */,
                           float radius, uint32_t flags /* 0 or BVH_SCENE_RADIUS_TRIS_SORTED */, uint32_t* d_offsets /* u32[n_queries + 1], device */,
                           bvh_instance_tri_hit* d_hits /* [capacity], device, or NULL: count only */, uint64_t capacity,
                           uint64_t* total_out /* host, may be NULL */);
#define BVH_SCENE_WINDING_KEEP_BLAS 1u
int  bvh_scene_winding_prepare(bvh_scene* scene, uint32_t flags /* 0 or BVH_SCENE_WINDING_KEEP_BLAS */);
int  bvh_scene_winding_number(bvh_scene* scene, const bvh_point_query* d_points /* radius ignored */, uint32_t n_points, float beta,
                              float* d_w /* f32[n_points], device */);
int  bvh_scene_winding_moments(const bvh_scene* scene, uint32_t blas /* or BVH_INVALID: the top level */, const bvh_winding_moment** d_moments, uint32_t* count);
int  bvh_scene_winding_instances(const bvh_scene* scene, const bvh_winding_moment** d_inst_moments /* [n_instances] */,
                                 const bvh_winding_map** d_maps /* [n_instances] */);
int  bvh_scene_tlas(const bvh_scene* scene, bvh_result* out);

/* ---- stage-level entry points (one per reference kernel / library call on the path) -------------------------- */

/* CalculateSceneExtents (src/CommonBlocksKernel.h:92-114): Triangle[n] -> Aabb[n] + scene Aabb.
 * d_scene_extent is reset to {+FltMax,-FltMax} first (src/PLOC++Bvh.cpp:23-25). */
int  bvh_stage_extents(bvh_ctx* ctx, const void* d_tris, uint32_t n, void* d_prim_aabbs, void* d_scene_extent);
/* CalculateMortonCodes (src/CommonBlocksKernel.h:374-385): 30-bit extended Morton keys, values = 0..n-1. d_vals may be NULL. */
int  bvh_stage_morton(bvh_ctx* ctx, const void* d_prim_aabbs, uint32_t n, const void* d_scene_extent,
                      uint32_t* d_keys, uint32_t* d_vals);
/* Oro::RadixSort::sort(KeyValueSoA src, KeyValueSoA dst, n, startBit, endBit, stream)
 * (call sites src/TwoPassLbvh.cpp:71-89 ...): stable ascending LSD radix sort on key bits [start_bit, end_bit).
 * d_vals_in == NULL sorts (key, index) pairs.  src is not modified. */
int  bvh_sort_pairs(bvh_ctx* ctx, const uint32_t* d_keys_in, const uint32_t* d_vals_in, uint32_t n,
                    uint32_t* d_keys_out, uint32_t* d_vals_out, int start_bit, int end_bit);
/* InitBvhNodes + BvhBuildAndFit (src/SinglePassLbvhKernel.h:27-126) -> Bvh2Node[2n-1], *root_out = root index */
int  bvh_emit_lbvh_single(bvh_ctx* ctx, const void* d_prim_aabbs, const uint32_t* d_sorted_keys,
                          const uint32_t* d_sorted_vals, uint32_t n, void* d_nodes, uint32_t* root_out);
/* InitBvhNodesPrimRef + BvhBuild + FitBvhNodes (src/TwoPassLbvhKernel.h:164-235) -> Bvh2Node[2n-1], root 0 */
int  bvh_emit_lbvh_two(bvh_ctx* ctx, const void* d_prim_aabbs, const uint32_t* d_sorted_keys,
                       const uint32_t* d_sorted_vals, uint32_t n, void* d_nodes);
/* SetupClusters + Ploc/SinglePassPloc + host loop (src/Ploc++Kernel.h:39-362, src/PLOC++Bvh.cpp:132-152) */
int  bvh_emit_ploc(bvh_ctx* ctx, const void* d_prim_aabbs, const uint32_t* d_sorted_vals, uint32_t n,
                   void* d_nodes, void* d_leaves, uint32_t* iterations_out);
/* SetupClusters + HPloc (src/HplocKernel.h:39-315) */
int  bvh_emit_hploc(bvh_ctx* ctx, const void* d_prim_aabbs, const uint32_t* d_sorted_keys,
                    const uint32_t* d_sorted_vals, uint32_t n, void* d_nodes, void* d_leaves);

/* ---- consumers' helpers --------------------------------------------------------------------------------------- */
/* PLOC layout -> LBVH layout (Bvh2Node[2n-1]) so that the reference's traversal kernels (src/TraversalKernel.h) can
 * consume PLOC/HPLOC trees; the adapter the reference never wrote. */
int  bvh_to_lbvh_layout(bvh_ctx* ctx, const bvh_result* in, void* d_nodes_2n_minus_1);
/* CollapseToWide4Bvh (src/TwoPassLbvhKernel.h:237-336, src/Ploc++Kernel.h:364-465) + host set-up (src/TwoPassLbvh.cpp:154-183):
 * BVH2 -> BVH4.  d_bvh4: Bvh4Node[n] (128 B each, src/Common.h:560-566), d_primnodes: PrimNode[n] (src/Common.h:568-572);
 * wide root = node 0; *n_wide_out = number of wide nodes.  Blocking (reads the level bounds back). */
int  bvh_collapse4(bvh_ctx* ctx, const bvh_result* in, void* d_bvh4, void* d_primnodes, uint32_t* n_wide_out);
/* duration of the last bvh_collapse4 on this ctx (the reference's CollapseBvhTime token); 0 unless profiling was on */
int  bvh_ctx_last_collapse_ms(const bvh_ctx* ctx, float* ms_out);
/* ---- consumer side used by the image check ---- */
/* GenerateRays (src/CommonBlocksKernel.h:432-463).  h_camera: 64-byte Camera record (src/Common.h:550-558) on the host;
 * d_rays: Ray[width*height] (32 bytes each, src/Common.h:533-539), ray of pixel (gx,gy) at index gx*height+gy. */
int  bvh_generate_rays(bvh_ctx* ctx, const void* h_camera, void* d_rays, uint32_t width, uint32_t height);
/* BvhTraversalWhile (src/TraversalKernel.h:238-335): while-while closest-hit traversal of an LBVH-layout Bvh2Node[2n-1] array
 * (use bvh_to_lbvh_layout for PLOC/HPLOC results).  h_transform: 64-byte Transformation (src/Common.h:541-548) on the host.
 * d_rgba: width*height*4 bytes, cleared, then u8 (u*255, v*255, (1-u-v)*255, 255) per hit pixel at index gx*width+gy.
 * Square images only (the reference indexes rays with height and pixels with width). */
int  bvh_trace_while(bvh_ctx* ctx, const void* d_rays, const void* d_tris, const void* d_nodes_lbvh, uint32_t root, uint32_t n_internal,
                     const void* h_transform, void* d_rgba, uint32_t width, uint32_t height);
/* The reference's four traversal kernels behind one entry point: BvhTraversalRestartTrail (src/TraversalKernel.h:49-146; stackless, a
 * restart re-enters at node 0, so root must be 0), BvhTraversalifif (:148-236), BvhTraversalWhile (:238-335), BvhTraversalSpeculativeWhile
 * (:337-451; the wave vote spans 64 lanes here).  Same arguments as bvh_trace_while; d_ray_counter (optional, u32[width*height]) receives
 * the triangle tests per ray (the reference's rayCounter; not counted by the while-while kernel: zeroed).  All four produce the same image. */
typedef enum { BVH_TRACE_WHILE_WHILE = 0, BVH_TRACE_RESTART_TRAIL = 1, BVH_TRACE_IF_IF = 2, BVH_TRACE_SPECULATIVE_WHILE = 3 } bvh_trace_kind;
int  bvh_trace(bvh_ctx* ctx, bvh_trace_kind kind, const void* d_rays, const void* d_tris, const void* d_nodes_lbvh, uint32_t root, uint32_t n_internal,
               const void* h_transform, void* d_rgba, uint32_t* d_ray_counter, uint32_t width, uint32_t height);
/* BVH2 SAH cost with the formula of Utility::calculateLbvhCost (src/Utility.cpp:317-349), device reduction, f64. */
int  bvh_sah_cost(bvh_ctx* ctx, const bvh_result* in, double* cost_out);
/* BVH4 cost with the formula of Utility::calculatebvh4Cost (src/Utility.cpp:351-396) — the value the reference's builders store in
 * m_cost after the collapse (src/TwoPassLbvh.cpp:196, src/SinglePassLbvh.cpp:186, src/PLOC++Bvh.cpp:195, src/Hploc.cpp:164).
 * d_bvh4 / d_primnodes / n_wide: outputs of bvh_collapse4; d_prim_aabbs: Aabb[n] by primitive index (bvh_result.d_prim_aabbs).
 * Device reduction, f32 terms, f64 accumulation.  Blocking. */
int  bvh_bvh4_cost(bvh_ctx* ctx, const void* d_bvh4, uint32_t n_wide, const void* d_primnodes, const void* d_prim_aabbs, uint32_t n, double* cost_out);
/* Order-independent 64-bit checksum of a result's node array, leaf array (PLOC layouts) and root index: equal checksums <=> byte-identical
 * results (up to hash collisions).  Lets hosts compare builds (batched vs single, run vs run) without reading the arrays back.  Blocking. */
int  bvh_checksum(bvh_ctx* ctx, const bvh_result* in, uint64_t* checksum_out);
/* copy a result's arrays to host (blocking), sizes per layout; any pointer may be NULL.  h_sorted_keys: u32[n] or, for
 * key_bits == 64 results, u64[n] */
int  bvh_download(bvh_ctx* ctx, const bvh_result* in, void* h_nodes, void* h_leaves, void* h_sorted_keys,
                  uint32_t* h_sorted_vals, void* h_scene_extent);

/* BatchedBvhBuilder::build (src/BatchedBuilder.h:12-31) re-purposed as the multi-GPU scene shard (BASELINE.json config 5), one
 * process: mesh m -> devs[m % n_dev], one ctx + host thread per device, then ONE RCCL all-gather of the root AABBs.
 * h_tris[m]: host Triangle[n_tris[m]].  root_aabbs_out: 6 floats per mesh (min xyz, max xyz).  build_ms_out (optional):
 * E+M+S+B milliseconds per mesh.  Blocking. */
int  bvh_batched_build(int n_dev, const int* devs, bvh_algo algo, const void* const* h_tris, const uint32_t* n_tris, int n_meshes,
                       float* root_aabbs_out, float* build_ms_out);
/* The same as a reusable object: the per-device contexts (arenas), the RCCL communicator and the gather buffers are created once and
 * kept across builds (bvh_batched_build pays for them on every call).  Report fields are optional except root_aabbs. */
typedef struct bvh_batch bvh_batch;
/* where one mesh's tree lives after bvh_batch_build (the reference's BatchedBvhBuilder keeps every mesh's nodes and leaves on the device: d_bvhNodes / d_primRefs /
 * d_rootNodes, src/BatchedBuilder.h:24-26).  Device memory owned by the batch, valid until its next build or bvh_batch_destroy; child indices are mesh-local. */
typedef struct {
    int32_t     device;        /* HIP device the arrays live on */
    uint32_t    n_leaves, n_internal, n_nodes, root, layout;   /* as bvh_result; n_nodes = Bvh2Node records at d_nodes (layout 0: 2n-1, layout 1: n-1) */
    const void* d_nodes;       /* Bvh2Node[n_nodes] */
    const void* d_leaves;      /* PrimRef[n_leaves] (layout 1) or NULL (layout 0: the leaves are nodes n-1 .. 2n-2) */
} bvh_batch_mesh;
typedef struct {
    float*    root_aabbs;      /* [6 * n_meshes] min xyz, max xyz per mesh, as all-gathered (device devs[0]'s copy) */
    float*    build_ms;        /* [n_meshes] or NULL: E+M+S+B per mesh (stage events) */
    uint64_t* checksums;       /* [n_meshes] or NULL: bvh_checksum of each mesh's tree */
    double*   sah;             /* [n_meshes] or NULL: bvh_sah_cost of each mesh's tree */
    float     allgather_us;    /* out: duration of the RCCL all-gather of the root boxes (HIP events, max over devices) */
    float     wall_ms;         /* out: host wall time of the call (H2D copies of the inputs included) */
    bvh_batch_mesh* meshes;    /* [n_meshes] or NULL: every mesh's tree is copied out of its context's arena and kept (ABI 4) */
    int32_t   lanes_per_device;/* out: contexts (streams + host threads) each device pipelined its meshes on: min(3, meshes per device) (ABI 4) */
    int32_t   reserved;
} bvh_batch_report;
int  bvh_batch_create(int n_dev, const int* devs, bvh_batch** out);
/* mesh m is built on devs[m % n_dev]; a device that holds several meshes pipelines them on up to three contexts (H2D of one mesh, build of another, checksum /
 * tree copy of a third overlap); one ncclAllGather of the root boxes at the end.  Blocking. */
int  bvh_batch_build(bvh_batch* batch, bvh_algo algo, const void* const* h_tris, const uint32_t* n_tris, int n_meshes, bvh_batch_report* report);
/* read one kept tree back (h_nodes: Bvh2Node[n_nodes], h_leaves: PrimRef[n_leaves] or NULL) */
int  bvh_batch_download(bvh_batch* batch, const bvh_batch_mesh* mesh, void* h_nodes, void* h_leaves);
void bvh_batch_destroy(bvh_batch* batch);

/* wait for everything enqueued on the ctx's stream (bvh_build is asynchronous unless it has to read something back:
 * profiling on, single-pass root index, PLOC++ iteration batches, collapse level counts; those read-backs are 4-byte
 * copies into pinned host words behind the build's launches on the in-order stream, and the call returns once the word
 * has landed — the host polls it, which notices the end of the build a few microseconds before hipStreamSynchronize does —
 * i.e. when every launch of the build has completed) */
int  bvh_ctx_synchronize(bvh_ctx* ctx);
/* the overflow words of the ctx's last query call (a scene's calls use its ctx's): how many queries the stack walks of its first (count) pass and of its fill
 * pass left to the stackless kernels; either pointer may be NULL.  Waits for the stream and reads 8 bytes back: for tests and diagnosis.  BVH_E_INVALID_ARG for
 * a NULL ctx or one that has never reserved its arena */
int  bvh_ctx_query_overflow(bvh_ctx* ctx, uint32_t* first_pass_out, uint32_t* fill_pass_out);

/* plain device-memory helpers so that hosts without a HIP binding (ctypes, cgo, JNI ...) can stage buffers */
int  bvh_dev_alloc(bvh_ctx* ctx, uint64_t bytes, void** out);
int  bvh_dev_free(bvh_ctx* ctx, void* p);
int  bvh_dev_upload(bvh_ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes);
int  bvh_dev_download(bvh_ctx* ctx, void* h_dst, const void* d_src, uint64_t bytes);
int  bvh_dev_copy(bvh_ctx* ctx, void* d_dst, const void* d_src, uint64_t bytes);   /* device->device, asynchronous on the ctx's stream */

const char* bvh_version(void);
/* ABI revision of this header (BVH_ABI_VERSION): bumped whenever a struct of this file changes size or an entry point changes signature, so that a host
 * compiled against an older header can refuse to run instead of handing the library a too-small bvh_result.  Revision 3: bvh_result carries d_tris and
 * d_morton_keys (88 bytes; round 2 grew it without a bump), bvh_ctx_set_option / bvh_ctx_get_option exist.  Revision 4: bvh_batch_report carries `meshes`
 * and `lanes_per_device` (56 bytes), bvh_batch_mesh / bvh_batch_download / bvh_stage_morton_plan exist. */
#define BVH_ABI_VERSION 4
uint32_t bvh_abi_version(void);
/* sizeof(bvh_result) / sizeof(bvh_timings) / sizeof(bvh_build_input) as the LIBRARY was compiled: out[0..2] */
void bvh_abi_struct_sizes(uint32_t out[3]);

#ifdef __cplusplus
}
#endif
#endif
