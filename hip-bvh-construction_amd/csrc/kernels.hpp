// kernels.hpp — host-side launch interface of the gfx950 kernels (internal; the public boundary is include/bvh_mi355x.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bvh/types.h"

namespace bvh {

// Optional per-kernel timing (bvh_ctx_set_profiling(ctx, 2)): launchers announce each kernel (or group of launches of one
// kernel) with a KernelScope; when a recorder is installed for the calling thread it records ONE hipEvent on the launch
// stream at that point.  The time between two consecutive marks is attributed to the earlier mark's name (kernel duration
// including its launch boundary) — half the events of a begin/end pair, which matters when a build is ~70 launches.
struct KernelRecorder {
    virtual void mark(hipStream_t s, const char* name) = 0;
    virtual ~KernelRecorder() {}
};
extern thread_local KernelRecorder* g_recorder;
struct KernelScope {
    KernelScope(hipStream_t stream, const char* name) { if (g_recorder) g_recorder->mark(stream, name); }
};

constexpr int EM_BLOCK = 256;
// what the build path's first kernel clears before it starts (the stand-alone sort entry point clears the same through sort_prepare / k_prepare)
struct PrepArgs { uint32_t* hist = nullptr; uint32_t hist_words = 0; uint4* status = nullptr; uint32_t status_vecs = 0; uint32_t* counters = nullptr;
                  uint32_t* extra = nullptr; uint32_t extra_words = 0;
                  // PLOC++ builds: the iteration bookkeeping of ploc_begin (look-back status words of every iteration, state words with counts[0] = n)
                  uint4* ploc_status = nullptr; uint32_t ploc_status_vecs = 0; uint64_t* ploc_tail = nullptr; uint32_t ploc_tail_words = 0;
                  uint32_t* ploc_state = nullptr; uint32_t ploc_count = 0; };
#ifdef BVH_ABLATION
constexpr int SORT_COUNTER_CLEAR = 64;      // (+ the look-back statistics of the measurement build)
#else
constexpr int SORT_COUNTER_CLEAR = 8;       // = SORT_MAX_PASSES tile tickets
#endif

// ---- stage E / M (stage_em.hip)
// reset_scene: launch the Aabb::reset of d_scene first (false when sort_prepare already did it)
void launch_extents(hipStream_t s, const void* d_tris, uint32_t n, void* d_boxes, void* d_scene, bool reset_scene = true, const PrepArgs* prep = nullptr);
void launch_extents_packed(hipStream_t s, const void* d_tris36, uint32_t n, void* d_boxes, void* d_scene, bool reset_scene = true, const PrepArgs* prep = nullptr);
void launch_extents_indexed(hipStream_t s, const void* d_vertices, const void* d_indices, uint32_t n_vertices, uint32_t n, void* d_boxes, void* d_scene, bool reset_scene = true, const PrepArgs* prep = nullptr);
// bvh_build_boxes' stage E: bvh_aabb[n] (device; may be d_boxes itself) copied into d_boxes and unioned into d_scene
void launch_extents_boxes(hipStream_t s, const void* d_in, uint32_t n, void* d_boxes, void* d_scene, bool reset_scene = true, const PrepArgs* prep = nullptr);
void launch_morton(hipStream_t s, const void* d_boxes, uint32_t n, const void* d_scene, uint32_t* d_keys, uint32_t* d_vals,
                   uint32_t* d_hist /*may be null*/, int hist_bits, int passes, float* d_reset_next = nullptr /* Aabb::reset of another extent (the next build's) */);
// extended Morton code with a 60-bit budget in u64 keys (total_bits = 30 reproduces launch_morton's codes: the parity pin)
void launch_morton64(hipStream_t s, const void* d_boxes, uint32_t n, const void* d_scene, uint64_t* d_keys, int total_bits,
                     uint32_t* d_hist /*may be null*/, int passes, float* d_reset_next = nullptr);

// the per-scene bit plan the Morton kernels derive from a scene extent, evaluated on the device: int[10] = {axis[3], bits[3], pre[2], pre_sum, swap}
void launch_morton_plan(hipStream_t s, const void* d_scene, int* d_out, int total_bits);

// ---- stage S (sort.hip): one-sweep LSD radix sort, SORT_BITS-bit digits
constexpr int SORT_BITS = 8;
constexpr int SORT_RADIX = 1 << SORT_BITS;
constexpr int SORT_BLOCK = 256;
#ifndef BVH_SORT_IPT
#define BVH_SORT_IPT 12
#endif
constexpr int SORT_IPT = BVH_SORT_IPT;                        // keys per thread
constexpr int SORT_TILE = SORT_BLOCK * SORT_IPT;              // keys per workgroup (sizes the status rows)
constexpr int SORT_IPT_WIDE = 20;                            // keys per thread for large inputs
#ifndef BVH_SORT_WIDE_MIN_N
#define BVH_SORT_WIDE_MIN_N 1000000
#endif
constexpr uint32_t SORT_WIDE_MIN_N = BVH_SORT_WIDE_MIN_N;
constexpr int SORT_MAX_PASSES = 8;                          // 8 digits: 64-bit keys
static_assert(SORT_COUNTER_CLEAR >= SORT_MAX_PASSES, "the build path's first kernel clears the tile tickets of every pass");
// The digit histograms exist in SORT_HIST_COPIES copies (copy c at hist + c * SORT_HIST_STRIDE): a producer workgroup flushes its counts
// into copy blockIdx % copies, a sort tile adds the copies up.  One address takes ~90 atomics/us on this chip: 2048 workgroups flushing
// into ONE copy spent 23 us queueing on every bin (k_morton 88 us at 10 M, of which the stream is 45); with 16 copies it is 1.5 us.
constexpr int SORT_HIST_COPIES = 16;
constexpr int SORT_HIST_STRIDE = SORT_MAX_PASSES * (1 << SORT_BITS);
// The build's u32 sort runs on key bits [0, 30) (8/8/8/6).  The extended Morton code is the reference's unsigned wrap-around arithmetic
// (src/CommonBlocksKernel.h:252-356) and does NOT stay below 2^30 on every scene (a planar scene with an axis ratio >= 2^32: ADVICE r04) — the reference sorts
// all 32 bits, so such keys must sort by them.  k_morton raises this word (row 4 of histogram copy 0: unused by a four-pass sort, cleared with the histograms)
// when a code has bit 30 or 31 set; the narrow last pass then returns at once and the 8-bit instantiation enqueued behind it (a no-op otherwise) does the pass.
constexpr int SORT_WIDE_FLAG_WORD = 4 * (1 << SORT_BITS);
struct SortScratch {
    void*     pairs0;        // interleaved {key,value} records of the intermediate passes, ping (8 B x n for u32 keys, 16 B x n for u64)
    void*     pairs1;        // pong
    uint32_t* hist;          // u32[SORT_HIST_COPIES * SORT_HIST_STRIDE]: per copy, per pass, per digit (zeroed by sort_prepare)
    uint32_t* status;        // u32[SORT_MAX_PASSES * tiles * SORT_RADIX] (zeroed by sort_prepare)
    uint32_t* counters;      // u32[SORT_MAX_PASSES]                 (zeroed by sort_prepare)
    int       test_knobs;    // BVH_OPT_SORT_TEST_KNOBS (8 | 32): forces the helping path; results unchanged
};
inline uint32_t sort_tiles(uint32_t n) { return (n + SORT_TILE - 1) / SORT_TILE; }
inline int sort_passes(int start_bit, int end_bit) { return (end_bit - start_bit + SORT_BITS - 1) / SORT_BITS; }
size_t sort_status_bytes(uint32_t n);
// zero hist/status/counters for `passes` digits (must precede the histogram producer) — one launch that can also reset a scene
// extent (Aabb::reset) and zero one more small word array
void sort_prepare(hipStream_t s, const SortScratch& sc, uint32_t n, int passes, float* d_scene_reset = nullptr,
                  uint32_t* d_extra = nullptr, uint32_t extra_words = 0);
// hist_ready: sc.hist already holds the per-pass digit counts (fused into the Morton kernel); else a histogram kernel runs.
// gated_narrow_top (the build's u32 path only; needs hist_ready and the flag word maintained by k_morton): see SORT_WIDE_FLAG_WORD
void sort_pairs(hipStream_t s, const SortScratch& sc, const uint32_t* keys_in, const uint32_t* vals_in, uint32_t n,
                uint32_t* keys_out, uint32_t* vals_out, int start_bit, int end_bit, bool hist_ready, bool gated_narrow_top = false);
void sort_pairs64(hipStream_t s, const SortScratch& sc, const uint64_t* keys_in, const uint32_t* vals_in, uint32_t n,
                  uint64_t* keys_out, uint32_t* vals_out, int start_bit, int end_bit, bool hist_ready);

// ---- stage B (lbvh.hip, hploc.hip, ploc.hip)
// key_bits: 32 = u32 sorted keys (30-bit Morton codes, the reference), 64 = u64 sorted keys (60-bit codes)
// d_slots: u64[n] hand-off words, all-zero before the call and left all-zero (self-cleaning).  d_queue / d_queue_count: scratch of the
// tile scheduler used for large n (uint4[lbvh_queue_capacity(n)], u32[64 * 32]); pass d_queue = nullptr to force the one-launch kernel.
size_t lbvh_queue_capacity(uint32_t n);
void launch_lbvh_single(hipStream_t s, const void* d_boxes, const void* d_skeys, int key_bits, const uint32_t* d_svals, uint32_t n,
                        void* d_nodes, uint64_t* d_slots /*u64[n]*/, uint32_t* d_root, void* d_queue, size_t queue_capacity, uint32_t* d_queue_count,
                        bool heads_cleared = false /* d_queue_count is already zero */, int scheduler = 0 /* BVH_OPT_LBVH_SCHEDULER */);
// small inputs: k_karras + k_refit (d_parent u32[2n-1]; d_flags u32[n], all 0xFFFFFFFF before the call and left so); large inputs: the tile
// scheduler with the two-pass numbering (d_slots / d_root / d_queue / d_queue_count as for launch_lbvh_single)
void launch_lbvh_two(hipStream_t s, const void* d_boxes, const void* d_skeys, int key_bits, const uint32_t* d_svals, uint32_t n,
                     void* d_nodes, uint32_t* d_parent /*u32[2n-1]*/, uint32_t* d_flags /*u32[n]*/, uint64_t* d_slots, uint32_t* d_root,
                     void* d_queue, size_t queue_capacity, uint32_t* d_queue_count, bool heads_cleared = false, int scheduler = 0);
// HPLOC scratch (hploc.hip).  dep must be all-zero before a build and is left all-zero by a completed build.
struct HplocScratch {
    void*     recs;          // 32-byte survivor records {id, rep, box} x n
    uint64_t* dep;           // u64[n] dependency words {count:2 | R:30 | L:30}
    uint32_t* zero_parent;   // u32[1]
    uint32_t* queue_pc;      // u32[queue_capacity]   (block-local mode: nodes ready for k_hploc_ext)
    uint64_t* queue_rng;     // u64[queue_capacity]
    uint32_t* queue_count;   // u32[64 * 32]          (one padded head per sub-queue)
    size_t    queue_capacity;
    const void* leaf_tris = nullptr;   // build path, 64-byte triangles only: the emitters stage a leaf's box from its triangle (one aligned 64-byte line per
                                       // leaf) instead of from the 24-byte box array (a box straddles two 64-byte lines one time in four); nullptr: boxes
};
size_t hploc_queue_capacity(uint32_t n);
uint32_t hploc_block_tile();
uint32_t hploc_head_words();     // words of queue_count every build starts from zero (the build path's first kernel clears them)
void launch_hploc(hipStream_t s, const void* d_boxes, const void* d_skeys, int key_bits, const uint32_t* d_svals, uint32_t n,
                  void* d_nodes, void* d_leaves, const HplocScratch& sc);
void launch_hploc_block(hipStream_t s, const void* d_boxes, const void* d_skeys, int key_bits, const uint32_t* d_svals, uint32_t n,
                        void* d_nodes, void* d_leaves, const HplocScratch& sc, bool heads_cleared = false /* sc.queue_count is already zero */);
struct PlocScratch {
    void*     list0;         // 32-byte cluster entries {id, box} x n (ping)
    void*     list1;         // pong
    uint32_t* ids1;          // u32[n]
    uint64_t* status;        // u64[PLOC_MAX_ITERS * chunks]
    uint32_t* state;         // u32[PLOC_STATE_WORDS]
    bool      static_ids = true;   // grids of <= 256 workgroups take chunk = workgroup id (no ticket); false: tickets always (BVH_OPT_PLOC_SCHEDULER 1: hosts that share the device)
};
constexpr int PLOC_CHUNK = 1024;
constexpr int PLOC_MAX_ITERS = 96;
constexpr int PLOC_STATE_WORDS = 2 * PLOC_MAX_ITERS + 4;     // counts[MAX+1] | tickets[MAX] | iterations done | (spare)
inline uint32_t ploc_chunks(uint32_t n) { return (n + PLOC_CHUNK - 1) / PLOC_CHUNK; }
void ploc_begin(hipStream_t s, const PlocScratch& sc, uint32_t n);
void ploc_begin_prep(const PlocScratch& sc, uint32_t n, PrepArgs& prep);   // the same clearing as fields of the build path's first kernel (no launch)
void ploc_reset(hipStream_t s, const PlocScratch& sc, uint32_t n, uint32_t count);
// fresh: iteration `first` is the build's very first one — it reads d_svals / d_boxes and writes d_leaves (SetupClusters fused)
void ploc_enqueue(hipStream_t s, const PlocScratch& sc, uint32_t n, void* d_nodes, void* d_leaves, const void* d_boxes, const uint32_t* d_svals,
                  int first, int count, int parity, bool fresh);

// ---- refit (refit.hip): bvh_refit's two kernels after stage E.  parent: u32[2n-1] plan over {internal [0, n-1), leaf j at n-1+j}; flags: u32[n-1] exchange
// words, all-INVALID before the climb and left so.  layout 0: leaves are nodes n-1 .. 2n-2; layout 1: d_leaves = PrimRef[n]
void launch_refit_plan(hipStream_t s, const void* d_nodes, uint32_t n, uint32_t root, uint32_t* d_parent);
void launch_refit_climb(hipStream_t s, const void* d_prim_boxes, void* d_nodes, void* d_leaves, int layout, uint32_t n, const uint32_t* d_parent, uint32_t* d_flags);

// ---- partial refit (refit_subset.hip): bvh_refit_subset's kernels.  d_leaf_of_prim: u32[n], the leaf (sorted position) that holds each primitive, INVALID where none
// does — launch_refit_leafmap makes it from the leaf records.  d_owner: u32[n] per leaf, d_pending: u32[n-1] per internal node, all-zero before the launches and
// left so.  launch_refit_subset_boxes: k_refit_subset_boxes (claims each listed leaf once, stage E's box of its triangle into d_prim_boxes and the leaf record);
// launch_refit_subset_climb: k_refit_subset_mark + k_refit_subset_climb (the boxes of the ancestors, the root's box into d_scene).  Triangles: a validated
// bvh_build_input's fields, parent: the plan of launch_refit_plan
void launch_refit_leafmap(hipStream_t s, const void* d_nodes, const void* d_leaves, int layout, uint32_t n, uint32_t* d_leaf_of_prim);
void launch_refit_subset_boxes(hipStream_t s, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                               const uint32_t* d_prims, uint32_t n_dirty, const uint32_t* d_leaf_of_prim, uint32_t* d_owner, void* d_prim_boxes, void* d_nodes,
                               void* d_leaves, int layout, uint32_t n);
void launch_refit_subset_climb(hipStream_t s, const uint32_t* d_prims, uint32_t n_dirty, const uint32_t* d_leaf_of_prim, uint32_t* d_owner, uint32_t* d_pending,
                               const uint32_t* d_parent, const void* d_prim_boxes, void* d_nodes, const void* d_leaves, int layout, uint32_t n, uint32_t root,
                               void* d_scene);

// ---- tree optimisation (optimize.hip): one round of bvh_optimize's treelet restructuring (treelet roots: nodes with >= gamma leaves).  d_parent: the plan of
// launch_refit_plan, kept right (the rebuild rewrites the parents of what it moves); d_flags: u32[n-1] exchange words, all-INVALID before the launch and left so
void launch_optimize(hipStream_t s, void* d_nodes, const void* d_leaves, int layout, uint32_t n, uint32_t gamma, uint32_t* d_parent, uint32_t* d_flags);

// ---- ray queries (query.hip): bvh_intersect's two kernels.  k_intersect (short stack) and k_intersect_deep (stackless re-traversal of the rays it marked, through
// the parent plan of launch_refit_plan; returns at once while *d_overflow == 0).  d_overflow: one word, zeroed before the launch.  Triangles: a validated
// bvh_build_input's fields (tri_format, d_tris, d_vertices, d_indices, n_vertices)
void launch_intersect(hipStream_t s, int layout, int query, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                      const void* d_rays, uint32_t n_rays, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, void* d_hits,
                      uint32_t* d_overflow, const uint32_t* d_parent);

// ---- point queries (point_query.hip): bvh_closest_point's two kernels, arguments as launch_intersect's (d_points: bvh_point_query[n_points], d_hits:
// bvh_point_hit[n_points]).  k_closest_point (short stack) and k_closest_point_deep (stackless, returns at once while *d_overflow == 0)
void launch_closest_point(hipStream_t s, int layout, int query, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices,
                          uint32_t n_vertices, const void* d_points, uint32_t n_points, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root,
                          void* d_hits, uint32_t* d_overflow, const uint32_t* d_parent);

// ---- winding numbers (winding.hip).  launch_winding_prepare: k_winding_climb (the seven raw sums of every internal node into d_moments, bvh_winding_moment[n-1],
// through the parent plan of launch_refit_plan and the flags words of launch_refit_climb, all-INVALID before and left so) + k_winding_finish (first moment ->
// centre and radius).  launch_winding: k_winding (short stack; marks a query it leaves in d_w[i]) + k_winding_deep (stackless, returns at once while
// *d_overflow == 0); tree / triangle / point arguments as launch_closest_point's, d_w: f32[n_points]
void launch_winding_prepare(hipStream_t s, int layout, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                            const void* d_nodes, const void* d_leaves, uint32_t n, const uint32_t* d_parent, uint32_t* d_flags, void* d_moments);
void launch_winding(hipStream_t s, int layout, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                    const void* d_points, uint32_t n_points, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, const void* d_moments,
                    float beta, float* d_w, uint32_t* d_overflow, const uint32_t* d_parent);

// ---- k-nearest queries (knn.hip): bvh_knn's two kernels, arguments as launch_closest_point's (d_hits: bvh_knn_hit[n_points * k], query i's list at i * k;
// d_counts: u32[n_points] or null; 1 <= k <= KNN_MAX_K).  k_knn (short stack, marks a query it leaves in d_hits[i * k].prim_idx) and k_knn_deep (stackless,
// returns at once while *d_overflow == 0)
constexpr int KNN_MAX_K = 32;                                // BVH_KNN_MAX_K (knn.hip asserts it): the largest list bucket
void launch_knn(hipStream_t s, int layout, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                const void* d_points, uint32_t n_points, uint32_t k, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, void* d_hits,
                uint32_t* d_counts, uint32_t* d_overflow, const uint32_t* d_parent);

// ---- box queries (overlap.hip): bvh_overlap's kernels.  launch_overlap_count: k_overlap_count (short stack; d_offsets[i] = query i's count) + k_overlap_deep
// (stackless, returns at once while *d_overflow == 0) + k_overlap_scan (two launches: the counts become u32[n_boxes + 1] offsets in place, saturated at
// 0xFFFFFFFF, and *d_total the 64-bit total; d_sums: u64[OVERLAP_SCAN_BLOCKS] scratch).  launch_overlap_fill: k_overlap_fill + k_overlap_deep, which return at
// once unless *d_total <= capacity and *d_total < 2^32; query i's primitives go to d_prims[d_offsets[i] ..].  Each pass has an overflow word of its own, zeroed
// before the launches.  mode: bvh_overlap_mode
constexpr uint32_t OVERLAP_SCAN_BLOCKS = 1024;
void launch_overlap_count(hipStream_t s, int layout, int mode, const void* d_boxes, uint32_t n_boxes, const void* d_nodes, const void* d_leaves, uint32_t n,
                          uint32_t root, uint32_t* d_offsets, uint32_t* d_overflow, const uint32_t* d_parent, uint64_t* d_sums, uint64_t* d_total);
void launch_overlap_fill(hipStream_t s, int layout, int mode, const void* d_boxes, uint32_t n_boxes, const void* d_nodes, const void* d_leaves, uint32_t n,
                         uint32_t root, uint32_t* d_offsets, uint32_t* d_prims, uint64_t capacity, const uint64_t* d_total, uint32_t* d_overflow,
                         const uint32_t* d_parent);
// the scan alone (launch_overlap_count ends with it): d_offsets' n_boxes counts become n_boxes + 1 offsets in place, *d_total the 64-bit total
void launch_overlap_scan(hipStream_t s, uint32_t* d_offsets, uint32_t n_boxes, uint64_t* d_sums, uint64_t* d_total);

// ---- convex-volume queries (cull.hip): bvh_cull's kernels.  d_planes: float[n_volumes][planes][4].  group false: k_cull_walk (one volume per lane, short stack);
// group true: k_cull_group (one volume per workgroup of CULL_GROUP_BLOCK threads, LDS work stack of BVH_CULL_GROUP_STACK entries).  Either marks a volume it
// cannot finish and k_cull_deep (stackless, returns at once while *d_overflow == 0) redoes it.  launch_cull_count ends with launch_overlap_scan;
// launch_cull_fill's kernels return at once unless *d_total <= capacity and *d_total < 2^32; volume i's bvh_cull_hit records go to d_hits[d_offsets[i] ..].
// Each pass has an overflow word of its own, zeroed before the launches
constexpr int CULL_GROUP_BLOCK = 256;
constexpr uint32_t CULL_AUTO_MAX_VOLUMES = 65536;            // BVH_CULL_AUTO takes the group walk iff n_volumes <= this (the largest count measured: the group walk won there) ...
constexpr uint32_t CULL_AUTO_MIN_LEAVES = 1024;              // ... and n_leaves >= this
void launch_cull_count(hipStream_t s, int layout, bool group, const float* d_planes, uint32_t n_volumes, uint32_t planes, const void* d_nodes,
                       const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, uint32_t* d_overflow, const uint32_t* d_parent, uint64_t* d_sums,
                       uint64_t* d_total);
void launch_cull_fill(hipStream_t s, int layout, bool group, const float* d_planes, uint32_t n_volumes, uint32_t planes, const void* d_nodes,
                      const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, void* d_hits, uint64_t capacity, const uint64_t* d_total,
                      uint32_t* d_overflow, const uint32_t* d_parent);

// ---- crossing triangle pairs (intersect_tris.hip): bvh_intersect_tris' kernels.  A TrisMesh is one triangle array in a bvh_tri_format (device pointers);
// tree_tris: the tree's triangles, queries: the other mesh's (self mode: the same array).  launch_tris_count: k_tris_count (short stack; d_offsets[i] = the number
// of tree triangles query triangle i crosses) + k_tris_deep (stackless, returns at once while *d_overflow == 0) + launch_overlap_scan.  launch_tris_fill:
// k_tris_fill + k_tris_deep, which return at once unless *d_total <= capacity and *d_total < 2^32; query i's primitives go to d_prims[d_offsets[i] ..].  Each pass
// has an overflow word of its own, zeroed before the launches.  mode: bvh_tris_mode
struct TrisMesh { int tri_format; const void* d_tris; const void* d_vertices; const void* d_indices; uint32_t n_vertices; };
void launch_tris_count(hipStream_t s, int layout, int mode, const TrisMesh& tree_tris, const TrisMesh& queries, uint32_t n_queries, const void* d_nodes,
                       const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, uint32_t* d_overflow, const uint32_t* d_parent, uint64_t* d_sums,
                       uint64_t* d_total);
void launch_tris_fill(hipStream_t s, int layout, int mode, const TrisMesh& tree_tris, const TrisMesh& queries, uint32_t n_queries, const void* d_nodes,
                      const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, uint32_t* d_prims, uint64_t capacity, const uint64_t* d_total,
                      uint32_t* d_overflow, const uint32_t* d_parent);

// ---- mesh-to-mesh distance (closest_tris.hip): bvh_closest_tris's two kernels.  tree_tris / queries as launch_tris_count's; d_hits: bvh_tri_hit[n_queries];
// radius: the call's one bound.  k_closest_tris (short stack, marks a query it leaves in d_hits[i].prim_idx) and k_closest_tris_deep (stackless, returns at once
// while *d_overflow == 0)
void launch_closest_tris(hipStream_t s, int layout, int query, const TrisMesh& tree_tris, const TrisMesh& queries, uint32_t n_queries, float radius,
                         const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, void* d_hits, uint32_t* d_overflow, const uint32_t* d_parent);

// ---- every triangle within a radius, mesh to mesh (radius_tris.hip): bvh_radius_tris's kernels.  tree_tris / queries as launch_tris_count's (self mode: the
// same mesh twice); flags: the call's BVH_RADIUS_TRIS_* bits; radius: the call's one bound.  launch_radius_tris_count: k_radius_tris_walk (short stack;
// d_offsets[i] = query triangle i's number of accepted candidates) + k_radius_tris_deep (stackless, returns at once while *d_overflow == 0) +
// launch_overlap_scan.  launch_radius_tris_fill: the same two kernels' fill forms, which return at once unless *d_total <= capacity and *d_total < 2^32; query
// i's bvh_tri_hit records go to d_hits[d_offsets[i] ..], in ascending (dist2, prim) order with BVH_RADIUS_TRIS_SORTED.  Each pass has an overflow word of its
// own, zeroed before the launches
void launch_radius_tris_count(hipStream_t s, int layout, uint32_t flags, const TrisMesh& tree_tris, const TrisMesh& queries, uint32_t n_queries, float radius,
                              const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, uint32_t* d_overflow,
                              const uint32_t* d_parent, uint64_t* d_sums, uint64_t* d_total);
void launch_radius_tris_fill(hipStream_t s, int layout, uint32_t flags, const TrisMesh& tree_tris, const TrisMesh& queries, uint32_t n_queries, float radius,
                             const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, void* d_hits, uint64_t capacity,
                             const uint64_t* d_total, uint32_t* d_overflow, const uint32_t* d_parent);

// ---- all-hits ray queries (multihit.hip): bvh_intersect_all's kernels, tree / triangle / ray arguments as launch_intersect's.  launch_hits_count: k_hits_count
// (short stack; d_offsets[i] = ray i's number of accepted hits) + k_hits_deep (stackless, returns at once while *d_overflow == 0) + launch_overlap_scan.
// launch_hits_fill: k_hits_fill + k_hits_deep, which return at once unless *d_total <= capacity and *d_total < 2^32; ray i's bvh_hit records go to
// d_hits[d_offsets[i] ..], in ascending (t, prim) order when sorted != 0.  Each pass has an overflow word of its own, zeroed before the launches
void launch_hits_count(hipStream_t s, int layout, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                       const void* d_rays, uint32_t n_rays, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets,
                       uint32_t* d_overflow, const uint32_t* d_parent, uint64_t* d_sums, uint64_t* d_total);
void launch_hits_fill(hipStream_t s, int layout, int tri_format, int sorted, const void* d_tris, const void* d_vertices, const void* d_indices,
                      uint32_t n_vertices, const void* d_rays, uint32_t n_rays, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root,
                      uint32_t* d_offsets, void* d_hits, uint64_t capacity, const uint64_t* d_total, uint32_t* d_overflow, const uint32_t* d_parent);

// ---- radius searches (radius.hip): bvh_radius_search's kernels, tree / triangle / point arguments as launch_closest_point's.  launch_radius_count:
// k_radius_count (short stack; d_offsets[i] = query i's number of accepted candidates) + k_radius_deep (stackless, returns at once while *d_overflow == 0) +
// launch_overlap_scan.  launch_radius_fill: k_radius_fill + k_radius_deep, which return at once unless *d_total <= capacity and *d_total < 2^32; query i's
// bvh_knn_hit records go to d_hits[d_offsets[i] ..], in ascending (dist2, prim) order when sorted != 0.  Each pass has an overflow word of its own, zeroed
// before the launches
void launch_radius_count(hipStream_t s, int layout, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                         const void* d_points, uint32_t n_points, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets,
                         uint32_t* d_overflow, const uint32_t* d_parent, uint64_t* d_sums, uint64_t* d_total);
void launch_radius_fill(hipStream_t s, int layout, int tri_format, int sorted, const void* d_tris, const void* d_vertices, const void* d_indices,
                        uint32_t n_vertices, const void* d_points, uint32_t n_points, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root,
                        uint32_t* d_offsets, void* d_hits, uint64_t capacity, const uint64_t* d_total, uint32_t* d_overflow, const uint32_t* d_parent);

// ---- early split clipping (split.hip): bvh_split_refs' kernels, triangle arguments as launch_intersect's.  launch_split_count: k_split_count (d_offsets[p] =
// triangle p's number of references; triangles a wave will fill are appended to d_heavy_list, u32[n], counted in *d_heavy_count, zeroed before the launch) +
// launch_overlap_scan.  launch_split_fill: k_split_fill (one triangle per lane) + k_split_heavy (one listed triangle per wave), which return at once unless
// *d_total <= capacity and *d_total < 2^32; triangle p's references go to d_ref_boxes / d_ref_prims [d_offsets[p] ..].  launch_remap_leaves: bvh_remap_leaves' kernel
constexpr uint32_t SPLIT_HEAVY_BLOCKS = 1024;
void launch_split_count(hipStream_t s, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices, uint32_t n,
                        float sa_max, uint32_t max_depth, uint32_t* d_offsets, uint32_t* d_heavy_list, uint32_t* d_heavy_count, uint64_t* d_sums,
                        uint64_t* d_total);
void launch_split_fill(hipStream_t s, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices, uint32_t n,
                       float sa_max, uint32_t max_depth, const uint32_t* d_offsets, void* d_ref_boxes, uint32_t* d_ref_prims, uint64_t capacity,
                       const uint64_t* d_total, const uint32_t* d_heavy_list, const uint32_t* d_heavy_count);
void launch_remap_leaves(hipStream_t s, void* d_nodes, void* d_leaves, int layout, uint32_t n, const uint32_t* d_map, uint32_t n_map);

// ---- batched small-mesh builds (many.hip): bvh_build_many's kernels.  ManyArgs: the validated input (a bvh_build_input's fields) and the output arrays of a
// bvh_many_out (skeys / svals may be null).  launch_many: k_many_wave (meshes of at most 64 triangles, one wave each) and k_many_block (at most 128 / 256 /
// MANY_MAX triangles, one workgroup each) over d_items, uint4 {first, count, out_off, mesh} records binned by size class: n_class[0..3] of each, in that order.
// karras: the two-pass builder's node numbering instead of the single-pass one (lbvh.hip)
constexpr int MANY_MAX = 512;                                // BVH_MANY_LDS_MAX_PRIMS (api.hip asserts it)
struct ManyArgs { const void* tris; const void* verts; const void* idx; uint32_t n_verts; bvh_aabb* boxes; bvh_aabb* scenes; bvh2_node* nodes; uint32_t* roots;
                  uint32_t* skeys; uint32_t* svals; };
void launch_many(hipStream_t s, const ManyArgs& a, int tri_format, bool karras, const void* d_items, const uint32_t n_class[4]);
// ... and bvh_build_many_ploc's (many_ploc.hip): k_many_ploc_wave / k_many_ploc_block over the same item records; nodes = Bvh2Node[total - n_meshes] (mesh m's
// n - 1 records from record out_off - m, root = local node 0), leaves = PrimRef[total]
struct ManyPlocArgs { const void* tris; const void* verts; const void* idx; uint32_t n_verts; bvh_aabb* boxes; bvh_aabb* scenes; bvh2_node* nodes; bvh_primref* leaves;
                      uint32_t* skeys; uint32_t* svals; };
void launch_many_ploc(hipStream_t s, const ManyPlocArgs& a, int tri_format, const void* d_items, const uint32_t n_class[4]);

// ---- instanced scenes (scene.hip): bvh_scene's kernels.  SceneBlas: the device copy of one validated bvh_blas (64 bytes, read whole when a ray enters an
// instance); tris = Triangle[n] / float[9n] / the vertices of INDEXED input, idx = INDEXED indices, parent = the BLAS's k_refit_plan plan (u32[2n-1]).
struct SceneBlas { const void* nodes; const void* leaves; const void* tris; const void* idx; const uint32_t* parent; uint32_t n, root, layout, fmt, nv, pad; };
static_assert(sizeof(SceneBlas) == 64, "SceneBlas is one 64-byte record");
// per instance, written by k_instance_boxes: world-to-object 3x4 (row-major, f32), the BLAS index (BVH_INVALID: inactive, never entered) and, in pad[0], the
// bits of the f32 scale bound s2 of bvh_scene_closest_point (0 for an inactive instance)
struct SceneInst { float w2o[12]; uint32_t blas, pad[3]; };
static_assert(sizeof(SceneInst) == 64, "SceneInst is one 64-byte record");
struct SceneQuery {
    const void* rays; void* hits; uint32_t* overflow;           // bvh_ray[n_rays], bvh_instance_hit[n_rays], one word zeroed before the launch
                                                                // (point queries: bvh_point_query[n_rays], bvh_instance_point_hit[n_rays])
    const void* tnodes; const void* tleaves; const uint32_t* tparent;   // top-level tree (n_inst >= 2) and its plan
    const SceneInst* inst; const SceneBlas* blas; const void* wbox;      // SceneInst[n_inst], SceneBlas[n_blas], bvh_aabb[n_inst]
    uint32_t n_rays, n_inst, troot, tlayout;
    const void* inst_in;                                        // bvh_instance[n_inst], the caller's records: the forward matrices (point queries only)
    uint32_t* counts = nullptr; uint32_t k = 0, pad = 0;        // bvh_scene_knn only (appended: the other kernels never read them): hits =
                                                                // bvh_instance_knn_hit[n_rays * k], counts = u32[n_rays] or null, 1 <= k <= KNN_MAX_K
};
// one thread per instance: inverse, active flag and world box from d_instances (bvh_instance[n_inst]) and the BLASes' root boxes
void launch_instance_boxes(hipStream_t s, const void* d_instances, uint32_t n_inst, const SceneBlas* d_blas, uint32_t n_blas, SceneInst* d_inst, void* d_wbox);
// k_scene_intersect (short stack shared by both levels) + k_scene_intersect_deep (stackless, returns at once while *overflow == 0)
void launch_scene_intersect(hipStream_t s, int query, const SceneQuery& q);
// k_scene_closest_point (short stack shared by both levels) + k_scene_closest_point_deep (stackless, returns at once while *overflow == 0); scene_point.hip
void launch_scene_closest_point(hipStream_t s, int query, const SceneQuery& q);
// k_scene_knn<8 / 16 / 32 by q.k> (k_scene_closest_point's walk, the list in LDS beside the stack; marks a query it leaves in hits[i * k].prim_idx) +
// k_scene_knn_deep (stackless, returns at once while *overflow == 0); scene_knn.hip
void launch_scene_knn(hipStream_t s, const SceneQuery& q);
// bvh_scene_intersect_all's extra arguments (scene_multihit.hip), beside a SceneQuery whose hits field is unused and whose overflow word is the pass's own:
// offsets = u32[n_rays + 1] (the count pass's counts, then the scan's offsets), hits = bvh_instance_hit[capacity] (fill pass), total = the scan's 64-bit total
struct SceneHits { uint32_t* offsets; void* hits; const uint64_t* total; uint64_t capacity; };
// k_scene_hits_count (short stack shared by both levels; offsets[i] = ray i's number of accepted hits) + k_scene_hits_deep (stackless, returns at once while
// *q.overflow == 0) + launch_overlap_scan.  launch_scene_hits_fill: k_scene_hits_fill + k_scene_hits_deep, which return at once unless *h.total <= h.capacity
// and *h.total < 2^32; ray i's records go to hits[offsets[i] ..], in ascending (t, instance, prim) order when sorted != 0.  Each pass has an overflow word of
// its own, zeroed before the launches
void launch_scene_hits_count(hipStream_t s, const SceneQuery& q, const SceneHits& h, uint64_t* d_sums, uint64_t* d_total);
void launch_scene_hits_fill(hipStream_t s, int sorted, const SceneQuery& q, const SceneHits& h);
// bvh_scene_radius_search (scene_radius.hip): the same two calls over point queries, with hits = bvh_instance_knn_hit[capacity].  k_scene_radius_count +
// k_scene_radius_deep + launch_overlap_scan; launch_scene_radius_fill: k_scene_radius_fill + k_scene_radius_deep, which return at once unless
// *h.total <= h.capacity and *h.total < 2^32; query i's records go to hits[offsets[i] ..], in ascending (dist2, instance, prim) order when sorted != 0
void launch_scene_radius_count(hipStream_t s, const SceneQuery& q, const SceneHits& h, uint64_t* d_sums, uint64_t* d_total);
void launch_scene_radius_fill(hipStream_t s, int sorted, const SceneQuery& q, const SceneHits& h);
// bvh_scene_overlap (scene_overlap.hip): the same two calls over query boxes (q.rays = bvh_aabb[n_rays]), with hits = bvh_instance_prim[capacity].
// k_scene_overlap_count + k_scene_overlap_deep + launch_overlap_scan; launch_scene_overlap_fill: k_scene_overlap_fill + k_scene_overlap_deep, which return at
// once unless *h.total <= h.capacity and *h.total < 2^32; query i's records go to hits[offsets[i] ..], in ascending (instance, prim) order when sorted != 0
void launch_scene_overlap_count(hipStream_t s, const SceneQuery& q, const SceneHits& h, uint64_t* d_sums, uint64_t* d_total);
void launch_scene_overlap_fill(hipStream_t s, int sorted, const SceneQuery& q, const SceneHits& h);
// bvh_scene_cull (scene_cull.hip): the same two calls over convex volumes (q.rays = float[n_rays][planes][4], WORLD space), with hits =
// bvh_scene_cull_hit[capacity].  group false: k_scene_cull_walk (one volume per lane, the short stack shared by both levels); group true: k_scene_cull_group (one
// volume per workgroup of CULL_GROUP_BLOCK threads, LDS work stack of BVH_SCENE_CULL_GROUP_STACK {instance, node} entries; max_pops bounds its expansions on
// arrays that are not a tree).  Either marks a volume it cannot finish and k_scene_cull_deep (stackless, returns at once while *q.overflow == 0) redoes it.
// launch_scene_cull_count ends with launch_overlap_scan; launch_scene_cull_fill's kernels return at once unless *h.total <= h.capacity and *h.total < 2^32
constexpr uint32_t SCENE_CULL_AUTO_MAX_VOLUMES = CULL_AUTO_MAX_VOLUMES;   // BVH_CULL_AUTO on a scene takes the group walk iff n_volumes <= this (bvh_cull's measured value) ...
constexpr uint32_t SCENE_CULL_AUTO_MIN_LEAVES = 1024;                     // ... and n_instances + the largest BLAS's n_leaves >= this (carried over from bvh_cull: DESIGN.md §8zc)
void launch_scene_cull_count(hipStream_t s, bool group, const SceneQuery& q, const SceneHits& h, uint32_t planes, uint64_t max_pops, uint64_t* d_sums,
                             uint64_t* d_total);
void launch_scene_cull_fill(hipStream_t s, bool group, const SceneQuery& q, const SceneHits& h, uint32_t planes, uint64_t max_pops);
// bvh_scene_intersect_tris (scene_tris.hip): the same two calls over query triangles (q.rays is unused), with hits = bvh_instance_prim[capacity].  SceneTris is
// the query side: the caller's world-space mesh (mode BVH_SCENE_TRIS_QUERY) or the instance whose world triangles ask (BVH_SCENE_TRIS_INSTANCE; queries unused).
// k_scene_tris_count + k_scene_tris_deep + launch_overlap_scan; launch_scene_tris_fill: k_scene_tris_fill + k_scene_tris_deep, which return at once unless
// *h.total <= h.capacity and *h.total < 2^32; query i's records go to hits[offsets[i] ..], in ascending (instance, prim) order when sorted != 0
struct SceneTris { TrisMesh queries; int mode; uint32_t query_instance; };
void launch_scene_tris_count(hipStream_t s, const SceneQuery& q, const SceneHits& h, const SceneTris& t, uint64_t* d_sums, uint64_t* d_total);
void launch_scene_tris_fill(hipStream_t s, int sorted, const SceneQuery& q, const SceneHits& h, const SceneTris& t);
// bvh_scene_closest_tris (scene_closest_tris.hip): q.rays is unused, q.hits = bvh_instance_tri_hit[q.n_rays]; t as for launch_scene_tris_count; radius: the call's
// one bound.  k_scene_closest_tris (short stack shared by both levels, marks a query it leaves in hits[i].prim_idx) + k_scene_closest_tris_deep (stackless,
// returns at once while *q.overflow == 0)
void launch_scene_closest_tris(hipStream_t s, int query, float radius, const SceneQuery& q, const SceneTris& t);
// bvh_scene_radius_tris (scene_radius_tris.hip): launch_scene_tris_count's two calls with bvh_scene_closest_tris's candidates (q.rays is unused), with hits =
// bvh_instance_tri_hit[capacity]; radius: the call's one bound.  k_scene_radius_tris_walk + k_scene_radius_tris_deep + launch_overlap_scan;
// launch_scene_radius_tris_fill: the same two kernels' fill forms, which return at once unless *h.total <= h.capacity and *h.total < 2^32; query i's records
// go to hits[offsets[i] ..], in ascending (dist2, instance, prim) order when sorted != 0
void launch_scene_radius_tris_count(hipStream_t s, float radius, const SceneQuery& q, const SceneHits& h, const SceneTris& t, uint64_t* d_sums, uint64_t* d_total);
void launch_scene_radius_tris_fill(hipStream_t s, int sorted, float radius, const SceneQuery& q, const SceneHits& h, const SceneTris& t);
// bvh_scene_collide (scene_collide.hip): every instance's triangles ask at once (q.rays is unused, q.n_rays = row_capacity), with hits = bvh_instance_prim[capacity].
// SceneCollide is the row table: d_row_first = the caller's u32[n_inst + 1], d_n_rows = a scratch u64 of its own (it must survive the count pass's scan, which
// writes the query total elsewhere), both = BVH_SCENE_COLLIDE_BOTH.  launch_scene_collide_rows: k_scene_collide_rows (one thread per instance: n_leaves of its
// BLAS, 0 if inactive) + launch_overlap_scan over them, which leaves row_first and *d_n_rows.  launch_scene_collide_count: k_scene_collide_count +
// k_scene_collide_deep + launch_overlap_scan; launch_scene_collide_fill: k_scene_collide_fill + k_scene_collide_deep, which return at once unless
// *h.total <= h.capacity and *h.total < 2^32; row r's records go to hits[offsets[r] ..], in ascending (instance, prim) order when sorted != 0.  Every kernel of
// the two passes answers "no records" when *d_n_rows > q.n_rays
struct SceneCollide { uint32_t* d_row_first; uint64_t* d_n_rows; int both; };
void launch_scene_collide_rows(hipStream_t s, const SceneQuery& q, const SceneCollide& c, uint64_t* d_sums);
void launch_scene_collide_count(hipStream_t s, const SceneQuery& q, const SceneHits& h, const SceneCollide& c, uint64_t* d_sums, uint64_t* d_total);
void launch_scene_collide_fill(hipStream_t s, int sorted, const SceneQuery& q, const SceneHits& h, const SceneCollide& c);
// bvh_scene_winding_prepare / bvh_scene_winding_number (scene_winding.hip), beside a SceneQuery (rays = bvh_point_query[n_rays], hits = f32[n_rays]).  SceneWind is
// the scene's winding memory: first = u32[n_blas + 1], the exclusive sum of the BLASes' leaf counts (BLAS b's exchange words are flags[first[b] ..
// first[b + 1]), its n - 1 moments start at bmom + (first[b] - b)); flags all-INVALID before and left so; maps / imom per instance, tmom = the top-level
// tree's n_inst - 1 records.  launch_scene_winding_blas: k_scene_winding_climb + k_scene_winding_finish over ALL BLASes (two launches whatever n_blas is).
// launch_scene_winding_top: k_scene_winding_inst, then (n_inst >= 2) the same two kernels' top-level forms on the top-level plan and d_tflags (u32[n_inst],
// all-INVALID before and left so).  launch_scene_winding: k_scene_winding (short stack shared by both levels; marks a query it leaves in hits[i]) +
// k_scene_winding_deep (stackless, returns at once while *q.overflow == 0)
struct SceneWind {
    const uint32_t* first; uint32_t* flags; bvh_winding_moment* bmom; bvh_winding_map* maps; bvh_winding_moment* imom; bvh_winding_moment* tmom;
    uint32_t n_blas, total_leaves;
};
void launch_scene_winding_blas(hipStream_t s, const SceneQuery& q, const SceneWind& w);
void launch_scene_winding_top(hipStream_t s, const SceneQuery& q, const SceneWind& w, uint32_t* d_tflags);
void launch_scene_winding(hipStream_t s, const SceneQuery& q, const SceneWind& w, float beta);

// ---- BVH2 -> BVH4 collapse (collapse.hip)
constexpr int COLLAPSE_MAX_BATCH = 64;                       // levels per batch of launches (one counter word per level)
constexpr int COLLAPSE_STATE_WORDS = COLLAPSE_MAX_BATCH;
void collapse_begin(hipStream_t s, uint2* d_taskq, uint32_t* d_state, uint32_t root, bool with_root);
void collapse_enqueue(hipStream_t s, const void* d_nodes, const void* d_leaves, void* d_wide, void* d_prims, uint2* d_taskq,
                      uint32_t* d_state, uint32_t base_begin, uint32_t base_len, int count, uint32_t n, int layout,
                      const uint32_t* expect = nullptr /* count words: the levels' task counts of the previous same-size collapse (grid sizing only) */);

// ---- consumer side (trace.hip)
void launch_generate_rays(hipStream_t s, const void* d_cam, void* d_rays, uint32_t width, uint32_t height);
void launch_trace_while(hipStream_t s, const void* d_rays, const void* d_tris, const void* d_nodes, const void* d_xf, void* d_rgba,
                        uint32_t root, uint32_t width, uint32_t height, uint32_t n_internal);

// kind: 1 restart trail, 2 if-if, 3 speculative while-while; d_counter (optional): triangle tests per ray
void launch_trace_kind(hipStream_t s, int kind, const void* d_rays, const void* d_tris, const void* d_nodes, const void* d_xf, void* d_rgba,
                       uint32_t* d_counter, uint32_t root, uint32_t width, uint32_t height, uint32_t n_internal);

// ---- helpers (misc.hip)
void launch_to_lbvh_layout(hipStream_t s, const void* d_nodes, const void* d_leaves, uint32_t n, void* d_out);
void launch_copy_bytes(hipStream_t s, void* d_dst, const void* d_src, size_t bytes);
// na words at d_a, then nb words at d_b (either may be empty), written as pairs {v, ~v} into 2 (na + nb) device-accessible pinned host words
void launch_readback(hipStream_t s, const uint32_t* d_a, uint32_t na, const uint32_t* d_b, uint32_t nb, uint32_t* pinned_pairs);      // device-to-device copy as a kernel (no runtime copy path)
void launch_sah_cost(hipStream_t s, const void* d_nodes, const void* d_leaves, uint32_t root, uint32_t n, int layout, double* d_out /*[1], zeroed inside*/);

void launch_bvh4_cost(hipStream_t s, const void* d_wide, uint32_t n_wide, const void* d_prims, const void* d_prim_boxes, uint32_t n, double* d_out /*[1], zeroed inside*/);
void launch_checksum(hipStream_t s, const void* d_nodes, uint32_t n_nodes, const void* d_leaves /*may be null*/, uint32_t n_leaves, uint32_t root, uint64_t* d_out /*[1], zeroed inside*/);

// one kernel of each translation unit of the build path is touched (hipFuncGetAttributes): the runtime loads that unit's code object now instead of at its first launch
void warm_stage_em(); void warm_sort(); void warm_lbvh(); void warm_hploc(); void warm_ploc(); void warm_misc(); void warm_collapse(); void warm_refit(); void warm_refit_subset(); void warm_query(); void warm_optimize(); void warm_scene(); void warm_scene_point(); void warm_scene_knn(); void warm_scene_multihit(); void warm_scene_radius(); void warm_scene_overlap(); void warm_scene_cull(); void warm_scene_tris(); void warm_scene_closest_tris(); void warm_scene_radius_tris(); void warm_scene_collide(); void warm_scene_winding(); void warm_point_query(); void warm_winding(); void warm_overlap(); void warm_tris(); void warm_closest_tris(); void warm_knn(); void warm_multihit(); void warm_radius(); void warm_radius_tris(); void warm_split(); void warm_many(); void warm_many_ploc();

} // namespace bvh
