// split.hip — bvh_split_refs on gfx950: early split clipping (reference Utility::doEarlySplitClipping, src/Utility.cpp:456-538, a host std::queue there) as a
// count -> scan -> fill device pass, and bvh_remap_leaves, the relabelling of a tree built over the references.
// A triangle's references are the leaves of its SPLIT TREE: the root is stage E's box of the triangle; a box whose Aabb::area exceeds sa_max is cut at its centre
// on its longest axis (Aabb::maximumExtentDim) into a left half (max = c) and a right half (min = c), unless the depth cap is reached or the cut makes no progress
// (include/bvh_mi355x.h states the rule operation for operation).  Output order: triangles in index order, a triangle's references depth-first, left first.
//   split_walk     : one lane walks one (sub)tree without a stack of boxes: going down replaces ONE plane of the box, so the lane keeps the replaced plane per
//                    level in LDS (16 floats per lane, 4 KiB per wave), the axis of every level in a dims word (2 bits each) and the side it is on in a path
//                    word.  Left child done: the saved max comes back, the cut becomes the min, the slot takes the parent's min; right child done: the slot
//                    restores the parent's min.  Count and fill are the same walk.
//   k_split_count  : one triangle per lane from the root; d_offsets[p] = its count.  Triangles with more than SPLIT_HEAVY_MIN references are appended to the
//                    heavy list (ballot + one atomic per wave; the list's order does not reach the output).
//   k_split_fill   : the light triangles, one per lane, into their slices.  A heavy triangle's lane returns at once.
//   k_split_heavy  : one WAVE per heavy triangle (one scene-sized triangle at depth 16 is 65 536 references).  Lane l owns the subtree whose depth-6 path is l,
//                    first level in the most significant bit, so lane order is depth-first order; a leaf above depth 6 belongs to the lane whose remaining path
//                    bits are zero and the other lanes below it idle.  Every lane replays its at most 6 cuts from the root box, counts its subtree, a wave
//                    exclusive scan of the counts gives its write offset, and it walks again and writes: at most 2^(max_depth - 6) references of serial work.
// The same f32 expressions evaluated in the same order on the same box give the same bits whichever kernel, lane or pass evaluates them, so count and fill agree
// and the bytes do not depend on the path that served a triangle.  The scan and the total word are bvh_overlap's (launch_overlap_scan); both fill kernels decide
// ON THE DEVICE whether they run.  A fill lane never writes outside its triangle's slice.
// Compiled WITHOUT -fno-honor-nans (Makefile default): stage E's clamp of NaN and infinity and the NaN-emits-at-once rule must not be folded away.
#include <type_traits>
#include "common.hpp"
#include "kernels.hpp"
#include "bvh_mi355x.h"

namespace bvh {

constexpr int SPLIT_BLOCK = 256;
constexpr int SPLIT_LEVELS = BVH_SPLIT_MAX_DEPTH;            // undo slots per lane: a cut is made at depths 0 .. max_depth - 1
constexpr u32 SPLIT_LANE_BITS = 6;                           // a heavy triangle's wave owns the 64 depth-6 subtrees
// more references than this: the triangle is filled by a wave, not by a lane.  At the threshold every lane of the wave has one reference on average; below it a
// wave would mostly idle (a wave per triangle costs 64 lanes 6 replayed cuts each), above it one lane would hold its 63 neighbours back (LEADS.md)
constexpr u32 SPLIT_HEAVY_MIN = 64;
static_assert(SPLIT_LEVELS == 16 && (1 << SPLIT_LANE_BITS) == WAVE, "dims word: 2 bits x 16 levels; one lane per depth-6 path");

struct SplitTris { const void* tris; const void* verts; const u32* idx; u32 n_verts; };

template <int FMT> __device__ __forceinline__ Box split_root(const SplitTris& in, u32 p) {   // stage E's box of triangle p, stage E's own expression
    if (FMT == BVH_TRI_PADDED64)      return stage_e_box_padded(static_cast<const float4*>(in.tris), p);
    else if (FMT == BVH_TRI_PACKED36) return stage_e_box9(static_cast<const float*>(in.tris) + (size_t)p * 9);
    else                              return stage_e_box_indexed(static_cast<const float*>(in.verts), in.idx, in.n_verts, p);
}

// (selects of registers, never an indexed array: nothing goes to scratch)
__device__ __forceinline__ float sel3(u32 d, float x, float y, float z) { return d == 0u ? x : d == 1u ? y : z; }
__device__ __forceinline__ float box_lo(const Box& b, u32 d) { return sel3(d, b.lx, b.ly, b.lz); }
__device__ __forceinline__ float box_hi(const Box& b, u32 d) { return sel3(d, b.hx, b.hy, b.hz); }
__device__ __forceinline__ void set_lo(Box& b, u32 d, float v) { b.lx = d == 0u ? v : b.lx; b.ly = d == 1u ? v : b.ly; b.lz = d == 2u ? v : b.lz; }
__device__ __forceinline__ void set_hi(Box& b, u32 d, float v) { b.hx = d == 0u ? v : b.hx; b.hy = d == 1u ? v : b.hy; b.hz = d == 2u ? v : b.hz; }

// the rule at one node: true = emit the box; false = cut axis `dim` at `c`.  Aabb::area (box_area), maximumExtentDim and center of src/Common.h:347-365
__device__ __forceinline__ bool split_emits(const Box& b, u32 depth, float sa_max, u32 max_depth, u32& dim, float& c) {
    const float ex = b.hx - b.lx, ey = b.hy - b.ly, ez = b.hz - b.lz;
    const float area = box_area(b);
    dim = (ex > ey && ex > ez) ? 0u : (ey > ez) ? 1u : 2u;
    const float lo = box_lo(b, dim), hi = box_hi(b, dim);
    c = (hi + lo) * 0.5f;
    return !(area > sa_max) || depth == max_depth || !(lo < c && c < hi);
}

// the subtree under (b, d0), depth-first, left first; returns its number of references.  FILL: reference k goes to out_boxes[k] / out_prims[k] while k < room.
// undo: the lane's LDS column (slot d at undo[d * SPLIT_BLOCK]); slots d0 .. max_depth - 1 are used
template <bool FILL>
__device__ __forceinline__ u32 split_walk(Box b, u32 d0, float sa_max, u32 max_depth, float* undo, bvh_aabb* out_boxes, u32* out_prims, u32 prim, u32 room) {
    u32 depth = d0, dims = 0u, path = 0u, k = 0u;
    for (;;) {
        u32 dim; float c;
        if (!split_emits(b, depth, sa_max, max_depth, dim, c)) {  // down into the left half (depth < max_depth <= 16 here)
            undo[depth * SPLIT_BLOCK] = box_hi(b, dim);
            set_hi(b, dim, c);
            dims = (dims & ~(3u << (2u * depth))) | (dim << (2u * depth));
            path &= ~(1u << depth);
            ++depth;
            continue;
        }
        if (FILL) { if (k < room) { box_store(out_boxes + k, b); out_prims[k] = prim; } }
        ++k;
        for (;;) {                                                // up, until a left child hands over to its right sibling
            if (depth == d0) return k;
            const u32 d = depth - 1u, dm = (dims >> (2u * d)) & 3u;
            float* const slot = undo + d * SPLIT_BLOCK;
            if (!((path >> d) & 1u)) {
                const float parent_hi = *slot;
                *slot = box_lo(b, dm);                            // the parent's min
                set_lo(b, dm, box_hi(b, dm));                     // the cut
                set_hi(b, dm, parent_hi);
                path |= 1u << d;
                break;
            }
            set_lo(b, dm, *slot);                                 // right child done: b is the parent's box again
            depth = d;
        }
    }
}

template <int FMT>
__global__ __launch_bounds__(SPLIT_BLOCK) void k_split_count(SplitTris in, u32 n, float sa_max, u32 max_depth, u32* __restrict__ offsets,
                                                             u32* __restrict__ heavy_list, u32* heavy_count) {
    __shared__ float s_undo[SPLIT_LEVELS * SPLIT_BLOCK];
    const u32 p = bid_x() * SPLIT_BLOCK + tid_x();
    u32 cnt = 0u;
    if (p < n) {
        cnt = split_walk<false>(split_root<FMT>(in, p), 0u, sa_max, max_depth, s_undo + tid_x(), nullptr, nullptr, p, 0u);
        offsets[p] = cnt;
    }
    const bool heavy = cnt > SPLIT_HEAVY_MIN;
    const u64 m = __ballot(heavy);
    if (m != 0ull) {                                              // (wave-uniform)
        const int leader = __builtin_ctzll(m);
        u32 base = 0u;
        if (lane_id() == leader) base = atomicAdd(heavy_count, (u32)__popcll(m));
        base = (u32)__shfl((int)base, leader);
        if (heavy) heavy_list[base + (u32)__popcll(m & lanemask_lt())] = p;      // (at most one entry per triangle: base + rank < n)
    }
}

template <int FMT>
__global__ __launch_bounds__(SPLIT_BLOCK) void k_split_fill(SplitTris in, u32 n, float sa_max, u32 max_depth, const u32* __restrict__ offsets,
                                                            bvh_aabb* __restrict__ boxes, u32* __restrict__ prims, const u64* __restrict__ total_word, u64 capacity) {
    __shared__ float s_undo[SPLIT_LEVELS * SPLIT_BLOCK];
    { const u64 t = *total_word; if (t > capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 p = bid_x() * SPLIT_BLOCK + tid_x();
    if (p >= n) return;
    const u32 base = offsets[p], end = offsets[p + 1];
    if (end <= base || end - base > SPLIT_HEAVY_MIN) return;      // (a heavy triangle: k_split_heavy's)
    split_walk<true>(split_root<FMT>(in, p), 0u, sa_max, max_depth, s_undo + tid_x(), boxes + base, prims + base, p, end - base);
}

template <int FMT>
__global__ __launch_bounds__(SPLIT_BLOCK) void k_split_heavy(SplitTris in, u32 n, float sa_max, u32 max_depth, const u32* __restrict__ offsets,
                                                             bvh_aabb* __restrict__ boxes, u32* __restrict__ prims, const u64* __restrict__ total_word, u64 capacity,
                                                             const u32* __restrict__ heavy_list, const u32* __restrict__ heavy_count) {
    __shared__ float s_undo[SPLIT_LEVELS * SPLIT_BLOCK];
    { const u64 t = *total_word; if (t > capacity || t > 0xFFFFFFFFull) return; }
    u32 nh = *heavy_count; if (nh > n) nh = n;
    const u32 lane = tid_x() & (u32)(WAVE - 1), waves = nbid_x() * (u32)(SPLIT_BLOCK / WAVE);
    for (u32 h = bid_x() * (u32)(SPLIT_BLOCK / WAVE) + tid_x() / (u32)WAVE; h < nh; h += waves) {      // (h is wave-uniform)
        const u32 p = heavy_list[h];
        if (p >= n) continue;
        const u32 base = offsets[p], end = offsets[p + 1];
        if (end <= base) continue;
        Box b = split_root<FMT>(in, p);
        u32 depth = 0u;
        bool own = true;
        while (depth < SPLIT_LANE_BITS) {                         // the lane's cuts from the root: level d is bit 5 - d of the lane index
            u32 dim; float c;
            if (split_emits(b, depth, sa_max, max_depth, dim, c)) { own = (lane & ((1u << (SPLIT_LANE_BITS - depth)) - 1u)) == 0u; break; }
            if ((lane >> (SPLIT_LANE_BITS - 1u - depth)) & 1u) set_lo(b, dim, c); else set_hi(b, dim, c);
            ++depth;
        }
        const u32 cnt = own ? split_walk<false>(b, depth, sa_max, max_depth, s_undo + tid_x(), nullptr, nullptr, p, 0u) : 0u;
        u32 incl = cnt;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) { const u32 up = (u32)__shfl_up((int)incl, o); if (lane >= (u32)o) incl += up; }
        const u32 at = incl - cnt, room = end - base;             // (a slice shorter than the counts say — the arrays changed in between — is not overrun)
        if (own && at < room) split_walk<true>(b, depth, sa_max, max_depth, s_undo + tid_x(), boxes + base + at, prims + base + at, p, room - at);
    }
}

// every leaf's primitive index q < n_map becomes map[q]; nothing else is written
template <int LAYOUT>
__global__ __launch_bounds__(SPLIT_BLOCK) void k_remap_leaves(bvh2_node* nodes, bvh_primref* leaves, u32 n, const u32* __restrict__ map, u32 n_map) {
    const u32 j = bid_x() * SPLIT_BLOCK + tid_x();
    if (j >= n) return;
    u32* const word = LAYOUT == 0 ? reinterpret_cast<u32*>(nodes + (n - 1 + j)) : &leaves[j].prim_idx;
    const u32 q = *word;
    if (q < n_map) *word = map[q];
}

namespace {
template <typename F> void by_format(int tri_format, F&& go) {
    switch (tri_format) {
        case BVH_TRI_PADDED64: go(std::integral_constant<int, BVH_TRI_PADDED64>{}); break;
        case BVH_TRI_PACKED36: go(std::integral_constant<int, BVH_TRI_PACKED36>{}); break;
        default:               go(std::integral_constant<int, BVH_TRI_INDEXED>{}); break;
    }
}
} // namespace

void launch_split_count(hipStream_t s, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices, uint32_t n,
                        float sa_max, uint32_t max_depth, uint32_t* d_offsets, uint32_t* d_heavy_list, uint32_t* d_heavy_count, uint64_t* d_sums,
                        uint64_t* d_total) {
    const SplitTris in{ d_tris, d_vertices, (const u32*)d_indices, n_vertices };
    const u32 blocks = (n + SPLIT_BLOCK - 1) / SPLIT_BLOCK;
    { KernelScope ks(s, "k_split_count");
      by_format(tri_format, [&](auto F) {
          hipLaunchKernelGGL((k_split_count<decltype(F)::value>), dim3(blocks), dim3(SPLIT_BLOCK), 0, s, in, n, sa_max, max_depth, d_offsets, d_heavy_list, d_heavy_count);
      }); }
    launch_overlap_scan(s, d_offsets, n, d_sums, d_total);
}

void launch_split_fill(hipStream_t s, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices, uint32_t n,
                       float sa_max, uint32_t max_depth, const uint32_t* d_offsets, void* d_ref_boxes, uint32_t* d_ref_prims, uint64_t capacity,
                       const uint64_t* d_total, const uint32_t* d_heavy_list, const uint32_t* d_heavy_count) {
    const SplitTris in{ d_tris, d_vertices, (const u32*)d_indices, n_vertices };
    const u32 blocks = (n + SPLIT_BLOCK - 1) / SPLIT_BLOCK;
    const u32 per_block = SPLIT_BLOCK / WAVE, want = (n + per_block - 1) / per_block, heavy_blocks = want < SPLIT_HEAVY_BLOCKS ? want : SPLIT_HEAVY_BLOCKS;
    by_format(tri_format, [&](auto F) {
        constexpr int FM = decltype(F)::value;
        { KernelScope ks(s, "k_split_fill");
          hipLaunchKernelGGL((k_split_fill<FM>), dim3(blocks), dim3(SPLIT_BLOCK), 0, s, in, n, sa_max, max_depth, d_offsets, (bvh_aabb*)d_ref_boxes, d_ref_prims,
                             d_total, (u64)capacity); }
        { KernelScope ks(s, "k_split_heavy");                     // (returns at once when the fill is skipped; an empty heavy list ends its loop at once)
          hipLaunchKernelGGL((k_split_heavy<FM>), dim3(heavy_blocks), dim3(SPLIT_BLOCK), 0, s, in, n, sa_max, max_depth, d_offsets, (bvh_aabb*)d_ref_boxes,
                             d_ref_prims, d_total, (u64)capacity, d_heavy_list, d_heavy_count); }
    });
}

void launch_remap_leaves(hipStream_t s, void* d_nodes, void* d_leaves, int layout, uint32_t n, const uint32_t* d_map, uint32_t n_map) {
    const u32 blocks = (n + SPLIT_BLOCK - 1) / SPLIT_BLOCK;
    KernelScope ks(s, "k_remap_leaves");
    if (layout == 0) hipLaunchKernelGGL(k_remap_leaves<0>, dim3(blocks), dim3(SPLIT_BLOCK), 0, s, (bvh2_node*)d_nodes, (bvh_primref*)d_leaves, n, d_map, n_map);
    else             hipLaunchKernelGGL(k_remap_leaves<1>, dim3(blocks), dim3(SPLIT_BLOCK), 0, s, (bvh2_node*)d_nodes, (bvh_primref*)d_leaves, n, d_map, n_map);
}

void warm_split() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_split_count<BVH_TRI_PADDED64>)); }

} // namespace bvh
