// overlap.hip — bvh_overlap on gfx950: which primitives' leaf boxes does each query box touch, against a built BVH2 in either node layout (no counterpart in the
// reference).  The answer has a variable length, so the call is count -> scan -> fill; count and fill are the SAME walk, templated on node layout, pass and mode.
//   k_overlap_walk  : one query per lane, short per-lane stack in LDS (QUERY_STACK entries, query.hip's layout).  Per internal node both children's records are
//                     fetched and tested; a leaf child that overlaps is counted / stored at once; of two overlapping internal children the left one is entered
//                     and the right one pushed (every overlapping subtree must be visited: there is no order to prefer).  A query whose push would overflow (or
//                     whose walk exceeds the node count: arrays that are not a tree) is marked and bumps the pass's overflow word.  Count pass: the mark is the
//                     count word (QUERY_MARK is never a count: n < 2^30).  Fill pass: a query with an empty slice is not walked at all, so a marked query has a
//                     slot and the mark is its slice's first word (QUERY_MARK is never a primitive).
//   k_overlap_deep  : launched after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked query from its start, stackless
//                     through the parent links of bvh_refit's plan (k_refit_plan), left child first.  Correct at any depth.  Both walks report exactly the leaves
//                     whose own box and every box above them (the root's excepted: neither walk tests it) overlap the query, so count and fill agree whichever
//                     walk served a query.
//   k_overlap_reduce / k_overlap_scan : the exclusive scan of the n_boxes counts into u32[n_boxes + 1] offsets, in place, by a fixed grid of SCAN_BLOCKS workgroups
//                     over contiguous chunks: chunk sums (u64) first, then every workgroup adds up the sums before its chunk and scans it.  Sums are 64-bit; offsets
//                     saturate at 0xFFFFFFFF; the last workgroup stores the 64-bit total.
// The fill pass decides ON THE DEVICE whether it runs: total <= capacity and total < 2^32, read from the total word.
// Box tests are comparisons only (box_overlap, query.hpp): no margin, the answer is exact for every query.  Built WITH the SLP vectoriser (unlike
// scene.o / point_query.o): there is no f32 arithmetic to pack and no tie-breaking record update for it to reorder.
#include <type_traits>
#include "query.hpp"
#include "kernels.hpp"

namespace bvh {

constexpr int SCAN_BLOCK = 256;                // threads per scan workgroup
constexpr int SCAN_IPT = 4;                    // consecutive words per thread
constexpr u32 SCAN_TILE = SCAN_BLOCK * SCAN_IPT;
static_assert(OVERLAP_SCAN_BLOCKS <= 1024, "k_overlap_scan adds up the chunk sums with one pass of its 256 threads over at most 1024 words");

// where a walk's results go.  Count pass: a counter.  Fill pass: the query's slice [base, base + room) of d_prims, never written past its end (a walk of arrays
// that are not a tree may find more than the count pass did only if the arrays changed in between; the bound keeps that in the slice)
template <bool FILL> struct Sink {
    u32* out; u32 room, k = 0;
    __device__ __forceinline__ void put(u32 prim) { if (FILL) { if (k < room) out[k] = prim; } ++k; }
};

// a leaf child's primitive: in range (never followed otherwise) and, in self mode, above the query's own index (every unordered pair once)
template <bool SELF> __device__ __forceinline__ bool prim_ok(u32 prim, u32 n, u32 i) { return prim < n && (!SELF || prim > i); }

template <int LAYOUT, bool FILL, bool SELF>
__global__ __launch_bounds__(QUERY_BLOCK) void k_overlap_walk(const bvh_aabb* __restrict__ boxes, u32 n_boxes, const bvh2_node* __restrict__ nodes,
                                                              const bvh_primref* __restrict__ leaves, u32 n, u32 root, u32* __restrict__ offsets,
                                                              u32* __restrict__ prims, const u64* __restrict__ total_word, u64 capacity, u32* __restrict__ overflow) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 t = *total_word; if (t > capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= n_boxes) return;
    Sink<FILL> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = offsets[i], end = offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = prims + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    const Box q = box_load_u(boxes + i);
    bool deep = false;
    if (box_valid(q)) {                                           // (NaN or inverted: overlaps nothing)
        const u32 ni = n - 1, total = 2 * n - 1;
        u32 nl, nr; { const uint2 lr = *reinterpret_cast<const uint2*>(nodes + root); nl = lr.x; nr = lr.y; }
        u32 top = 0, steps = 0;
        for (;;) {
            if (++steps > n) { deep = true; break; }              // more expansions than internal nodes: not a tree (a tree never gets here)
            u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
            Box ba, bb;
            bool ha = false, hb = false;
            if (nl < total) { rec_fetch<LAYOUT>(nodes, leaves, nl, ni, a0, a1, ba); ha = box_overlap(q, ba); }
            if (nr < total) { rec_fetch<LAYOUT>(nodes, leaves, nr, ni, b0, b1, bb); hb = box_overlap(q, bb); }
            if (ha && nl >= ni) { if (prim_ok<SELF>(a0, n, i)) sink.put(a0); ha = false; }
            if (hb && nr >= ni) { if (prim_ok<SELF>(b0, n, i)) sink.put(b0); hb = false; }
            if (ha || hb) {
                if (ha && hb) {
                    if (top == (u32)QUERY_STACK) { deep = true; break; }
                    stack[top * QUERY_BLOCK] = nr; ++top;
                }
                nl = ha ? a0 : b0; nr = ha ? a1 : b1;             // (selects of values: as separate branches the links went through scratch slots)
            } else {
                if (top == 0) break;
                const u32 node = stack[--top * QUERY_BLOCK];
                const uint2 lr = *reinterpret_cast<const uint2*>(nodes + node);
                nl = lr.x; nr = lr.y;
            }
        }
    }
    if (deep) atomicAdd(overflow, 1u);
    if (FILL) { if (deep) sink.out[0] = QUERY_MARK; }
    else offsets[i] = deep ? QUERY_MARK : sink.k;
}

// the stackless re-walk of the marked queries: parent links of the plan, left child first
template <int LAYOUT, bool FILL, bool SELF>
__global__ __launch_bounds__(QUERY_BLOCK) void k_overlap_deep(const bvh_aabb* __restrict__ boxes, u32 n_boxes, const bvh2_node* __restrict__ nodes,
                                                              const bvh_primref* __restrict__ leaves, u32 n, u32 root, u32* __restrict__ offsets,
                                                              u32* __restrict__ prims, const u32* __restrict__ overflow, const u32* __restrict__ parent) {
    if (*overflow == 0u) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < n_boxes; i += nbid_x() * QUERY_BLOCK) {
        Sink<FILL> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = offsets[i], end = offsets[i + 1];
            if (end <= base || prims[base] != QUERY_MARK) continue;
            sink.out = prims + base; sink.room = end - base;
        } else if (offsets[i] != QUERY_MARK) continue;
        const Box q = box_load_u(boxes + i);                      // (a marked query passed box_valid)
        u32 cur = root, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < total && steps < bound; ++steps) {
            if (down) {
                u32 w0, w1; Box b;
                rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                if (cur >= ni) {
                    if (box_overlap(q, b) && prim_ok<SELF>(w0, n, i)) sink.put(w0);
                    last = cur; cur = parent[cur]; down = false;
                    continue;
                }
                if (cur != root && !box_overlap(q, b)) { last = cur; cur = parent[cur]; down = false; continue; }   // (the root's own box: as k_overlap_walk, not tested)
                if (w0 < total) { cur = w0; continue; }
                last = w0; down = false;                          // (a left link out of range: as if its subtree were done)
                continue;
            }
            if (cur >= ni) break;                                 // (parent links are internal nodes or INVALID)
            const uint2 lr = *reinterpret_cast<const uint2*>(nodes + cur);
            if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
            last = cur; cur = parent[cur];
        }
        if (!FILL) offsets[i] = sink.k;
    }
}

// ---- counts -> offsets.  words = n_boxes + 1 (the word behind the last count is read as 0: nothing has written it yet); workgroup b owns the words
// [b * chunk, (b + 1) * chunk), chunk a multiple of SCAN_TILE
__device__ __forceinline__ u64 block_sum(u64 v, u64* s_red) {
    for (int o = 32; o > 0; o >>= 1) { v += (u64)__shfl_down((u32)v, o) | ((u64)__shfl_down((u32)(v >> 32), o) << 32); }
    if ((tid_x() & 63u) == 0u) s_red[tid_x() >> 6] = v;
    __syncthreads();
    const u64 r = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_overlap_reduce(const u32* __restrict__ offsets, u32 n_boxes, u32 chunk, u64* __restrict__ sums) {
    __shared__ u64 s_red[SCAN_BLOCK / 64];
    const u64 lo = (u64)bid_x() * chunk, hi = lo + chunk < (u64)n_boxes ? lo + chunk : (u64)n_boxes;
    u64 acc = 0;
    for (u64 k = lo + tid_x(); k < hi; k += SCAN_BLOCK) acc += offsets[k];
    const u64 r = block_sum(acc, s_red);
    if (tid_x() == 0) sums[bid_x()] = r;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_overlap_scan(u32* __restrict__ offsets, u32 n_boxes, u32 chunk, const u64* __restrict__ sums,
                                                             u64* __restrict__ total_word) {
    __shared__ u64 s_red[SCAN_BLOCK / 64];
    __shared__ u64 s_scan[SCAN_BLOCK];
    const u32 b = bid_x(), t = tid_x();
    u64 before = 0;
    for (u32 k = t; k < b; k += SCAN_BLOCK) before += sums[k];
    u64 carry = block_sum(before, s_red);                          // everything in front of this chunk
    if (b + 1 == nbid_x() && t == 0) *total_word = carry + sums[b];
    const u64 words = (u64)n_boxes + 1ull;
    const u64 lo = (u64)b * chunk, hi = lo + chunk < words ? lo + chunk : words;
    for (u64 tile = lo; tile < hi; tile += SCAN_TILE) {
        const u64 at = tile + (u64)t * SCAN_IPT;
        u32 v[SCAN_IPT];
        u64 mine = 0;
        for (int k = 0; k < SCAN_IPT; ++k) { v[k] = at + k < (u64)n_boxes ? offsets[at + k] : 0u; mine += v[k]; }
        s_scan[t] = mine;
        __syncthreads();
        for (u32 o = 1; o < (u32)SCAN_BLOCK; o <<= 1) {           // (inclusive, Hillis-Steele: eight rounds of 256 words — this is not the hot path)
            const u64 add = t >= o ? s_scan[t - o] : 0ull;
            __syncthreads();
            s_scan[t] += add;
            __syncthreads();
        }
        u64 run = carry + (s_scan[t] - mine);
        const u64 tile_sum = s_scan[SCAN_BLOCK - 1];
        for (int k = 0; k < SCAN_IPT; ++k) {
            if (at + k < hi) offsets[at + k] = run > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)run;
            run += v[k];
        }
        carry += tile_sum;
        __syncthreads();
    }
}

void launch_overlap_count(hipStream_t s, int layout, int mode, const void* d_boxes, uint32_t n_boxes, const void* d_nodes, const void* d_leaves, uint32_t n,
                          uint32_t root, uint32_t* d_offsets, uint32_t* d_overflow, const uint32_t* d_parent, uint64_t* d_sums, uint64_t* d_total) {
    const u32 blocks = (n_boxes + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    const bvh_aabb* boxes = (const bvh_aabb*)d_boxes; const bvh2_node* nodes = (const bvh2_node*)d_nodes; const bvh_primref* leaves = (const bvh_primref*)d_leaves;
    auto go = [&](auto L, auto S) {
        constexpr int LA = decltype(L)::value; constexpr bool SE = decltype(S)::value;
        { KernelScope ks(s, "k_overlap_count");
          hipLaunchKernelGGL((k_overlap_walk<LA, false, SE>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, boxes, n_boxes, nodes, leaves, n, root, d_offsets,
                             (u32*)nullptr, (const u64*)nullptr, (u64)0, d_overflow); }
        { KernelScope ks(s, "k_overlap_deep");
          hipLaunchKernelGGL((k_overlap_deep<LA, false, SE>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, boxes, n_boxes, nodes, leaves, n, root, d_offsets,
                             (u32*)nullptr, (const u32*)d_overflow, d_parent); }
    };
    using L0 = std::integral_constant<int, 0>; using L1 = std::integral_constant<int, 1>;
    auto by_mode = [&](auto L) { if (mode == BVH_OVERLAP_SELF) go(L, std::true_type{}); else go(L, std::false_type{}); };
    if (layout == 0) by_mode(L0{}); else by_mode(L1{});
    launch_overlap_scan(s, d_offsets, n_boxes, d_sums, d_total);
}

// the scan: at most OVERLAP_SCAN_BLOCKS chunks of whole tiles over the n_boxes + 1 words (bvh_intersect_all's counts go through it too: multihit.hip)
void launch_overlap_scan(hipStream_t s, uint32_t* d_offsets, uint32_t n_boxes, uint64_t* d_sums, uint64_t* d_total) {
    const u64 words = (u64)n_boxes + 1ull, tiles = (words + SCAN_TILE - 1) / SCAN_TILE;
    const u64 tiles_per = (tiles + OVERLAP_SCAN_BLOCKS - 1) / OVERLAP_SCAN_BLOCKS;
    const u32 chunk = (u32)(tiles_per * SCAN_TILE), scan_blocks = (u32)((tiles + tiles_per - 1) / tiles_per);
    KernelScope ks(s, "k_overlap_scan");
    hipLaunchKernelGGL(k_overlap_reduce, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, s, (const u32*)d_offsets, n_boxes, chunk, d_sums);
    hipLaunchKernelGGL(k_overlap_scan, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, s, d_offsets, n_boxes, chunk, (const u64*)d_sums, d_total);
}

void launch_overlap_fill(hipStream_t s, int layout, int mode, const void* d_boxes, uint32_t n_boxes, const void* d_nodes, const void* d_leaves, uint32_t n,
                         uint32_t root, uint32_t* d_offsets, uint32_t* d_prims, uint64_t capacity, const uint64_t* d_total, uint32_t* d_overflow,
                         const uint32_t* d_parent) {
    const u32 blocks = (n_boxes + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    const bvh_aabb* boxes = (const bvh_aabb*)d_boxes; const bvh2_node* nodes = (const bvh2_node*)d_nodes; const bvh_primref* leaves = (const bvh_primref*)d_leaves;
    auto go = [&](auto L, auto S) {
        constexpr int LA = decltype(L)::value; constexpr bool SE = decltype(S)::value;
        { KernelScope ks(s, "k_overlap_fill");
          hipLaunchKernelGGL((k_overlap_walk<LA, true, SE>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, boxes, n_boxes, nodes, leaves, n, root, d_offsets, d_prims,
                             d_total, (u64)capacity, d_overflow); }
        { KernelScope ks(s, "k_overlap_deep");                    // (its overflow word stays 0 when the fill returned at once)
          hipLaunchKernelGGL((k_overlap_deep<LA, true, SE>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, boxes, n_boxes, nodes, leaves, n, root, d_offsets, d_prims,
                             (const u32*)d_overflow, d_parent); }
    };
    using L0 = std::integral_constant<int, 0>; using L1 = std::integral_constant<int, 1>;
    auto by_mode = [&](auto L) { if (mode == BVH_OVERLAP_SELF) go(L, std::true_type{}); else go(L, std::false_type{}); };
    if (layout == 0) by_mode(L0{}); else by_mode(L1{});
}

void warm_overlap() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_overlap_walk<0, false, false>));
}

} // namespace bvh
