// multihit.hip — bvh_intersect_all on gfx950: EVERY accepted hit along each ray, against a built BVH2 in either node layout (no counterpart in the reference).
// The answer has a variable length, so the call is count -> scan -> fill as in overlap.hip; count and fill are the SAME walk, templated on node layout, triangle
// format, pass and order.  The hit test and the box test are bvh_intersect's (tri_hit, box_pass: query.hpp); what differs from k_intersect is that the bound
// never shrinks — box_pass runs against tmax for the whole walk — so every passing subtree is visited and the answer is a set of records.
//   k_hits_walk : one ray per lane, short per-lane stack in LDS (QUERY_STACK entries, query.hip's layout).  Per internal node both children's records are fetched
//                 and box-tested; a passing leaf child is hit-tested at once and an accepted hit counted / stored; of two passing internal children the left one is
//                 entered and the right one pushed (every passing subtree must be visited: near-first ordering buys nothing).  A ray whose push would overflow (or
//                 whose walk exceeds the node count: arrays that are not a tree) is marked and bumps the pass's overflow word.  Count pass: the mark is the count
//                 word (QUERY_MARK is never a count: n < 2^30).  Fill pass: a ray with an empty slice is not walked at all, so a marked ray has a record and the
//                 mark is the prim_idx of its slice's first record (QUERY_MARK is never a primitive).
//   k_hits_deep : launched after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked ray from its start, stackless
//                 through the parent links of bvh_refit's plan (k_refit_plan), left child first.  Correct at any depth.  Both walks report exactly the accepted
//                 hits of the leaves whose own box and every box above them (the root's excepted: neither walk tests it) pass, so count and fill agree whichever
//                 walk served a ray.
// Fill: a lane writes whole 16-byte records into its own slice [d_offsets[i], d_offsets[i+1]) and never past it; no atomics.  SORTED: the lane keeps the slice in
// ascending (t, prim) order as it goes, inserting each hit by comparing and shifting whole records from the slice's tail (its own earlier stores, read back by the
// same lane).  An accepted t is finite and not NaN (tmin < t < tmax held), so plain float comparisons order it.
// The scan of the counts and the total word are bvh_overlap's (launch_overlap_scan, overlap.hip).  The fill decides ON THE DEVICE whether it runs.
// Compiled WITHOUT the SLP vectoriser (Makefile), like scene.hip / point_query.hip / knn.hip: the sorted insertion compares and replaces (t, u, v, prim) records.
#include <type_traits>
#include "query.hpp"
#include "kernels.hpp"

namespace bvh {

// where a walk's hits go.  Count pass: a counter.  Fill pass: the ray's slice [out, out + room) of d_hits, never written past its end (a walk of arrays that
// are not a tree may find more than the count pass did only if the arrays changed in between; the bound keeps that in the slice)
template <bool FILL, bool SORTED> struct HitSink {
    float4* out; u32 room, k = 0;
    __device__ __forceinline__ void put(float it, float iu, float iv, u32 prim) {
        if (FILL) {
            if (k < room) {
                u32 j = k;
                if (SORTED) {
                    while (j > 0) {                               // (records above (it, prim) move up by one; the slice below j + 1 stays sorted)
                        const float4 p = out[j - 1];
                        if (!(p.x > it || (p.x == it && __float_as_uint(p.w) > prim))) break;
                        out[j] = p; --j;
                    }
                }
                out[j] = make_float4(it, iu, iv, __uint_as_float(prim));
            }
        }
        ++k;
    }
};

// the candidate prim's test: in range (never followed otherwise) and an accepted hit
template <int FMT, bool FILL, bool SORTED>
__device__ __forceinline__ void hit_leaf(const TriSrc& src, u32 prim, u32 n, const QRay& r, HitSink<FILL, SORTED>& sink) {
    if (prim >= n) return;
    QF3 a, b, c; tri_fetch<FMT>(src, prim, a, b, c);
    float it, iu, iv;
    if (tri_hit(a, b, c, r, it, iu, iv) && r.tmin < it && it < r.tmax) sink.put(it, iu, iv, prim);
}

template <int LAYOUT, int FMT, bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_hits_walk(const bvh_ray* __restrict__ rays, u32 n_rays, const bvh2_node* __restrict__ nodes,
                                                           const bvh_primref* __restrict__ leaves, TriSrc src, u32 n, u32 root, u32* __restrict__ offsets,
                                                           float4* hits, const u64* __restrict__ total_word, u64 capacity, u32* __restrict__ overflow) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 t = *total_word; if (t > capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= n_rays) return;
    HitSink<FILL, SORTED> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = offsets[i], end = offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = hits + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    QRay r;
    const bool live = ray_load(rays, i, r);
    bool deep = false;
    if (live) {                                                   // (a NaN component or !(tmin < tmax): accepts nothing)
        const u32 ni = n - 1, total = 2 * n - 1;
        u32 nl, nr; { const uint2 lr = *reinterpret_cast<const uint2*>(nodes + root); nl = lr.x; nr = lr.y; }
        u32 top = 0, steps = 0;
        for (;;) {
            if (++steps > n) { deep = true; break; }              // more expansions than internal nodes: not a tree (a tree never gets here)
            u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
            Box ba, bb;
            float ta, tb;
            bool ha = false, hb = false;
            if (nl < total) { rec_fetch<LAYOUT>(nodes, leaves, nl, ni, a0, a1, ba); ha = box_pass(ba, r, r.tmax, ta); }
            if (nr < total) { rec_fetch<LAYOUT>(nodes, leaves, nr, ni, b0, b1, bb); hb = box_pass(bb, r, r.tmax, tb); }
            if (ha && nl >= ni) { hit_leaf<FMT>(src, a0, n, r, sink); ha = false; }
            if (hb && nr >= ni) { hit_leaf<FMT>(src, b0, n, r, sink); hb = false; }
            if (ha || hb) {
                if (ha && hb) {
                    if (top == (u32)QUERY_STACK) { deep = true; break; }
                    stack[top * QUERY_BLOCK] = nr; ++top;
                }
                nl = ha ? a0 : b0; nr = ha ? a1 : b1;             // (selects of values, not branches to them: overlap.hip)
            } else {
                if (top == 0) break;
                const u32 node = stack[--top * QUERY_BLOCK];
                const uint2 lr = *reinterpret_cast<const uint2*>(nodes + node);
                nl = lr.x; nr = lr.y;
            }
        }
    }
    if (deep) atomicAdd(overflow, 1u);
    if (FILL) { if (deep) reinterpret_cast<u32*>(sink.out)[3] = QUERY_MARK; }
    else offsets[i] = deep ? QUERY_MARK : sink.k;
}

// the stackless re-walk of the marked rays: parent links of the plan, left child first
template <int LAYOUT, int FMT, bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_hits_deep(const bvh_ray* __restrict__ rays, u32 n_rays, const bvh2_node* __restrict__ nodes,
                                                           const bvh_primref* __restrict__ leaves, TriSrc src, u32 n, u32 root, u32* __restrict__ offsets,
                                                           float4* hits, const u32* __restrict__ overflow, const u32* __restrict__ parent) {
    if (*overflow == 0u) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < n_rays; i += nbid_x() * QUERY_BLOCK) {
        HitSink<FILL, SORTED> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = offsets[i], end = offsets[i + 1];
            if (end <= base || __float_as_uint(hits[base].w) != QUERY_MARK) continue;
            sink.out = hits + base; sink.room = end - base;
        } else if (offsets[i] != QUERY_MARK) continue;
        QRay r;
        ray_load(rays, i, r);                                     // (a marked ray passed the checks)
        u32 cur = root, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < total && steps < bound; ++steps) {
            if (down) {
                u32 w0, w1; Box b; float tn;
                rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                if (cur >= ni) {
                    if (box_pass(b, r, r.tmax, tn)) hit_leaf<FMT>(src, w0, n, r, sink);
                    last = cur; cur = parent[cur]; down = false;
                    continue;
                }
                if (cur != root && !box_pass(b, r, r.tmax, tn)) { last = cur; cur = parent[cur]; down = false; continue; }   // (the root's own box: as k_hits_walk, not tested)
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

namespace {
struct HitsArgs {
    hipStream_t s; const bvh_ray* rays; u32 n_rays; const bvh2_node* nodes; const bvh_primref* leaves; TriSrc src; u32 n, root; u32* offsets; float4* hits;
    const u64* total; u64 capacity; u32* overflow; const u32* parent;
};

template <bool FILL, bool SORTED> void hits_pass(const HitsArgs& a, int layout, int tri_format) {
    const u32 blocks = (a.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    auto go = [&](auto L, auto F) {
        constexpr int LA = decltype(L)::value, FM = decltype(F)::value;
        { KernelScope ks(a.s, FILL ? "k_hits_fill" : "k_hits_count");
          hipLaunchKernelGGL((k_hits_walk<LA, FM, FILL, SORTED>), dim3(blocks), dim3(QUERY_BLOCK), 0, a.s, a.rays, a.n_rays, a.nodes, a.leaves, a.src, a.n, a.root,
                             a.offsets, a.hits, a.total, a.capacity, a.overflow); }
        { KernelScope ks(a.s, "k_hits_deep");                     // (the fill's overflow word stays 0 when the fill returned at once)
          hipLaunchKernelGGL((k_hits_deep<LA, FM, FILL, SORTED>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, a.s, a.rays, a.n_rays, a.nodes, a.leaves, a.src, a.n,
                             a.root, a.offsets, a.hits, (const u32*)a.overflow, a.parent); }
    };
    auto by_fmt = [&](auto L) {
        switch (tri_format) {
            case BVH_TRI_PADDED64: go(L, std::integral_constant<int, BVH_TRI_PADDED64>{}); break;
            case BVH_TRI_PACKED36: go(L, std::integral_constant<int, BVH_TRI_PACKED36>{}); break;
            default:               go(L, std::integral_constant<int, BVH_TRI_INDEXED>{}); break;
        }
    };
    if (layout == 0) by_fmt(std::integral_constant<int, 0>{}); else by_fmt(std::integral_constant<int, 1>{});
}
} // namespace

void launch_hits_count(hipStream_t s, int layout, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                       const void* d_rays, uint32_t n_rays, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets,
                       uint32_t* d_overflow, const uint32_t* d_parent, uint64_t* d_sums, uint64_t* d_total) {
    const HitsArgs a{ s, (const bvh_ray*)d_rays, n_rays, (const bvh2_node*)d_nodes, (const bvh_primref*)d_leaves,
                      TriSrc{ d_tris, (const float*)d_vertices, (const u32*)d_indices, n_vertices }, n, root, d_offsets, nullptr, nullptr, 0, d_overflow, d_parent };
    hits_pass<false, false>(a, layout, tri_format);
    launch_overlap_scan(s, d_offsets, n_rays, d_sums, d_total);
}

void launch_hits_fill(hipStream_t s, int layout, int tri_format, int sorted, const void* d_tris, const void* d_vertices, const void* d_indices,
                      uint32_t n_vertices, const void* d_rays, uint32_t n_rays, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root,
                      uint32_t* d_offsets, void* d_hits, uint64_t capacity, const uint64_t* d_total, uint32_t* d_overflow, const uint32_t* d_parent) {
    const HitsArgs a{ s, (const bvh_ray*)d_rays, n_rays, (const bvh2_node*)d_nodes, (const bvh_primref*)d_leaves,
                      TriSrc{ d_tris, (const float*)d_vertices, (const u32*)d_indices, n_vertices }, n, root, d_offsets, (float4*)d_hits, d_total, capacity,
                      d_overflow, d_parent };
    if (sorted) hits_pass<true, true>(a, layout, tri_format); else hits_pass<true, false>(a, layout, tri_format);
}

void warm_multihit() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_hits_walk<0, BVH_TRI_PADDED64, false, false>));
}

} // namespace bvh
