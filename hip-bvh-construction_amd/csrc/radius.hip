// radius.hip — bvh_radius_search on gfx950: EVERY triangle within the radius of each query point, against a built BVH2 in either node layout (no counterpart in
// the reference).  The answer has a variable length, so the call is count -> scan -> fill as in multihit.hip; count and fill are the SAME walk, templated on node
// layout, triangle format, pass and order.  The candidate and the box test are bvh_closest_point's (tri_closest, box_dist_pass: query.hpp); what differs from
// k_closest_point / k_knn is that the bound never shrinks — box_dist_pass runs against r2 for the whole walk — so every passing subtree is visited and the answer
// is a set of {dist2, prim} records.
//   k_radius_walk : one query per lane, short per-lane stack in LDS (QUERY_STACK entries, query.hip's layout).  Per internal node both children's records are
//                   fetched and box-tested; a passing leaf child's candidate is computed at once and an accepted one counted / stored; of two passing internal
//                   children the left one is entered and the right one pushed (every passing subtree must be visited: near-first ordering buys nothing).  A query
//                   whose push would overflow (or whose walk exceeds the node count: arrays that are not a tree) is marked and bumps the pass's overflow word.
//                   Count pass: the mark is the count word (QUERY_MARK is never a count: n < 2^30).  Fill pass: a query with an empty slice is not walked at all,
//                   so a marked query has a record and the mark is the prim_idx of its slice's first record (QUERY_MARK is never a primitive).
//   k_radius_deep : launched after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked query from its start, stackless
//                   through the parent links of bvh_refit's plan (k_refit_plan), left child first.  Correct at any depth.  Both walks report exactly the accepted
//                   candidates of the leaves whose own box and every box above them (the root's excepted: neither walk tests it) pass, so count and fill agree
//                   whichever walk served a query.
// Fill: a lane writes whole 8-byte records into its own slice [d_offsets[i], d_offsets[i+1]) and never past it; no atomics.  SORTED: the lane keeps the slice in
// ascending (dist2, prim) order as it goes, inserting each record by comparing and shifting whole records from the slice's tail (its own earlier stores, read
// back by the same lane) on knn.hip's u64 key (float_as_uint(dist2) << 32) | prim: an accepted dist2 is a sum of squares, never negative and never NaN, so the
// u64 order is the contract's lexicographic order.  The insertion is quadratic in the slice's length.
// The scan of the counts and the total word are bvh_overlap's (launch_overlap_scan, overlap.hip).  The fill decides ON THE DEVICE whether it runs.
// Compiled WITHOUT the SLP vectoriser (Makefile), like point_query.hip / knn.hip / multihit.hip: the sorted insertion compares and replaces (dist2, prim) records.
#include <type_traits>
#include "query.hpp"
#include "kernels.hpp"

namespace bvh {

// where a walk's records go.  Count pass: a counter.  Fill pass: the query's slice [out, out + room) of d_hits as {dist2 bits, prim} words, never written past
// its end (a walk of arrays that are not a tree may find more than the count pass did only if the arrays changed in between; the bound keeps that in the slice)
template <bool FILL, bool SORTED> struct RadiusSink {
    uint2* out; u32 room, k = 0;
    __device__ __forceinline__ void put(float d2, u32 prim) {
        if (FILL) {
            if (k < room) {
                u32 j = k;
                const u32 db = __float_as_uint(d2);
                if (SORTED) {
                    const u64 key = ((u64)db << 32) | prim;
                    while (j > 0) {                               // (records above the key move up by one; the slice below j + 1 stays sorted)
                        const uint2 p = out[j - 1];
                        if (!((((u64)p.x << 32) | p.y) > key)) break;
                        out[j] = p; --j;
                    }
                }
                out[j] = make_uint2(db, prim);
            }
        }
        ++k;
    }
};

// the candidate of prim: in range (never followed otherwise) and accepted iff dist2 <= r2 (a NaN dist2 fails)
template <int FMT, bool FILL, bool SORTED>
__device__ __forceinline__ void radius_leaf(const TriSrc& src, u32 prim, u32 n, QF3 p, float r2, RadiusSink<FILL, SORTED>& sink) {
    if (prim >= n) return;
    QF3 a, b, c; tri_fetch<FMT>(src, prim, a, b, c);
    QF3 q; float u, v;
    const float d2 = tri_closest(a, b, c, p, q, u, v);
    if (d2 <= r2) sink.put(d2, prim);
}

template <int LAYOUT, int FMT, bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_radius_walk(const bvh_point_query* __restrict__ pts, u32 n_points, const bvh2_node* __restrict__ nodes,
                                                             const bvh_primref* __restrict__ leaves, TriSrc src, u32 n, u32 root, u32* __restrict__ offsets,
                                                             uint2* hits, const u64* __restrict__ total_word, u64 capacity, u32* __restrict__ overflow) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 t = *total_word; if (t > capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= n_points) return;
    RadiusSink<FILL, SORTED> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = offsets[i], end = offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = hits + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    QF3 p; float r2;
    const bool live = point_load(pts, i, p, r2);
    bool deep = false;
    if (live) {                                                   // (a NaN coordinate, a NaN or negative radius: accepts nothing)
        const u32 ni = n - 1, total = 2 * n - 1;
        u32 nl, nr; { const uint2 lr = *reinterpret_cast<const uint2*>(nodes + root); nl = lr.x; nr = lr.y; }
        u32 top = 0, steps = 0;
        for (;;) {
            if (++steps > n) { deep = true; break; }              // more expansions than internal nodes: not a tree (a tree never gets here)
            u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
            Box ba, bb;
            float la, lb;
            bool ha = false, hb = false;
            if (nl < total) { rec_fetch<LAYOUT>(nodes, leaves, nl, ni, a0, a1, ba); ha = box_dist_pass(ba, p, r2, la); }
            if (nr < total) { rec_fetch<LAYOUT>(nodes, leaves, nr, ni, b0, b1, bb); hb = box_dist_pass(bb, p, r2, lb); }
            if (ha && nl >= ni) { radius_leaf<FMT>(src, a0, n, p, r2, sink); ha = false; }
            if (hb && nr >= ni) { radius_leaf<FMT>(src, b0, n, p, r2, sink); hb = false; }
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
    if (FILL) { if (deep) sink.out[0].y = QUERY_MARK; }
    else offsets[i] = deep ? QUERY_MARK : sink.k;
}

// the stackless re-walk of the marked queries: parent links of the plan, left child first
template <int LAYOUT, int FMT, bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_radius_deep(const bvh_point_query* __restrict__ pts, u32 n_points, const bvh2_node* __restrict__ nodes,
                                                             const bvh_primref* __restrict__ leaves, TriSrc src, u32 n, u32 root, u32* __restrict__ offsets,
                                                             uint2* hits, const u32* __restrict__ overflow, const u32* __restrict__ parent) {
    if (*overflow == 0u) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < n_points; i += nbid_x() * QUERY_BLOCK) {
        RadiusSink<FILL, SORTED> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = offsets[i], end = offsets[i + 1];
            if (end <= base || hits[base].y != QUERY_MARK) continue;
            sink.out = hits + base; sink.room = end - base;
        } else if (offsets[i] != QUERY_MARK) continue;
        QF3 p; float r2;
        point_load(pts, i, p, r2);                                // (a marked query passed the checks)
        u32 cur = root, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < total && steps < bound; ++steps) {
            if (down) {
                u32 w0, w1; Box b; float lb;
                rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                if (cur >= ni) {
                    if (box_dist_pass(b, p, r2, lb)) radius_leaf<FMT>(src, w0, n, p, r2, sink);
                    last = cur; cur = parent[cur]; down = false;
                    continue;
                }
                if (cur != root && !box_dist_pass(b, p, r2, lb)) { last = cur; cur = parent[cur]; down = false; continue; }   // (the root's own box: as k_radius_walk, not tested)
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
struct RadiusArgs {
    hipStream_t s; const bvh_point_query* pts; u32 n_points; const bvh2_node* nodes; const bvh_primref* leaves; TriSrc src; u32 n, root; u32* offsets; uint2* hits;
    const u64* total; u64 capacity; u32* overflow; const u32* parent;
};

template <bool FILL, bool SORTED> void radius_pass(const RadiusArgs& a, int layout, int tri_format) {
    const u32 blocks = (a.n_points + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    auto go = [&](auto L, auto F) {
        constexpr int LA = decltype(L)::value, FM = decltype(F)::value;
        { KernelScope ks(a.s, FILL ? "k_radius_fill" : "k_radius_count");
          hipLaunchKernelGGL((k_radius_walk<LA, FM, FILL, SORTED>), dim3(blocks), dim3(QUERY_BLOCK), 0, a.s, a.pts, a.n_points, a.nodes, a.leaves, a.src, a.n, a.root,
                             a.offsets, a.hits, a.total, a.capacity, a.overflow); }
        { KernelScope ks(a.s, "k_radius_deep");                   // (the fill's overflow word stays 0 when the fill returned at once)
          hipLaunchKernelGGL((k_radius_deep<LA, FM, FILL, SORTED>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, a.s, a.pts, a.n_points, a.nodes, a.leaves, a.src, a.n,
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

static_assert(sizeof(bvh_knn_hit) == sizeof(uint2), "a record is two words: dist2's bits, then prim_idx");

void launch_radius_count(hipStream_t s, int layout, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                         const void* d_points, uint32_t n_points, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets,
                         uint32_t* d_overflow, const uint32_t* d_parent, uint64_t* d_sums, uint64_t* d_total) {
    const RadiusArgs a{ s, (const bvh_point_query*)d_points, n_points, (const bvh2_node*)d_nodes, (const bvh_primref*)d_leaves,
                        TriSrc{ d_tris, (const float*)d_vertices, (const u32*)d_indices, n_vertices }, n, root, d_offsets, nullptr, nullptr, 0, d_overflow, d_parent };
    radius_pass<false, false>(a, layout, tri_format);
    launch_overlap_scan(s, d_offsets, n_points, d_sums, d_total);
}

void launch_radius_fill(hipStream_t s, int layout, int tri_format, int sorted, const void* d_tris, const void* d_vertices, const void* d_indices,
                        uint32_t n_vertices, const void* d_points, uint32_t n_points, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root,
                        uint32_t* d_offsets, void* d_hits, uint64_t capacity, const uint64_t* d_total, uint32_t* d_overflow, const uint32_t* d_parent) {
    const RadiusArgs a{ s, (const bvh_point_query*)d_points, n_points, (const bvh2_node*)d_nodes, (const bvh_primref*)d_leaves,
                        TriSrc{ d_tris, (const float*)d_vertices, (const u32*)d_indices, n_vertices }, n, root, d_offsets, (uint2*)d_hits, d_total, capacity,
                        d_overflow, d_parent };
    if (sorted) radius_pass<true, true>(a, layout, tri_format); else radius_pass<true, false>(a, layout, tri_format);
}

void warm_radius() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_radius_walk<0, BVH_TRI_PADDED64, false, false>));
}

} // namespace bvh
