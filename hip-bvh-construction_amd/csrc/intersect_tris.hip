// intersect_tris.hip — bvh_intersect_tris on gfx950: which triangles of a built BVH2 does each query triangle properly cross (no counterpart in the reference).
// bvh_overlap's broad phase (overlap.hip) with the exact narrow phase run at the leaf, so no pair list travels through HBM: count -> scan -> fill, count and
// fill the SAME walk, templated on node layout, the tree's triangle format, pass and mode.  The scan is bvh_overlap's (launch_overlap_scan).
//   k_tris_walk  : one query triangle per lane, 64-lane workgroups, short per-lane stack in LDS (QUERY_STACK entries, query.hip's layout).  The query's box is
//                  stage E's box of its three vertices (stage_e_box, common.hpp: the expression k_extents* evaluates, clamps included).  Per internal node both
//                  children's records are fetched (rec_fetch) and tested with box_overlap; a leaf child that passes fetches its triangle (tri_fetch) and runs the
//                  f64 predicate at once — both children's leaves go through ONE copy of the predicate (a two-trip loop that is not unrolled: the predicate is 24
//                  determinants, and lanes whose left child is the leaf run it together with lanes whose right child is).  Of two passing internal children the
//                  left one is entered and the right one pushed.  A query whose push would overflow (or whose walk exceeds the node count: arrays that are not a
//                  tree) is marked and bumps the pass's overflow word, exactly as in k_overlap_walk.
//   k_tris_deep  : launched after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked query from its start, stackless
//                  through the parent links of bvh_refit's plan, left child first.  Both walks report exactly the leaves whose own box and every box above them
//                  (the root's excepted) overlap the query's box and whose triangle crosses the query's, so count and fill agree whichever walk served a query.
// The predicate (the header's contract, restated in numpy by tests/test_intersect_tris.py) lives in tri_cross.hpp, which scene_tris.hip shares.
// The query triangles' format is switched at run time (one fetch per lane, outside the loop); the tree's is a template parameter (one fetch per leaf test).
// Built WITHOUT the SLP vectoriser (Makefile): see there.
#include <type_traits>
#include "query.hpp"
#include "tri_cross.hpp"
#include "kernels.hpp"

namespace bvh {

// where a walk's results go (overlap.hip's Sink): a counter, or the query's slice [out, out + room) of d_prims, never written past its end
template <bool FILL> struct TrisSink {
    u32* out; u32 room, k = 0;
    __device__ __forceinline__ void put(u32 prim) { if (FILL) { if (k < room) out[k] = prim; } ++k; }
};

// a leaf child's primitive: in range (never followed otherwise) and, in self mode, above the query's own index (every unordered pair once)
template <bool SELF> __device__ __forceinline__ bool tt_prim_ok(u32 prim, u32 n, u32 i) { return prim < n && (!SELF || prim > i); }

template <int LAYOUT, int TFMT, bool FILL, bool SELF>
__global__ __launch_bounds__(QUERY_BLOCK) void k_tris_walk(TriSrc qsrc, int qfmt, u32 n_queries, const bvh2_node* __restrict__ nodes,
                                                           const bvh_primref* __restrict__ leaves, TriSrc tsrc, u32 n, u32 root, u32* __restrict__ offsets,
                                                           u32* __restrict__ prims, const u64* __restrict__ total_word, u64 capacity, u32* __restrict__ overflow) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 t = *total_word; if (t > capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= n_queries) return;
    TrisSink<FILL> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = offsets[i], end = offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = prims + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    QF3 x1, x2, x3;
    tri_fetch_rt(qfmt, qsrc, i, x1, x2, x3);
    const Box q = tt_box(x1, x2, x3);
    bool deep = false;
    if (box_valid(q) && tt_proper(x1, x2, x3)) {                  // (an axis that is all NaN or all +inf keeps the reset planes: inverted, overlaps nothing; a
                                                                  // query triangle that is not proper crosses nothing)
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
            u32 pa = INV, pb = INV;                               // the leaf children that passed: their primitives, left first
            if (ha && nl >= ni) { if (tt_prim_ok<SELF>(a0, n, i)) pa = a0; ha = false; }
            if (hb && nr >= ni) { if (tt_prim_ok<SELF>(b0, n, i)) pb = b0; hb = false; }
            if (pa == INV) { pa = pb; pb = INV; }
#pragma unroll 1
            while (pa != INV) {
                QF3 y1, y2, y3;
                tri_fetch<TFMT>(tsrc, pa, y1, y2, y3);
                if (tt_proper(y1, y2, y3) && tt_crosses(x1, x2, x3, y1, y2, y3)) sink.put(pa);
                pa = pb; pb = INV;
            }
            if (ha || hb) {
                if (ha && hb) {
                    if (top == (u32)QUERY_STACK) { deep = true; break; }
                    stack[top * QUERY_BLOCK] = nr; ++top;
                }
                nl = ha ? a0 : b0; nr = ha ? a1 : b1;             // (selects of values, as k_overlap_walk)
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
template <int LAYOUT, int TFMT, bool FILL, bool SELF>
__global__ __launch_bounds__(QUERY_BLOCK) void k_tris_deep(TriSrc qsrc, int qfmt, u32 n_queries, const bvh2_node* __restrict__ nodes,
                                                           const bvh_primref* __restrict__ leaves, TriSrc tsrc, u32 n, u32 root, u32* __restrict__ offsets,
                                                           u32* __restrict__ prims, const u32* __restrict__ overflow, const u32* __restrict__ parent) {
    if (*overflow == 0u) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < n_queries; i += nbid_x() * QUERY_BLOCK) {
        TrisSink<FILL> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = offsets[i], end = offsets[i + 1];
            if (end <= base || prims[base] != QUERY_MARK) continue;
            sink.out = prims + base; sink.room = end - base;
        } else if (offsets[i] != QUERY_MARK) continue;
        QF3 x1, x2, x3;
        tri_fetch_rt(qfmt, qsrc, i, x1, x2, x3);
        const Box q = tt_box(x1, x2, x3);                         // (a marked query passed box_valid and tt_proper)
        u32 cur = root, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < total && steps < bound; ++steps) {
            if (down) {
                u32 w0, w1; Box b;
                rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                if (cur >= ni) {
                    if (box_overlap(q, b) && tt_prim_ok<SELF>(w0, n, i)) {
                        QF3 y1, y2, y3;
                        tri_fetch<TFMT>(tsrc, w0, y1, y2, y3);
                        if (tt_proper(y1, y2, y3) && tt_crosses(x1, x2, x3, y1, y2, y3)) sink.put(w0);
                    }
                    last = cur; cur = parent[cur]; down = false;
                    continue;
                }
                if (cur != root && !box_overlap(q, b)) { last = cur; cur = parent[cur]; down = false; continue; }   // (the root's own box: as k_tris_walk, not tested)
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
struct TrisPass {
    hipStream_t s; TriSrc qsrc; int qfmt; u32 n_queries; const bvh2_node* nodes; const bvh_primref* leaves; TriSrc tsrc; u32 n, root; u32* offsets; u32* prims;
    const u64* total; u64 capacity; u32* overflow; const u32* parent;
};

template <bool FILL>
void tris_pass(const TrisPass& a, int layout, int tri_format, int mode) {
    const u32 blocks = (a.n_queries + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    auto go = [&](auto L, auto F, auto S) {
        constexpr int LA = decltype(L)::value, FM = decltype(F)::value; constexpr bool SE = decltype(S)::value;
        { KernelScope ks(a.s, FILL ? "k_tris_fill" : "k_tris_count");
          hipLaunchKernelGGL((k_tris_walk<LA, FM, FILL, SE>), dim3(blocks), dim3(QUERY_BLOCK), 0, a.s, a.qsrc, a.qfmt, a.n_queries, a.nodes, a.leaves, a.tsrc, a.n,
                             a.root, a.offsets, a.prims, a.total, a.capacity, a.overflow); }
        { KernelScope ks(a.s, "k_tris_deep");                     // (the fill's overflow word stays 0 when the fill returned at once)
          hipLaunchKernelGGL((k_tris_deep<LA, FM, FILL, SE>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, a.s, a.qsrc, a.qfmt, a.n_queries, a.nodes, a.leaves, a.tsrc,
                             a.n, a.root, a.offsets, a.prims, (const u32*)a.overflow, a.parent); }
    };
    auto by_mode = [&](auto L, auto F) { if (mode == BVH_TRIS_SELF) go(L, F, std::true_type{}); else go(L, F, std::false_type{}); };
    auto by_fmt = [&](auto L) {
        switch (tri_format) {
            case BVH_TRI_PADDED64: by_mode(L, std::integral_constant<int, BVH_TRI_PADDED64>{}); break;
            case BVH_TRI_PACKED36: by_mode(L, std::integral_constant<int, BVH_TRI_PACKED36>{}); break;
            default:               by_mode(L, std::integral_constant<int, BVH_TRI_INDEXED>{}); break;
        }
    };
    if (layout == 0) by_fmt(std::integral_constant<int, 0>{}); else by_fmt(std::integral_constant<int, 1>{});
}
} // namespace

void launch_tris_count(hipStream_t s, int layout, int mode, const TrisMesh& tree_tris, const TrisMesh& queries, uint32_t n_queries, const void* d_nodes,
                       const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, uint32_t* d_overflow, const uint32_t* d_parent, uint64_t* d_sums,
                       uint64_t* d_total) {
    const TrisPass a{ s, TriSrc{ queries.d_tris, (const float*)queries.d_vertices, (const u32*)queries.d_indices, queries.n_vertices }, queries.tri_format, n_queries,
                      (const bvh2_node*)d_nodes, (const bvh_primref*)d_leaves,
                      TriSrc{ tree_tris.d_tris, (const float*)tree_tris.d_vertices, (const u32*)tree_tris.d_indices, tree_tris.n_vertices }, n, root, d_offsets, nullptr,
                      nullptr, 0, d_overflow, d_parent };
    tris_pass<false>(a, layout, tree_tris.tri_format, mode);
    launch_overlap_scan(s, d_offsets, n_queries, d_sums, d_total);
}

void launch_tris_fill(hipStream_t s, int layout, int mode, const TrisMesh& tree_tris, const TrisMesh& queries, uint32_t n_queries, const void* d_nodes,
                      const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, uint32_t* d_prims, uint64_t capacity, const uint64_t* d_total,
                      uint32_t* d_overflow, const uint32_t* d_parent) {
    const TrisPass a{ s, TriSrc{ queries.d_tris, (const float*)queries.d_vertices, (const u32*)queries.d_indices, queries.n_vertices }, queries.tri_format, n_queries,
                      (const bvh2_node*)d_nodes, (const bvh_primref*)d_leaves,
                      TriSrc{ tree_tris.d_tris, (const float*)tree_tris.d_vertices, (const u32*)tree_tris.d_indices, tree_tris.n_vertices }, n, root, d_offsets, d_prims,
                      d_total, capacity, d_overflow, d_parent };
    tris_pass<true>(a, layout, tree_tris.tri_format, mode);
}

void warm_tris() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_tris_walk<0, BVH_TRI_PADDED64, false, false>));
}

} // namespace bvh
