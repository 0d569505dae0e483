// closest_tris.hip — bvh_closest_tris on gfx950: the nearest triangle of a built BVH2 to each triangle of another mesh, and the squared distance between the two
// (no counterpart in the reference).  One query triangle per lane, templated on node layout, query kind and the TREE's triangle format; the query mesh's format is
// switched at run time (one fetch per lane, outside the loop), as in intersect_tris.hip.  The traversal is point_query.hip's with a box-box distance test.
//   k_closest_tris      : near-child-first traversal with a short per-lane stack in LDS (QUERY_STACK entries).  Leaf children whose box passes are tested at
//                         once — both through ONE copy of the leaf routine (a two-trip loop that is not unrolled: the routine is six point-triangle and nine
//                         segment-segment terms and, where the boxes overlap, up to 24 f64 determinants); of two internal children the one with the smaller box
//                         lower bound is entered and the other pushed.  A query whose push would overflow (or whose walk exceeds the node count: arrays that are
//                         not a tree) writes QUERY_MARK into its record's prim_idx and bumps the overflow word.
//   k_closest_tris_deep : launched every time, returns at once while the overflow word is 0; otherwise re-walks the marked queries stackless through the parent
//                         links of bvh_refit's plan (k_refit_plan), left child first, testing each node's own box on the way down.  Correct at any depth.
// The candidate of a pair (tt_dist2, closest_tris.hpp, shared with scene_closest_tris.hip; the header's contract, restated in numpy by tests/test_closest_tris.py): a proper crossing (tri_cross.hpp's predicate,
// evaluated only where the two stage-E boxes overlap) is distance 0, feature 15; otherwise the smallest of 15 f32 terms — the three vertices of the query against
// the tree triangle and the reverse (tri_closest, query.hpp), and the nine edge pairs (seg_seg_dist2, Ericson's ClosestPtSegmentSegment).  The term loops are NOT
// unrolled and pick their operands with selects on the (wave-uniform) trip count: one copy of each formula, two triangles live (18 floats) and no indexed
// register array, so nothing goes to scratch.  A running minimum that reaches exactly 0 ends the terms at once (no term is below 0, and the first index that
// attains the minimum is the one reported), in both query kinds; BVH_QUERY_ANY additionally ends the WALK at the first accepted candidate.
// Box tests are conservative (box_box_dist_pass): every node box grows by QUERY_GROW * (its largest |coordinate|), the query's stage-E box once the
// same way, and a subtree is kept while the f32 sum of the squared per-axis gaps times (1 - 2^-20) is <= the best dist2 so far.  A leaf pair whose own two
// triangle boxes already fail that test against the current best is skipped before any term is computed.
// Built WITHOUT the SLP vectoriser (Makefile): the (dist2, prim) record update is point_query.hip's tie-breaking pattern.
#include <type_traits>
#include "query.hpp"
#include "tri_cross.hpp"
#include "closest_tris.hpp"
#include "kernels.hpp"

namespace bvh {

// the candidate prim's test and the record update; true when an any-hit query is done.  xg: the query's grown box (box_grown(xb))
template <int QUERY, int TFMT>
__device__ __forceinline__ bool leaf_tris(const TriSrc& tsrc, u32 prim, QF3 x1, QF3 x2, QF3 x3, bool xproper, const Box& xb, const Box& xg, TBest& best) {
    QF3 y1, y2, y3; tri_fetch<TFMT>(tsrc, prim, y1, y2, y3);
    const Box yb = tt_box(y1, y2, y3);
    float lb;
    if (!box_box_dist_pass(yb, xg, best.d2, lb)) return false;    // the pair's own boxes are already too far apart for the current best
    u32 feat;
    const float d2 = tt_dist2(x1, x2, x3, xproper, xb, y1, y2, y3, yb, feat);
    // closest: (d2, prim) below the best; best starts at {r2, INV}, so this is also the acceptance test d2 <= r2 (NaN fails both comparisons)
    if (!(d2 < best.d2 || (d2 == best.d2 && prim < best.prim))) return false;
    best.d2 = d2; best.prim = prim; best.feat = feat;
    return QUERY == BVH_QUERY_ANY;
}

template <int LAYOUT, int QUERY, int TFMT>
__global__ __launch_bounds__(QUERY_BLOCK) void k_closest_tris(TriSrc qsrc, int qfmt, u32 n_queries, float radius, const bvh2_node* __restrict__ nodes,
                                                              const bvh_primref* __restrict__ leaves, TriSrc tsrc, u32 n, u32 root,
                                                              bvh_tri_hit* __restrict__ hits, u32* __restrict__ overflow) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= n_queries) return;
    u32* const stack = s_stack + tid_x();
    QF3 x1, x2, x3; float r2;
    const bool live = tris_query_load(qfmt, qsrc, i, radius, x1, x2, x3, r2);
    TBest best{ r2, INV, 0u };
    bool deep = false;
    if (live) {
        const Box xb = tt_box(x1, x2, x3), xg = box_grown(xb);
        const bool xproper = tt_proper(x1, x2, x3);
        const u32 ni = n - 1, total = 2 * n - 1;
        u32 nl, nr; { const uint2 lr = *reinterpret_cast<const uint2*>(nodes + root); nl = lr.x; nr = lr.y; }
        u32 top = 0, steps = 0;
        for (;;) {
            if (++steps > n) { deep = true; break; }              // more expansions than internal nodes: not a tree (a tree never gets here)
            u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
            Box ba, bb;
            float la = 0.0f, lb = 0.0f;
            bool ha = false, hb = false;
            if (nl < total) { rec_fetch<LAYOUT>(nodes, leaves, nl, ni, a0, a1, ba); ha = box_box_dist_pass(ba, xg, best.d2, la); }
            if (nr < total) { rec_fetch<LAYOUT>(nodes, leaves, nr, ni, b0, b1, bb); hb = box_box_dist_pass(bb, xg, best.d2, lb); }
            u32 pa = INV, pb = INV;                               // the leaf children that passed: their primitives, left first (out of range: never followed)
            if (ha && nl >= ni) { if (a0 < n) pa = a0; ha = false; }
            if (hb && nr >= ni) { if (b0 < n) pb = b0; hb = false; }
            if (pa == INV) { pa = pb; pb = INV; }
            bool done = false;
#pragma unroll 1
            while (pa != INV) {
                done = leaf_tris<QUERY, TFMT>(tsrc, pa, x1, x2, x3, xproper, xb, xg, best);
                if (done) break;
                pa = pb; pb = INV;
            }
            if (done) break;
            if (ha && hb) {
                const bool left_first = la <= lb;
                if (top == (u32)QUERY_STACK) { deep = true; break; }
                stack[top * QUERY_BLOCK] = left_first ? nr : nl; ++top;
                nl = left_first ? a0 : b0; nr = left_first ? a1 : b1;
            } else if (ha) { nl = a0; nr = a1; }
            else if (hb) { nl = b0; nr = b1; }
            else {
                if (top == 0) break;
                const u32 node = stack[--top * QUERY_BLOCK];
                const uint2 lr = *reinterpret_cast<const uint2*>(nodes + node);
                nl = lr.x; nr = lr.y;
            }
        }
    }
    if (deep) {
        const TBest mark{ r2, QUERY_MARK, 0u };
        tri_hit_store(hits, i, mark); atomicAdd(overflow, 1u);
    } else tri_hit_store(hits, i, best);
}

// the stackless re-walk of the marked queries: parent links of the plan, left child first
template <int LAYOUT, int QUERY, int TFMT>
__global__ __launch_bounds__(QUERY_BLOCK) void k_closest_tris_deep(TriSrc qsrc, int qfmt, u32 n_queries, float radius, const bvh2_node* __restrict__ nodes,
                                                                   const bvh_primref* __restrict__ leaves, TriSrc tsrc, u32 n, u32 root,
                                                                   bvh_tri_hit* __restrict__ hits, const u32* __restrict__ overflow,
                                                                   const u32* __restrict__ parent) {
    if (*overflow == 0u) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < n_queries; i += nbid_x() * QUERY_BLOCK) {
        if (reinterpret_cast<const u32*>(hits + i)[1] != QUERY_MARK) continue;
        QF3 x1, x2, x3; float r2;
        tris_query_load(qfmt, qsrc, i, radius, x1, x2, x3, r2);   // (a marked query passed the checks)
        const Box xb = tt_box(x1, x2, x3), xg = box_grown(xb);
        const bool xproper = tt_proper(x1, x2, x3);
        TBest best{ r2, INV, 0u };
        u32 cur = root, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < total && steps < bound; ++steps) {
            u32 w0, w1; Box b;
            if (down) {
                rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                float lb;
                const bool pass = box_box_dist_pass(b, xg, best.d2, lb);
                if (cur >= ni) {
                    if (pass && w0 < n && leaf_tris<QUERY, TFMT>(tsrc, w0, x1, x2, x3, xproper, xb, xg, best)) break;
                    last = cur; cur = parent[cur]; down = false;
                    continue;
                }
                if (!pass) { last = cur; cur = parent[cur]; down = false; continue; }
                if (w0 < total) { cur = w0; continue; }
                last = w0; down = false;                          // (a left link out of range: as if its subtree were done)
                continue;
            }
            if (cur >= ni) break;                                 // (parent links are internal nodes or INVALID)
            const uint2 lr = *reinterpret_cast<const uint2*>(nodes + cur);
            if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
            last = cur; cur = parent[cur];
        }
        tri_hit_store(hits, i, best);
    }
}

void launch_closest_tris(hipStream_t s, int layout, int query, const TrisMesh& tree_tris, const TrisMesh& queries, uint32_t n_queries, float radius,
                         const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, void* d_hits, uint32_t* d_overflow, const uint32_t* d_parent) {
    const TriSrc tsrc{ tree_tris.d_tris, (const float*)tree_tris.d_vertices, (const u32*)tree_tris.d_indices, tree_tris.n_vertices };
    const TriSrc qsrc{ queries.d_tris, (const float*)queries.d_vertices, (const u32*)queries.d_indices, queries.n_vertices };
    const int qfmt = queries.tri_format;
    const u32 blocks = (n_queries + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    const bvh2_node* nodes = (const bvh2_node*)d_nodes; const bvh_primref* leaves = (const bvh_primref*)d_leaves;
    bvh_tri_hit* hits = (bvh_tri_hit*)d_hits;
    auto go = [&](auto L, auto Q, auto F) {
        constexpr int LA = decltype(L)::value, QU = decltype(Q)::value, FM = decltype(F)::value;
        { KernelScope ks(s, "k_closest_tris");
          hipLaunchKernelGGL((k_closest_tris<LA, QU, FM>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, qsrc, qfmt, n_queries, radius, nodes, leaves, tsrc, n, root, hits,
                             d_overflow); }
        { KernelScope ks(s, "k_closest_tris_deep");
          hipLaunchKernelGGL((k_closest_tris_deep<LA, QU, FM>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, qsrc, qfmt, n_queries, radius, nodes, leaves, tsrc, n,
                             root, hits, (const u32*)d_overflow, d_parent); }
    };
    using L0 = std::integral_constant<int, 0>; using L1 = std::integral_constant<int, 1>;
    auto by_fmt = [&](auto L, auto Q) {
        switch (tree_tris.tri_format) {
            case BVH_TRI_PADDED64: go(L, Q, std::integral_constant<int, BVH_TRI_PADDED64>{}); break;
            case BVH_TRI_PACKED36: go(L, Q, std::integral_constant<int, BVH_TRI_PACKED36>{}); break;
            default:               go(L, Q, std::integral_constant<int, BVH_TRI_INDEXED>{}); break;
        }
    };
    auto by_query = [&](auto L) {
        if (query == BVH_QUERY_ANY) by_fmt(L, std::integral_constant<int, BVH_QUERY_ANY>{});
        else by_fmt(L, std::integral_constant<int, BVH_QUERY_CLOSEST>{});
    };
    if (layout == 0) by_query(L0{}); else by_query(L1{});
}

void warm_closest_tris() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_closest_tris<0, BVH_QUERY_CLOSEST, BVH_TRI_PADDED64>));
}

} // namespace bvh
