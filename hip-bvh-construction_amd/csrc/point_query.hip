// point_query.hip — bvh_closest_point on gfx950: closest-point / any-within-radius queries against a built BVH2 in either node layout (no counterpart in the
// reference).  One query per lane, templated on node layout, query kind and triangle format; the traversal is query.hip's with a distance test for the slab test.
//   k_closest_point      : near-child-first traversal with a short per-lane stack in LDS (QUERY_STACK entries).  Leaf children whose box passes are tested at
//                          once; of two internal children the one with the smaller box lower bound is entered and the other pushed.  A query whose push would
//                          overflow (or whose walk exceeds the node count: arrays that are not a tree) writes QUERY_MARK into its hit record and bumps the
//                          overflow word.
//   k_closest_point_deep : launched every time, returns at once while the overflow word is 0; otherwise re-walks the marked queries stackless through the parent
//                          links of bvh_refit's plan (k_refit_plan), left child first, testing each node's own box on the way down.  Correct at any depth.
// Box tests are conservative (box_dist_pass): every box grows by QUERY_GROW * (its largest |coordinate|), and a subtree is kept while its f32
// squared distance times (1 - 2^-20) is <= the best dist2 so far, so that a candidate at the current best dist2 (a tie with a smaller prim index) is still
// reached.  The candidate is Ericson's ClosestPtPointTriangle (tri_closest, query.hpp).
// Built without the SLP vectoriser (Makefile), as scene.o: the closest record update is the same tie-breaking pattern that it broke there.
#include <type_traits>
#include "query.hpp"
#include "kernels.hpp"

namespace bvh {

// the best candidate so far: closest point, dist2, weights, prim (INV: none)
struct PBest { QF3 q; float d2, u, v; u32 prim; };

// the candidate prim's test and the record update; true when an any-hit query is done
template <int QUERY, int FMT>
__device__ __forceinline__ bool leaf_point(const TriSrc& src, u32 prim, u32 n, QF3 p, PBest& best) {
    if (prim >= n) return false;                                  // (never in a tree: not followed)
    QF3 a, b, c; tri_fetch<FMT>(src, prim, a, b, c);
    QF3 q; float u, v;
    const float d2 = tri_closest(a, b, c, p, q, u, v);
    // closest: (d2, prim) below the best; best starts at {r2, INV}, so this is also the acceptance test d2 <= r2 (NaN fails both comparisons)
    if (!(d2 < best.d2 || (d2 == best.d2 && prim < best.prim))) return false;
    best.q = q; best.d2 = d2; best.u = u; best.v = v; best.prim = prim;
    return QUERY == BVH_QUERY_ANY;
}

__device__ __forceinline__ void point_hit_store(bvh_point_hit* hits, u32 i, const PBest& b) {
    float4* h = reinterpret_cast<float4*>(hits + i);
    const bool hit = b.prim != INV;
    h[0] = hit ? make_float4(b.q.x, b.q.y, b.q.z, b.d2) : make_float4(0.0f, 0.0f, 0.0f, b.d2);
    h[1] = hit ? make_float4(b.u, b.v, __uint_as_float(b.prim), 0.0f) : make_float4(0.0f, 0.0f, __uint_as_float(INV), 0.0f);
}

template <int LAYOUT, int QUERY, int FMT>
__global__ __launch_bounds__(QUERY_BLOCK) void k_closest_point(const bvh_point_query* __restrict__ pts, u32 n_points, const bvh2_node* __restrict__ nodes,
                                                               const bvh_primref* __restrict__ leaves, TriSrc src, u32 n, u32 root,
                                                               bvh_point_hit* __restrict__ hits, u32* __restrict__ overflow) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= n_points) return;
    u32* const stack = s_stack + tid_x();
    QF3 p; float r2;
    const bool live = point_load(pts, i, p, r2);
    PBest best{ { 0.0f, 0.0f, 0.0f }, r2, 0.0f, 0.0f, INV };
    bool deep = false;
    if (live) {
        const u32 ni = n - 1, total = 2 * n - 1;
        u32 nl, nr; { const uint2 lr = *reinterpret_cast<const uint2*>(nodes + root); nl = lr.x; nr = lr.y; }
        u32 top = 0, steps = 0;
        for (;;) {
            if (++steps > n) { deep = true; break; }              // more expansions than internal nodes: not a tree (a tree never gets here)
            u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
            Box ba, bb;
            float la = 0.0f, lb = 0.0f;
            bool ha = false, hb = false;
            if (nl < total) { rec_fetch<LAYOUT>(nodes, leaves, nl, ni, a0, a1, ba); ha = box_dist_pass(ba, p, best.d2, la); }
            if (nr < total) { rec_fetch<LAYOUT>(nodes, leaves, nr, ni, b0, b1, bb); hb = box_dist_pass(bb, p, best.d2, lb); }
            bool done = false;
            if (ha && nl >= ni) { done = leaf_point<QUERY, FMT>(src, a0, n, p, best); ha = false; }
            if (hb && nr >= ni && !done) { done = leaf_point<QUERY, FMT>(src, b0, n, p, best); hb = false; }
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
        const PBest mark{ { 0.0f, 0.0f, 0.0f }, r2, 0.0f, 0.0f, QUERY_MARK };
        point_hit_store(hits, i, mark); atomicAdd(overflow, 1u);
    } else point_hit_store(hits, i, best);
}

// the stackless re-walk of the marked queries: parent links of the plan, left child first
template <int LAYOUT, int QUERY, int FMT>
__global__ __launch_bounds__(QUERY_BLOCK) void k_closest_point_deep(const bvh_point_query* __restrict__ pts, u32 n_points, const bvh2_node* __restrict__ nodes,
                                                                    const bvh_primref* __restrict__ leaves, TriSrc src, u32 n, u32 root,
                                                                    bvh_point_hit* __restrict__ hits, const u32* __restrict__ overflow,
                                                                    const u32* __restrict__ parent) {
    if (*overflow == 0u) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < n_points; i += nbid_x() * QUERY_BLOCK) {
        if (reinterpret_cast<const u32*>(hits + i)[6] != QUERY_MARK) continue;
        QF3 p; float r2;
        point_load(pts, i, p, r2);                                // (a marked query passed the checks)
        PBest best{ { 0.0f, 0.0f, 0.0f }, r2, 0.0f, 0.0f, INV };
        u32 cur = root, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < total && steps < bound; ++steps) {
            u32 w0, w1; Box b;
            if (down) {
                if (cur >= ni) {
                    rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                    float lb;
                    if (box_dist_pass(b, p, best.d2, lb) && leaf_point<QUERY, FMT>(src, w0, n, p, best)) break;
                    last = cur; cur = parent[cur]; down = false;
                    continue;
                }
                rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                float lb;
                if (!box_dist_pass(b, p, best.d2, lb)) { last = cur; cur = parent[cur]; down = false; continue; }
                if (w0 < total) { cur = w0; continue; }
                last = w0; down = false;                          // (a left link out of range: as if its subtree were done)
                continue;
            }
            if (cur >= ni) break;                                 // (parent links are internal nodes or INVALID)
            const uint2 lr = *reinterpret_cast<const uint2*>(nodes + cur);
            if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
            last = cur; cur = parent[cur];
        }
        point_hit_store(hits, i, best);
    }
}

void launch_closest_point(hipStream_t s, int layout, int query, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices,
                          uint32_t n_vertices, const void* d_points, uint32_t n_points, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root,
                          void* d_hits, uint32_t* d_overflow, const uint32_t* d_parent) {
    const TriSrc src{ d_tris, (const float*)d_vertices, (const u32*)d_indices, n_vertices };
    const u32 blocks = (n_points + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    const bvh_point_query* pts = (const bvh_point_query*)d_points; const bvh2_node* nodes = (const bvh2_node*)d_nodes;
    const bvh_primref* leaves = (const bvh_primref*)d_leaves;
    bvh_point_hit* hits = (bvh_point_hit*)d_hits;
    auto go = [&](auto L, auto Q, auto F) {
        constexpr int LA = decltype(L)::value, QU = decltype(Q)::value, FM = decltype(F)::value;
        { KernelScope ks(s, "k_closest_point");
          hipLaunchKernelGGL((k_closest_point<LA, QU, FM>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, pts, n_points, nodes, leaves, src, n, root, hits, d_overflow); }
        { KernelScope ks(s, "k_closest_point_deep");
          hipLaunchKernelGGL((k_closest_point_deep<LA, QU, FM>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, pts, n_points, nodes, leaves, src, n, root, hits,
                             (const u32*)d_overflow, d_parent); }
    };
    using L0 = std::integral_constant<int, 0>; using L1 = std::integral_constant<int, 1>;
    auto by_fmt = [&](auto L, auto Q) {
        switch (tri_format) {
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

void warm_point_query() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_closest_point<0, BVH_QUERY_CLOSEST, BVH_TRI_PADDED64>));
}

} // namespace bvh
