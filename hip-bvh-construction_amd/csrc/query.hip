// query.hip — bvh_intersect on gfx950: closest-hit / any-hit ray queries against a built BVH2 in either node layout (no counterpart in the reference;
// trace.hip's kernels restate the reference's image kernels and stay as they are).  One ray per lane, templated on node layout, query kind and triangle format.
//   k_intersect      : near-child-first traversal with a short per-lane stack in LDS (QUERY_STACK entries).  Leaf children whose box passes are tested at once;
//                      of two internal children the nearer is entered and the other pushed.  A ray whose push would overflow (or whose walk exceeds the node
//                      count: arrays that are not a tree) writes QUERY_MARK into its hit record and bumps the overflow word.
//   k_intersect_deep : launched every time, returns at once while the overflow word is 0; otherwise re-traverses the marked rays stackless through the parent
//                      links of bvh_refit's plan (k_refit_plan), left child first, testing each node's own box on the way down.  Correct at any depth.
// Box tests are conservative: every box is grown on every axis by QUERY_GROW * (its largest |coordinate|), the slab interval of the ray's sign-ordered planes
// is widened by QUERY_REL relative on both ends, and compared against [tmin, best t] so that a hit at the current best t (a tie with a smaller prim index) is
// still reached.  Zero direction components give 1/0 = inf; the 0 * inf = NaN of an origin on a plane is read as "no constraint" by the NaN-dropping fminf / fmaxf,
// which is the right answer for the sign-ordered planes.  The triangle test is the reference's intersectTriangle (src/Common.h:516-531) without a transform.
// Compiled WITHOUT -fno-honor-nans / -mno-amdgpu-ieee (Makefile): the slab test relies on fminf / fmaxf dropping NaN operands.
#include <type_traits>
#include "query.hpp"
#include "kernels.hpp"

namespace bvh {

// the candidate prim's test and the record update; true when an any-hit query is done
template <int QUERY, int FMT>
__device__ __forceinline__ bool leaf_test(const TriSrc& src, u32 prim, u32 n, const QRay& r, float& bt, float& bu, float& bv, u32& bp) {
    if (prim >= n) return false;                                  // (never in a tree: not followed)
    QF3 a, b, c; tri_fetch<FMT>(src, prim, a, b, c);
    float it, iu, iv;
    if (!tri_hit(a, b, c, r, it, iu, iv) || !(r.tmin < it && it < r.tmax)) return false;
    if (QUERY == BVH_QUERY_CLOSEST && !(it < bt || (it == bt && prim < bp))) return false;
    bt = it; bu = iu; bv = iv; bp = prim;
    return QUERY == BVH_QUERY_ANY;
}

__device__ __forceinline__ void hit_store(bvh_hit* hits, u32 i, float t, float u, float v, u32 prim) {
    reinterpret_cast<float4*>(hits)[i] = make_float4(t, u, v, __uint_as_float(prim));
}

template <int LAYOUT, int QUERY, int FMT>
__global__ __launch_bounds__(QUERY_BLOCK) void k_intersect(const bvh_ray* __restrict__ rays, u32 n_rays, const bvh2_node* __restrict__ nodes,
                                                           const bvh_primref* __restrict__ leaves, TriSrc src, u32 n, u32 root, bvh_hit* __restrict__ hits,
                                                           u32* __restrict__ overflow) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= n_rays) return;
    u32* const stack = s_stack + tid_x();
    QRay r;
    const bool live = ray_load(rays, i, r);
    float bt = r.tmax, bu = 0.0f, bv = 0.0f;
    u32 bp = INV;
    bool deep = false;
    if (live) {
        const u32 ni = n - 1, total = 2 * n - 1;
        u32 nl, nr; { const uint2 lr = *reinterpret_cast<const uint2*>(nodes + root); nl = lr.x; nr = lr.y; }
        u32 top = 0, steps = 0;
        for (;;) {
            if (++steps > n) { deep = true; break; }              // more expansions than internal nodes: not a tree (a tree never gets here)
            u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
            Box ba, bb;
            float ta = 0.0f, tb = 0.0f;
            bool ha = false, hb = false;
            if (nl < total) { rec_fetch<LAYOUT>(nodes, leaves, nl, ni, a0, a1, ba); ha = box_pass(ba, r, bt, ta); }
            if (nr < total) { rec_fetch<LAYOUT>(nodes, leaves, nr, ni, b0, b1, bb); hb = box_pass(bb, r, bt, tb); }
            bool done = false;
            if (ha && nl >= ni) { done = leaf_test<QUERY, FMT>(src, a0, n, r, bt, bu, bv, bp); ha = false; }
            if (hb && nr >= ni && !done) { done = leaf_test<QUERY, FMT>(src, b0, n, r, bt, bu, bv, bp); hb = false; }
            if (done) break;
            if (ha && hb) {
                const bool left_first = ta <= tb;
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
    if (deep) { hit_store(hits, i, r.tmax, 0.0f, 0.0f, QUERY_MARK); atomicAdd(overflow, 1u); }
    else hit_store(hits, i, bt, bu, bv, bp);
}

// the stackless re-traversal of the marked rays: parent links of the plan, left child first
template <int LAYOUT, int QUERY, int FMT>
__global__ __launch_bounds__(QUERY_BLOCK) void k_intersect_deep(const bvh_ray* __restrict__ rays, u32 n_rays, const bvh2_node* __restrict__ nodes,
                                                                const bvh_primref* __restrict__ leaves, TriSrc src, u32 n, u32 root, bvh_hit* __restrict__ hits,
                                                                const u32* __restrict__ overflow, const u32* __restrict__ parent) {
    if (*overflow == 0u) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < n_rays; i += nbid_x() * QUERY_BLOCK) {
        if (__float_as_uint(reinterpret_cast<const float4*>(hits)[i].w) != QUERY_MARK) continue;
        QRay r;
        ray_load(rays, i, r);                                     // (a marked ray passed the checks)
        float bt = r.tmax, bu = 0.0f, bv = 0.0f;
        u32 bp = INV;
        u32 cur = root, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < total && steps < bound; ++steps) {
            u32 w0, w1; Box b;
            if (down) {
                if (cur >= ni) {
                    rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                    if (leaf_test<QUERY, FMT>(src, w0, n, r, bt, bu, bv, bp)) break;
                    last = cur; cur = parent[cur]; down = false;
                    continue;
                }
                rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                float tn;
                if (!box_pass(b, r, bt, tn)) { last = cur; cur = parent[cur]; down = false; continue; }
                if (w0 < total) { cur = w0; continue; }
                last = w0; down = false;                          // (a left link out of range: as if its subtree were done)
                continue;
            }
            if (cur >= ni) break;                                     // (parent links are internal nodes or INVALID)
            const uint2 lr = *reinterpret_cast<const uint2*>(nodes + cur);
            if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
            last = cur; cur = parent[cur];
        }
        hit_store(hits, i, bt, bu, bv, bp);
    }
}

void launch_intersect(hipStream_t s, int layout, int query, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                      const void* d_rays, uint32_t n_rays, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, void* d_hits,
                      uint32_t* d_overflow, const uint32_t* d_parent) {
    const TriSrc src{ d_tris, (const float*)d_vertices, (const u32*)d_indices, n_vertices };
    const u32 blocks = (n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    const bvh_ray* rays = (const bvh_ray*)d_rays; const bvh2_node* nodes = (const bvh2_node*)d_nodes; const bvh_primref* leaves = (const bvh_primref*)d_leaves;
    bvh_hit* hits = (bvh_hit*)d_hits;
    auto go = [&](auto L, auto Q, auto F) {
        constexpr int LA = decltype(L)::value, QU = decltype(Q)::value, FM = decltype(F)::value;
        { KernelScope ks(s, "k_intersect");
          hipLaunchKernelGGL((k_intersect<LA, QU, FM>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, rays, n_rays, nodes, leaves, src, n, root, hits, d_overflow); }
        { KernelScope ks(s, "k_intersect_deep");
          hipLaunchKernelGGL((k_intersect_deep<LA, QU, FM>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, rays, n_rays, nodes, leaves, src, n, root, hits,
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

void warm_query() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_intersect<0, BVH_QUERY_CLOSEST, BVH_TRI_PADDED64>)); }

} // namespace bvh
