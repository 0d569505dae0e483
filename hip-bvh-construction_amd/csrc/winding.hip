// winding.hip — bvh_winding_prepare / bvh_winding_number on gfx950: the generalized winding number of query points against a built BVH2 in either node layout,
// evaluated hierarchically (Barill et al., "Fast winding numbers for soups and clouds", 2018; no counterpart in the reference): a Barnes–Hut sum in which a far
// subtree contributes one dipole term from its per-node moments and a near one is opened down to the triangles' solid angles.  Nothing in the tree is written.
//   k_winding_climb  : one thread per sorted position j: the leaf's {area vector A, area, first moment M} from its triangle, then bvh_refit's bottom-up walk
//                      (the parent plan of k_refit_plan, second-arriver exchange on the self-cleaning flags words).  The second arriver at a node adds
//                      left + right and writes the seven raw sums into the node's moment record; a leaf sibling's values are recomputed from its triangle, an
//                      internal sibling's are read back with agent-scope loads.  The sums follow the tree, not the arrival order: bit-reproducible.
//   k_winding_finish : one thread per internal node: M -> p = M / area (the box centre when area is 0 or non-finite), r = distance from p to the farthest
//                      corner of the node's stored box.
//   k_winding        : one query per lane, the short stack of k_closest_point in LDS (QUERY_STACK entries, interleaved by lane, no scratch).  Left child first;
//                      a leaf child adds its solid angle, an internal child adds its dipole term iff d2 > (beta * r)^2 and is opened otherwise; of two opened
//                      children the left is entered and the right pushed.  Terms are f32, the sum is one f64 register.  A query whose push would overflow (or
//                      whose walk exceeds the node count: arrays that are not a tree) writes QUERY_MARK's bits into its answer and bumps the overflow word.
//   k_winding_deep   : launched every time, returns at once while the overflow word is 0; otherwise re-walks the marked queries stackless through the parent
//                      links of the plan, left child first.  Correct at any depth.
// An answer that is NaN is stored as the canonical quiet NaN, so that QUERY_MARK's bits (a NaN with another payload) can only be the mark.
// Built without the SLP vectoriser (Makefile).  No record here is replaced under a tie-breaking comparison, so the reason is cost alone: with it the cross and dot
// products became 892 v_pk_* instructions over the file's kernels (two scalar operations' worth each on gfx950) plus 660 register moves to pair their operands.
// Compiled without -fno-honor-nans: the opening test and the area test must be false on NaN.
#include <type_traits>
#include "winding.hpp"
#include "kernels.hpp"

namespace bvh {

// (the sums, the leaf values, the solid angle, the dipole term, the point load and the answer store are winding.hpp's, shared with scene_winding.hip)

template <int LAYOUT, int FMT>
__global__ __launch_bounds__(WIND_BLOCK) void k_winding_climb(const bvh2_node* __restrict__ nodes, const bvh_primref* __restrict__ leaves, TriSrc src,
                                                              const u32* __restrict__ parent, u32* flags, bvh_winding_moment* mom, u32 n) {
    const u32 j = bid_x() * WIND_BLOCK + tid_x();
    if (j >= n) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    u32 cur = ni + j;
    WSum s = wsum_leaf<FMT>(src, leaf_prim<LAYOUT>(nodes, leaves, cur, ni), n);
    u32 p = parent[cur];
    while (p < ni) {
        drain_stores();
        const u32 sib = __hip_atomic_exchange(flags + p, cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (sib == INV) break;
        st_agent(flags + p, INV);
        compiler_fence();
        WSum o = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
        if (sib < ni) o = wsum_load_agent(mom + sib);                                  // written in this launch by the sibling's second arriver
        else if (sib < total) o = wsum_leaf<FMT>(src, leaf_prim<LAYOUT>(nodes, leaves, sib, ni), n);
        s = nodes[p].left == cur ? wsum_add(s, o) : wsum_add(o, s);                    // left + right, whoever arrives second
        wsum_store_agent(mom + p, s);
        cur = p; p = parent[p];
    }
}

__global__ __launch_bounds__(WIND_BLOCK) void k_winding_finish(const bvh2_node* __restrict__ nodes, bvh_winding_moment* mom, u32 ni) {
    const u32 i = bid_x() * WIND_BLOCK + tid_x();
    if (i >= ni) return;
    const float4* q = reinterpret_cast<const float4*>(nodes + i);
    const float4 q0 = q[0], q1 = q[1];
    wind_finish(mom + i, Box{ q0.z, q0.w, q1.x, q1.y, q1.z, q1.w });
}

// ---- the query ------------------------------------------------------------------------------------------------------------------------------------------------
// the Van Oosterom–Strackee solid angle of primitive prim seen from q, over 4 pi
template <int FMT>
__device__ __forceinline__ float wind_leaf_term(const TriSrc& src, u32 prim, u32 n, QF3 q) {
    if (prim >= n) return 0.0f;                                   // (never in a tree: skipped)
    QF3 a, b, c; tri_fetch<FMT>(src, prim, a, b, c);
    return wind_solid_angle(a, b, c, q);
}
// one child of an opened node: adds its term and returns false, or returns true when it has to be opened (links out of range are skipped)
template <int LAYOUT, int FMT>
__device__ __forceinline__ bool wind_child(const bvh2_node* __restrict__ nodes, const bvh_primref* __restrict__ leaves, const TriSrc& src,
                                           const bvh_winding_moment* __restrict__ mom, u32 c, u32 n, QF3 q, float beta, double& acc) {
    const u32 ni = n - 1, total = 2 * n - 1;
    if (c >= total) return false;
    if (c >= ni) { acc += (double)wind_leaf_term<FMT>(src, leaf_prim<LAYOUT>(nodes, leaves, c, ni), n, q); return false; }
    float term;
    if (!wind_far(mom, c, q, beta, term)) return true;
    acc += (double)term;
    return false;
}

template <int LAYOUT, int FMT>
__global__ __launch_bounds__(QUERY_BLOCK) void k_winding(const bvh_point_query* __restrict__ pts, u32 n_points, const bvh2_node* __restrict__ nodes,
                                                         const bvh_primref* __restrict__ leaves, TriSrc src, const bvh_winding_moment* __restrict__ mom,
                                                         u32 n, u32 root, float beta, float* __restrict__ w, u32* __restrict__ overflow) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= n_points) return;
    u32* const stack = s_stack + tid_x();
    QF3 q;
    if (!wind_point_load(pts, i, q)) { reinterpret_cast<u32*>(w)[i] = WIND_NAN; return; }
    double acc = 0.0;
    bool deep = false;
    u32 nl, nr; { const uint2 lr = *reinterpret_cast<const uint2*>(nodes + root); nl = lr.x; nr = lr.y; }
    u32 top = 0, steps = 0;
    for (;;) {
        if (++steps > n) { deep = true; break; }                  // more expansions than internal nodes: not a tree (a tree never gets here)
        const bool oa = wind_child<LAYOUT, FMT>(nodes, leaves, src, mom, nl, n, q, beta, acc);
        const bool ob = wind_child<LAYOUT, FMT>(nodes, leaves, src, mom, nr, n, q, beta, acc);
        u32 next;
        if (oa && ob) {
            if (top == (u32)QUERY_STACK) { deep = true; break; }
            stack[top * QUERY_BLOCK] = nr; ++top;
            next = nl;
        } else if (oa) next = nl;
        else if (ob) next = nr;
        else {
            if (top == 0) break;
            next = stack[--top * QUERY_BLOCK];
        }
        const uint2 lr = *reinterpret_cast<const uint2*>(nodes + next);
        nl = lr.x; nr = lr.y;
    }
    if (deep) { reinterpret_cast<u32*>(w)[i] = QUERY_MARK; atomicAdd(overflow, 1u); }
    else wind_store(w, i, acc);
}

// the stackless re-walk of the marked queries: parent links of the plan, left child first; a node entered from above is approximated or opened there
template <int LAYOUT, int FMT>
__global__ __launch_bounds__(QUERY_BLOCK) void k_winding_deep(const bvh_point_query* __restrict__ pts, u32 n_points, const bvh2_node* __restrict__ nodes,
                                                              const bvh_primref* __restrict__ leaves, TriSrc src, const bvh_winding_moment* __restrict__ mom,
                                                              u32 n, u32 root, float beta, float* w, const u32* __restrict__ overflow,
                                                              const u32* __restrict__ parent) {
    if (*overflow == 0u) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < n_points; i += nbid_x() * QUERY_BLOCK) {
        if (reinterpret_cast<const u32*>(w)[i] != QUERY_MARK) continue;
        QF3 q;
        wind_point_load(pts, i, q);                               // (a marked query has no NaN coordinate)
        double acc = 0.0;
        u32 cur = root, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < total && steps < bound; ++steps) {
            if (down) {
                if (cur >= ni) {
                    acc += (double)wind_leaf_term<FMT>(src, leaf_prim<LAYOUT>(nodes, leaves, cur, ni), n, q);
                    last = cur; cur = parent[cur]; down = false;
                    continue;
                }
                float term;
                if (cur != root && wind_far(mom, cur, q, beta, term)) { acc += (double)term; last = cur; cur = parent[cur]; down = false; continue; }
                const u32 l = nodes[cur].left;
                if (l < total) { cur = l; continue; }
                last = l; down = false;                           // (a left link out of range: as if its subtree were done)
                continue;
            }
            if (cur >= ni) break;                                 // (parent links are internal nodes or INVALID)
            const uint2 lr = *reinterpret_cast<const uint2*>(nodes + cur);
            if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
            last = cur; cur = parent[cur];
        }
        wind_store(w, i, acc);
    }
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------------------------------------
template <typename Go>
static void wind_dispatch(int layout, int tri_format, Go go) {
    using L0 = std::integral_constant<int, 0>; using L1 = std::integral_constant<int, 1>;
    auto by_fmt = [&](auto L) {
        switch (tri_format) {
            case BVH_TRI_PADDED64: go(L, std::integral_constant<int, BVH_TRI_PADDED64>{}); break;
            case BVH_TRI_PACKED36: go(L, std::integral_constant<int, BVH_TRI_PACKED36>{}); break;
            default:               go(L, std::integral_constant<int, BVH_TRI_INDEXED>{}); break;
        }
    };
    if (layout == 0) by_fmt(L0{}); else by_fmt(L1{});
}

void launch_winding_prepare(hipStream_t s, int layout, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                            const void* d_nodes, const void* d_leaves, uint32_t n, const uint32_t* d_parent, uint32_t* d_flags, void* d_moments) {
    const TriSrc src{ d_tris, (const float*)d_vertices, (const u32*)d_indices, n_vertices };
    const bvh2_node* nodes = (const bvh2_node*)d_nodes; const bvh_primref* leaves = (const bvh_primref*)d_leaves;
    bvh_winding_moment* mom = (bvh_winding_moment*)d_moments;
    wind_dispatch(layout, tri_format, [&](auto L, auto F) {
        constexpr int LA = decltype(L)::value, FM = decltype(F)::value;
        KernelScope ks(s, "k_winding_climb");
        hipLaunchKernelGGL((k_winding_climb<LA, FM>), dim3((n + WIND_BLOCK - 1) / WIND_BLOCK), dim3(WIND_BLOCK), 0, s, nodes, leaves, src, d_parent, d_flags, mom, n);
    });
    KernelScope ks(s, "k_winding_finish");
    hipLaunchKernelGGL(k_winding_finish, dim3((n - 1 + WIND_BLOCK - 1) / WIND_BLOCK), dim3(WIND_BLOCK), 0, s, nodes, mom, n - 1);
}

void launch_winding(hipStream_t s, int layout, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                    const void* d_points, uint32_t n_points, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, const void* d_moments,
                    float beta, float* d_w, uint32_t* d_overflow, const uint32_t* d_parent) {
    const TriSrc src{ d_tris, (const float*)d_vertices, (const u32*)d_indices, n_vertices };
    const u32 blocks = (n_points + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    const bvh_point_query* pts = (const bvh_point_query*)d_points; const bvh2_node* nodes = (const bvh2_node*)d_nodes;
    const bvh_primref* leaves = (const bvh_primref*)d_leaves; const bvh_winding_moment* mom = (const bvh_winding_moment*)d_moments;
    wind_dispatch(layout, tri_format, [&](auto L, auto F) {
        constexpr int LA = decltype(L)::value, FM = decltype(F)::value;
        { KernelScope ks(s, "k_winding");
          hipLaunchKernelGGL((k_winding<LA, FM>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, pts, n_points, nodes, leaves, src, mom, n, root, beta, d_w, d_overflow); }
        { KernelScope ks(s, "k_winding_deep");
          hipLaunchKernelGGL((k_winding_deep<LA, FM>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, pts, n_points, nodes, leaves, src, mom, n, root, beta, d_w,
                             (const u32*)d_overflow, d_parent); }
    });
}

void warm_winding() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_winding<0, BVH_TRI_PADDED64>)); }

} // namespace bvh
