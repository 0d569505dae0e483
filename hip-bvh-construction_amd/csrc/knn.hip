// knn.hip — bvh_knn on gfx950: the k nearest triangles of each query point within its radius, against a built BVH2 in either node layout (no counterpart in the
// reference).  One query per lane, templated on node layout, triangle format and a k bucket (8 / 16 / 32: the list's LDS); the traversal is point_query.hip's,
// culled against the list's last entry once the list is full (r2 before that).
//   k_knn      : near-child-first traversal with the short per-lane stack in LDS (QUERY_STACK entries), as k_closest_point.  A query whose push would overflow
//                (or whose walk exceeds the node count: arrays that are not a tree) gets QUERY_MARK in the prim_idx of its first record and bumps the overflow
//                word.
//   k_knn_deep : launched every time, returns at once while the overflow word is 0; otherwise re-walks the marked queries stackless through the parent links of
//                bvh_refit's plan (k_refit_plan), left child first.  Correct at any depth.
// The candidate list never lives in a per-lane array (dynamic indexing would send it to scratch): it is a column of LDS, entry j of lane l at
// s_list[j * QUERY_BLOCK + l], each entry one u64 key (float_as_uint(dist2) << 32) | prim.  An accepted dist2 is a sum of squares, never negative and never
// NaN, so the u64 order is the contract's lexicographic (dist2, prim) order and an insertion is compare-and-shift on one word from the tail.  The lane keeps
// the list's length, its last key and that key's dist2 (the culling bound) in registers: with k == 1 an accepted candidate costs one LDS store and no load.
// Write-out of k_knn: the wave's 64 * k records leave LDS with consecutive lanes writing consecutive 8-byte records (KNN_COOP_STORE; false keeps the
// lane-per-query stores of stride 8k bytes that k_knn_deep uses).  DESIGN.md §8g has the measurements.
// Built without the SLP vectoriser (Makefile), as point_query.o: the list update is the same tie-breaking pattern.
#include <type_traits>
#include "query.hpp"
#include "kernels.hpp"

namespace bvh {

constexpr bool KNN_COOP_STORE = true;          // k_knn's write-out: the wave stores its 64 * k records from LDS in record order

static_assert(KNN_MAX_K == BVH_KNN_MAX_K, "the largest bucket holds BVH_KNN_MAX_K entries");

// one lane's list: col = its LDS column (stride QUERY_BLOCK), cnt entries of k, last = the key at place k-1 once cnt == k, bound = the culling / acceptance
// bound: last's dist2 once the list is full, r2 before
struct KList { u64* col; u32 k, cnt; u64 last; float bound; };

__device__ __forceinline__ u64 knn_key(float d2, u32 prim) { return ((u64)__float_as_uint(d2) << 32) | prim; }

__device__ __forceinline__ void knn_insert(KList& L, float d2, u32 prim) {
    if (!(d2 <= L.bound)) return;                                 // acceptance d2 <= r2 (NaN fails), and nothing above a full list's last entry
    const u64 key = knn_key(d2, prim);
    const bool full = L.cnt == L.k;
    if (full && !(key < L.last)) return;                          // equal dist2: only a smaller prim enters
    u32 j = full ? L.k - 1 : L.cnt;
    const u32 tail = j;
    while (j > 0) {
        const u64 prev = L.col[(j - 1) * QUERY_BLOCK];
        if (prev < key) break;
        L.col[j * QUERY_BLOCK] = prev; --j;
    }
    L.col[j * QUERY_BLOCK] = key;
    if (!full) ++L.cnt;
    if (L.cnt == L.k) {
        L.last = (j == tail) ? key : L.col[(L.k - 1) * QUERY_BLOCK];
        L.bound = __uint_as_float((u32)(L.last >> 32));
    }
}

template <int FMT>
__device__ __forceinline__ void leaf_knn(const TriSrc& src, u32 prim, u32 n, QF3 p, KList& L) {
    if (prim >= n) return;                                        // (never in a tree: not followed)
    QF3 a, b, c; tri_fetch<FMT>(src, prim, a, b, c);
    QF3 q; float u, v;
    knn_insert(L, tri_closest(a, b, c, p, q, u, v), prim);
}

__device__ __forceinline__ void knn_store(bvh_knn_hit* h, u64 key) { h->dist2 = __uint_as_float((u32)(key >> 32)); h->prim_idx = (u32)key; }

template <int LAYOUT, int FMT, int KB>
__global__ __launch_bounds__(QUERY_BLOCK) void k_knn(const bvh_point_query* __restrict__ pts, u32 n_points, const bvh2_node* __restrict__ nodes,
                                                     const bvh_primref* __restrict__ leaves, TriSrc src, u32 n, u32 root, u32 k,
                                                     bvh_knn_hit* __restrict__ hits, u32* __restrict__ counts, u32* __restrict__ overflow) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    __shared__ u64 s_list[KB * QUERY_BLOCK];
    const u32 base = bid_x() * QUERY_BLOCK, i = base + tid_x();
    u32* const stack = s_stack + tid_x();
    const bool in = i < n_points;
    QF3 p{ 0.0f, 0.0f, 0.0f }; float r2 = 0.0f;
    const bool live = in && point_load(pts, i, p, r2);
    KList L{ s_list + tid_x(), k, 0u, 0ull, r2 };
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
            if (nl < total) { rec_fetch<LAYOUT>(nodes, leaves, nl, ni, a0, a1, ba); ha = box_dist_pass(ba, p, L.bound, la); }
            if (nr < total) { rec_fetch<LAYOUT>(nodes, leaves, nr, ni, b0, b1, bb); hb = box_dist_pass(bb, p, L.bound, lb); }
            if (ha && nl >= ni) { leaf_knn<FMT>(src, a0, n, p, L); ha = false; }
            if (hb && nr >= ni) { leaf_knn<FMT>(src, b0, n, p, L); hb = false; }
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
    // the wave has reconverged: unused slots become {r2, INVALID}; a query left to k_knn_deep carries QUERY_MARK in its first record
    const u64 pad = knn_key(r2, INV);
    if (deep) { L.cnt = 0; atomicAdd(overflow, 1u); }
    if (in) {
        for (u32 j = L.cnt; j < k; ++j) L.col[j * QUERY_BLOCK] = pad;
        if (deep) L.col[0] = knn_key(r2, QUERY_MARK);
        if (counts) counts[i] = L.cnt;
    }
    if constexpr (KNN_COOP_STORE) {
        __syncthreads();                                          // (one wave per workgroup: orders the LDS columns before other lanes read them)
        const u32 nq = n_points - base < (u32)QUERY_BLOCK ? n_points - base : (u32)QUERY_BLOCK;
        bvh_knn_hit* const out = hits + (size_t)base * k;
        // record t of the wave's nq * k is query t / k, entry t % k; lane l takes t = l, l + 64, ...: (q, j) advance by (64 / k, 64 % k) with a carry
        const u32 dq = (u32)QUERY_BLOCK / k, dj = (u32)QUERY_BLOCK % k;
        u32 q = tid_x() / k, j = tid_x() % k;
        for (u32 t = tid_x(); t < nq * k; t += QUERY_BLOCK) {
            knn_store(out + t, s_list[j * QUERY_BLOCK + q]);
            q += dq; j += dj;
            if (j >= k) { j -= k; ++q; }
        }
    } else if (in) {
        for (u32 j = 0; j < k; ++j) knn_store(hits + (size_t)i * k + j, L.col[j * QUERY_BLOCK]);
    }
}

// the stackless re-walk of the marked queries: parent links of the plan, left child first
template <int LAYOUT, int FMT, int KB>
__global__ __launch_bounds__(QUERY_BLOCK) void k_knn_deep(const bvh_point_query* __restrict__ pts, u32 n_points, const bvh2_node* __restrict__ nodes,
                                                          const bvh_primref* __restrict__ leaves, TriSrc src, u32 n, u32 root, u32 k,
                                                          bvh_knn_hit* __restrict__ hits, u32* __restrict__ counts, const u32* __restrict__ overflow,
                                                          const u32* __restrict__ parent) {
    __shared__ u64 s_list[KB * QUERY_BLOCK];
    if (*overflow == 0u) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < n_points; i += nbid_x() * QUERY_BLOCK) {
        bvh_knn_hit* const mine = hits + (size_t)i * k;
        if (mine->prim_idx != QUERY_MARK) continue;
        QF3 p; float r2;
        point_load(pts, i, p, r2);                                // (a marked query passed the checks)
        KList L{ s_list + tid_x(), k, 0u, 0ull, r2 };
        u32 cur = root, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < total && steps < bound; ++steps) {
            u32 w0, w1; Box b;
            if (down) {
                if (cur >= ni) {
                    rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                    float lb;
                    if (box_dist_pass(b, p, L.bound, lb)) leaf_knn<FMT>(src, w0, n, p, L);
                    last = cur; cur = parent[cur]; down = false;
                    continue;
                }
                rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                float lb;
                if (!box_dist_pass(b, p, L.bound, lb)) { last = cur; cur = parent[cur]; down = false; continue; }
                if (w0 < total) { cur = w0; continue; }
                last = w0; down = false;                          // (a left link out of range: as if its subtree were done)
                continue;
            }
            if (cur >= ni) break;                                 // (parent links are internal nodes or INVALID)
            const uint2 lr = *reinterpret_cast<const uint2*>(nodes + cur);
            if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
            last = cur; cur = parent[cur];
        }
        const u64 pad = knn_key(r2, INV);
        for (u32 j = 0; j < k; ++j) knn_store(mine + j, j < L.cnt ? L.col[j * QUERY_BLOCK] : pad);
        if (counts) counts[i] = L.cnt;
    }
}

void launch_knn(hipStream_t s, int layout, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                const void* d_points, uint32_t n_points, uint32_t k, const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, void* d_hits,
                uint32_t* d_counts, uint32_t* d_overflow, const uint32_t* d_parent) {
    const TriSrc src{ d_tris, (const float*)d_vertices, (const u32*)d_indices, n_vertices };
    const u32 blocks = (n_points + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    const bvh_point_query* pts = (const bvh_point_query*)d_points; const bvh2_node* nodes = (const bvh2_node*)d_nodes;
    const bvh_primref* leaves = (const bvh_primref*)d_leaves;
    bvh_knn_hit* hits = (bvh_knn_hit*)d_hits;
    auto go = [&](auto L, auto F, auto K) {
        constexpr int LA = decltype(L)::value, FM = decltype(F)::value, KB = decltype(K)::value;
        { KernelScope ks(s, "k_knn");
          hipLaunchKernelGGL((k_knn<LA, FM, KB>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, pts, n_points, nodes, leaves, src, n, root, k, hits, d_counts, d_overflow); }
        { KernelScope ks(s, "k_knn_deep");
          hipLaunchKernelGGL((k_knn_deep<LA, FM, KB>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, pts, n_points, nodes, leaves, src, n, root, k, hits, d_counts,
                             (const u32*)d_overflow, d_parent); }
    };
    auto by_k = [&](auto L, auto F) {                             // the bucket sizes the list's LDS: 4 / 8 / 16 KiB per wave beside the 16 KiB stack
        if (k <= 8u) go(L, F, std::integral_constant<int, 8>{});
        else if (k <= 16u) go(L, F, std::integral_constant<int, 16>{});
        else go(L, F, std::integral_constant<int, KNN_MAX_K>{});
    };
    auto by_fmt = [&](auto L) {
        switch (tri_format) {
            case BVH_TRI_PADDED64: by_k(L, std::integral_constant<int, BVH_TRI_PADDED64>{}); break;
            case BVH_TRI_PACKED36: by_k(L, std::integral_constant<int, BVH_TRI_PACKED36>{}); break;
            default:               by_k(L, std::integral_constant<int, BVH_TRI_INDEXED>{}); break;
        }
    };
    if (layout == 0) by_fmt(std::integral_constant<int, 0>{}); else by_fmt(std::integral_constant<int, 1>{});
}

void warm_knn() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_knn<0, BVH_TRI_PADDED64, 8>));
}

} // namespace bvh
