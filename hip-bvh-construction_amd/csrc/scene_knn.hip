// scene_knn.hip — bvh_scene_knn on gfx950: the k nearest triangles of each query point within its radius, over all active instances of a scene (no counterpart
// in the reference).  One query per lane.  It is scene_point.hip's walk with knn.hip's list: the candidate of (instance k, primitive j) is tri_closest on the
// WORLD triangle (the BLAS's vertices mapped by the instance's forward matrix), the walk inside an instance runs in object space against the mapped point
// p' = W_k p with the box grown by QUERY_GROW * (its largest |coordinate|) + e and culled iff s2 * lb' * (1 - 2^-20) > bound (scene_query.hpp), and bound is the
// dist2 of the list's last entry once the list holds k entries (r2 before that), carried across instances and level changes.
//   k_scene_knn      : one per-lane LDS short stack shared by both levels (k_scene_closest_point's structure and walk order: near child first by lower bound
//                      at both levels, la <= lb goes left), leaf children whose box passes tested at once, the forward matrix re-loaded per leaf test.  With
//                      k == 1 the walk tests the same boxes against the same bound as k_scene_closest_point<CLOSEST> and keeps the same candidate.
//   k_scene_knn_deep : launched every time, returns at once while the overflow word is 0; otherwise re-walks the marked queries (QUERY_MARK in the prim_idx of
//                      their first record) stackless: the top-level plan, and for every instance whose world box passes, that BLAS's plan.
// A record is ordered by (dist2, instance, prim): 96 bits, so the list is two LDS columns interleaved by lane, entry j of lane l at [j * QUERY_BLOCK + l]: a u64
// key (float_as_uint(dist2) << 32) | instance and a u32 prim.  An accepted dist2 is a sum of squares, never negative and never NaN, so comparing the u64 first
// and the prim on a tie is the contract's lexicographic order.  The lane keeps the list's length, its last entry and that entry's dist2 (the bound) in
// registers: with k == 1 an accepted candidate costs two LDS stores and no load.  The list never lives in a per-lane array (scratch).
// Write-out of k_scene_knn: the wave's 64 * k records leave LDS in record order, consecutive lanes writing consecutive 16-byte records, one store each;
// k_scene_knn_deep keeps lane-per-query stores.
// Built without the SLP vectoriser (Makefile), as scene_point.o and knn.o: the list update is the same tie-breaking pattern.
#include <type_traits>
#include "scene_query.hpp"

namespace bvh {

static_assert(KNN_MAX_K == BVH_KNN_MAX_K, "the largest bucket holds BVH_KNN_MAX_K entries");
static_assert(sizeof(bvh_instance_knn_hit) == sizeof(uint4), "a record leaves in one 16-byte store");

// one lane's list: kcol / pcol = its LDS columns (stride QUERY_BLOCK), cnt entries of k, (last, lastp) = the entry at place k-1 once cnt == k, bound = the
// culling / acceptance bound: last's dist2 once the list is full, r2 before
struct SKList { u64* kcol; u32* pcol; u32 k, cnt; u64 last; u32 lastp; float bound; };

__device__ __forceinline__ u64 sknn_key(float d2, u32 inst) { return ((u64)__float_as_uint(d2) << 32) | inst; }

__device__ __forceinline__ void sknn_insert(SKList& L, float d2, u32 inst, u32 prim) {
    if (!(d2 <= L.bound)) return;                                 // acceptance d2 <= r2 (NaN fails), and nothing above a full list's last entry
    const u64 key = sknn_key(d2, inst);
    const bool full = L.cnt == L.k;
    if (full && !(key < L.last || (key == L.last && prim < L.lastp))) return;   // equal dist2: only a smaller (instance, prim) enters
    u32 j = full ? L.k - 1 : L.cnt;
    const u32 tail = j;
    while (j > 0) {
        const u64 pk = L.kcol[(j - 1) * QUERY_BLOCK];
        const u32 pp = L.pcol[(j - 1) * QUERY_BLOCK];
        if (pk < key || (pk == key && pp < prim)) break;
        L.kcol[j * QUERY_BLOCK] = pk; L.pcol[j * QUERY_BLOCK] = pp; --j;
    }
    L.kcol[j * QUERY_BLOCK] = key; L.pcol[j * QUERY_BLOCK] = prim;
    if (!full) ++L.cnt;
    if (L.cnt == L.k) {
        const bool mine = j == tail;
        L.last = mine ? key : L.kcol[(L.k - 1) * QUERY_BLOCK];
        L.lastp = mine ? prim : L.pcol[(L.k - 1) * QUERY_BLOCK];
        L.bound = __uint_as_float((u32)(L.last >> 32));
    }
}

// the candidate of (inst, prim): the world triangle's squared distance to the world point w, offered to the list.  The world triangle is blas_world_tri's
// (scene_query.hpp) written out: through the shared helper the same operations were scheduled differently and k_scene_knn<32> measured 0.5 % slower on the
// 64-instance scene (19.62 -> 19.73 ms per 2^20 points, four interleaved runs each, spread of either 0.4 %), so this leaf keeps the text it was measured with
__device__ __forceinline__ void sknn_leaf(const SceneQuery& a, const SceneBlas& B, u32 prim, u32 inst, QF3 w, SKList& L) {
    if (prim >= B.n) return;
    const TriSrc src{ B.tris, reinterpret_cast<const float*>(B.tris), reinterpret_cast<const u32*>(B.idx), B.nv };
    QF3 v1, v2, v3;
    if (B.fmt == BVH_TRI_PADDED64) tri_fetch<BVH_TRI_PADDED64>(src, prim, v1, v2, v3);
    else if (B.fmt == BVH_TRI_PACKED36) tri_fetch<BVH_TRI_PACKED36>(src, prim, v1, v2, v3);
    else tri_fetch<BVH_TRI_INDEXED>(src, prim, v1, v2, v3);
    const float4* mq = reinterpret_cast<const float4*>(reinterpret_cast<const bvh_instance*>(a.inst_in) + inst);
    const float4 m0 = mq[0], m1 = mq[1], m2 = mq[2];
    const float m[12] = { m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w };
    const QF3 wa = xf_point(m, v1.x, v1.y, v1.z), wb = xf_point(m, v2.x, v2.y, v2.z), wc = xf_point(m, v3.x, v3.y, v3.z);
    QF3 q; float u, v;
    sknn_insert(L, tri_closest(wa, wb, wc, w, q, u, v), inst, prim);
}

// one 16-byte record {dist2, prim_idx, instance_idx, 0}
__device__ __forceinline__ void sknn_store(bvh_instance_knn_hit* h, u64 key, u32 prim) {
    *reinterpret_cast<uint4*>(h) = make_uint4((u32)(key >> 32), prim, (u32)key, 0u);
}

template <int KB>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_knn(SceneQuery a) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    __shared__ u64 s_key[KB * QUERY_BLOCK];
    __shared__ u32 s_prim[KB * QUERY_BLOCK];
    const u32 base = bid_x() * QUERY_BLOCK, i = base + tid_x();
    const u32 k = a.k;
    u32* const stack = s_stack + tid_x();
    const bool in = i < a.n_rays;
    QF3 w{ 0.0f, 0.0f, 0.0f }; float r2 = 0.0f;
    const bool live = in && point_load(reinterpret_cast<const bvh_point_query*>(a.rays), i, w, r2);
    SKList L{ s_key + tid_x(), s_prim + tid_x(), k, 0u, 0ull, INV, r2 };
    bool deep = false;
    if (live) {
        const ScenePoint world{ w, 0.0f, 1.0f };
        ScenePoint c = world;
        SceneBlas B{};
        const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
        u32 ni = tni, total = ttotal;                                 // of the level the query is on
        bool in_blas = false, pop = false, entering = false;         // entering: instance `enter` is entered at the top of the next step
        u32 inst = INV, enter = INV;
        u32 nl = INV, nr = INV, top = 0, tsteps = 0, bsteps = 0;
        if (a.n_inst == 1) {                                          // no top-level tree: the instance's world box, then the instance
            float lb;
            if (scene_box_dist_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), world, L.bound, lb)) { enter = 0; entering = true; } else pop = true;
        } else {
            const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(a.tnodes) + a.troot); nl = lr.x; nr = lr.y;
        }
        for (;;) {
            if (entering) {
                entering = false;
                const u32 e = enter;
                if (e < a.n_inst && enter_instance_point(a, e, w, c, B)) {
                    in_blas = true; inst = e; ni = B.n - 1; total = 2 * B.n - 1; bsteps = 0;
                    const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(B.nodes) + B.root); nl = lr.x; nr = lr.y;
                } else pop = true;
            }
            if (!pop) {
                if (in_blas ? ++bsteps > B.n : ++tsteps > ttotal) { deep = true; break; }   // (a tree never gets here)
                const int layout = in_blas ? (int)B.layout : (int)a.tlayout;
                const void* nodes = in_blas ? B.nodes : a.tnodes; const void* leaves = in_blas ? B.leaves : a.tleaves;
                u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
                Box ba, bb;
                float la = 0.0f, lb = 0.0f;
                bool ha = false, hb = false;
                if (nl < total) { rec_fetch_rt(layout, nodes, leaves, nl, ni, a0, a1, ba); ha = scene_box_dist_pass(ba, c, L.bound, la); }
                if (nr < total) { rec_fetch_rt(layout, nodes, leaves, nr, ni, b0, b1, bb); hb = scene_box_dist_pass(bb, c, L.bound, lb); }
                if (in_blas) {                                        // triangles at once; at the top level a leaf is an instance, entered like a node
                    if (ha && nl >= ni) { sknn_leaf(a, B, a0, inst, w, L); ha = false; }
                    if (hb && nr >= ni) { sknn_leaf(a, B, b0, inst, w, L); hb = false; }
                }
                u32 n = INV, c0 = INV, c1 = INV;
                if (ha && hb) {
                    const bool left_first = la <= lb;
                    if (top == (u32)QUERY_STACK) { deep = true; break; }
                    stack[top * QUERY_BLOCK] = (left_first ? nr : nl) | (in_blas ? SCENE_BLAS_ENTRY : 0u); ++top;
                    n = left_first ? nl : nr; c0 = left_first ? a0 : b0; c1 = left_first ? a1 : b1;
                } else if (ha) { n = nl; c0 = a0; c1 = a1; }
                else if (hb) { n = nr; c0 = b0; c1 = b1; }
                if (n == INV) pop = true;
                else if (in_blas || n < tni) { nl = c0; nr = c1; }
                else { enter = c0; entering = true; }                 // a top-level leaf: its instance
            }
            if (pop) {
                pop = false;
                if (top == 0) break;
                const u32 e = stack[--top * QUERY_BLOCK];
                if (e & SCENE_BLAS_ENTRY) {
                    const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(B.nodes) + (e & ~SCENE_BLAS_ENTRY)); nl = lr.x; nr = lr.y;
                } else {
                    if (in_blas) { c = world; in_blas = false; ni = tni; total = ttotal; }   // back to the top level: the world point
                    u32 w0, w1; Box b;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, e, tni, w0, w1, b);
                    if (e < tni) { nl = w0; nr = w1; } else { enter = w0; entering = true; }
                }
            }
        }
    }
    // the wave has reconverged: unused slots become {r2, INVALID, INVALID}; a query left to k_scene_knn_deep carries QUERY_MARK in its first record
    const u64 pad = sknn_key(r2, INV);
    if (deep) { L.cnt = 0; atomicAdd(a.overflow, 1u); }
    if (in) {
        for (u32 j = L.cnt; j < k; ++j) { L.kcol[j * QUERY_BLOCK] = pad; L.pcol[j * QUERY_BLOCK] = INV; }
        if (deep) L.pcol[0] = QUERY_MARK;
        if (a.counts) a.counts[i] = L.cnt;
    }
    __syncthreads();                                              // (one wave per workgroup: orders the LDS columns before other lanes read them)
    const u32 nq = a.n_rays - base < (u32)QUERY_BLOCK ? a.n_rays - base : (u32)QUERY_BLOCK;
    bvh_instance_knn_hit* const out = reinterpret_cast<bvh_instance_knn_hit*>(a.hits) + (size_t)base * k;
    // record t of the wave's nq * k is query t / k, entry t % k; lane l takes t = l, l + 64, ...: (q, j) advance by (64 / k, 64 % k) with a carry
    const u32 dq = (u32)QUERY_BLOCK / k, dj = (u32)QUERY_BLOCK % k;
    u32 q = tid_x() / k, j = tid_x() % k;
    for (u32 t = tid_x(); t < nq * k; t += QUERY_BLOCK) {
        sknn_store(out + t, s_key[j * QUERY_BLOCK + q], s_prim[j * QUERY_BLOCK + q]);
        q += dq; j += dj;
        if (j >= k) { j -= k; ++q; }
    }
}

// stackless walk of instance k's BLAS (k_scene_closest_point_deep's walk through the BLAS's plan)
__device__ void sknn_walk_blas(const SceneQuery& a, u32 k, QF3 w, SKList& L) {
    ScenePoint c; SceneBlas B;
    if (k >= a.n_inst || !enter_instance_point(a, k, w, c, B)) return;
    const u32 ni = B.n - 1, total = 2 * B.n - 1;
    const u64 bound = 3ull * total + 3ull;
    u32 cur = B.root, last = INV;
    bool down = true;
    for (u64 steps = 0; cur < total && steps < bound; ++steps) {
        u32 w0, w1; Box b;
        if (down) {
            rec_fetch_rt((int)B.layout, B.nodes, B.leaves, cur, ni, w0, w1, b);
            float lb;
            const bool pass = scene_box_dist_pass(b, c, L.bound, lb);
            if (cur >= ni) {
                if (pass) sknn_leaf(a, B, w0, k, w, L);
                last = cur; cur = B.parent[cur]; down = false;
                continue;
            }
            if (!pass) { last = cur; cur = B.parent[cur]; down = false; continue; }
            if (w0 < total) { cur = w0; continue; }
            last = w0; down = false;
            continue;
        }
        if (cur >= ni) break;
        const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(B.nodes) + cur);
        if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
        last = cur; cur = B.parent[cur];
    }
}

template <int KB>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_knn_deep(SceneQuery a) {
    __shared__ u64 s_key[KB * QUERY_BLOCK];
    __shared__ u32 s_prim[KB * QUERY_BLOCK];
    if (*a.overflow == 0u) return;
    const u32 k = a.k;
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 bound = 3ull * ttotal + 3ull;
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < a.n_rays; i += nbid_x() * QUERY_BLOCK) {
        bvh_instance_knn_hit* const mine = reinterpret_cast<bvh_instance_knn_hit*>(a.hits) + (size_t)i * k;
        if (mine->prim_idx != QUERY_MARK) continue;
        QF3 w; float r2;
        point_load(reinterpret_cast<const bvh_point_query*>(a.rays), i, w, r2);   // (a marked query passed the checks)
        const ScenePoint world{ w, 0.0f, 1.0f };
        SKList L{ s_key + tid_x(), s_prim + tid_x(), k, 0u, 0ull, INV, r2 };
        if (a.n_inst == 1) {
            float lb;
            if (scene_box_dist_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), world, L.bound, lb)) sknn_walk_blas(a, 0, w, L);
        } else {
            u32 cur = a.troot, last = INV;
            bool down = true;
            for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
                u32 w0, w1; Box b;
                if (down) {
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, cur, tni, w0, w1, b);
                    float lb;
                    if (!scene_box_dist_pass(b, world, L.bound, lb)) { last = cur; cur = a.tparent[cur]; down = false; continue; }
                    if (cur >= tni) {                                 // an instance whose world box passes
                        sknn_walk_blas(a, w0, w, L);
                        last = cur; cur = a.tparent[cur]; down = false;
                        continue;
                    }
                    if (w0 < ttotal) { cur = w0; continue; }
                    last = w0; down = false;
                    continue;
                }
                if (cur >= tni) break;
                const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(a.tnodes) + cur);
                if (last == lr.x && lr.y < ttotal && lr.y != lr.x) { cur = lr.y; down = true; continue; }
                last = cur; cur = a.tparent[cur];
            }
        }
        const u64 pad = sknn_key(r2, INV);
        for (u32 j = 0; j < k; ++j) {
            const bool have = j < L.cnt;
            sknn_store(mine + j, have ? L.kcol[j * QUERY_BLOCK] : pad, have ? L.pcol[j * QUERY_BLOCK] : INV);
        }
        if (a.counts) a.counts[i] = L.cnt;
    }
}

void launch_scene_knn(hipStream_t s, const SceneQuery& q) {
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    auto go = [&](auto K) {                                       // the bucket sizes the list's LDS: 6 / 12 / 24 KiB per wave beside the 16 KiB stack
        constexpr int KB = decltype(K)::value;
        { KernelScope ks(s, "k_scene_knn"); hipLaunchKernelGGL(k_scene_knn<KB>, dim3(blocks), dim3(QUERY_BLOCK), 0, s, q); }
        { KernelScope ks(s, "k_scene_knn_deep"); hipLaunchKernelGGL(k_scene_knn_deep<KB>, dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q); }
    };
    if (q.k <= 8u) go(std::integral_constant<int, 8>{});
    else if (q.k <= 16u) go(std::integral_constant<int, 16>{});
    else go(std::integral_constant<int, KNN_MAX_K>{});
}

void warm_scene_knn() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_knn<8>)); }

} // namespace bvh
