// scene_point.hip — bvh_scene_closest_point on gfx950: closest-point / any-within-radius queries against an instanced scene (no counterpart in the reference).
// One query per lane.  The candidate of (instance k, primitive j) is bvh_closest_point's formula (tri_closest, query.hpp) on the WORLD triangle — the BLAS's
// vertices mapped by the instance's forward matrix — so point and dist2 are world-space values that do not depend on the walk.  The walk itself runs in object
// space: distances do not survive a general 3x4 transform, so a node box of instance k is tested against the mapped point p' = W_k p with
//   the box grown on every axis by QUERY_GROW * (its largest |coordinate|) + e,   e = 2^-20 max_i(((|w_i0||px| + |w_i1||py|) + |w_i2||pz|) + |w_i3|),
//   culled iff s2 * lb' * (1 - 2^-20) > best,
// with lb' the grown box's f32 squared distance to p', s2 the instance's scale bound (k_instance_boxes: |M x - p|^2 >= s2 |x - W p|^2 for every object point x)
// and best the world-space dist2 so far, carried across instances.  DESIGN.md §8n has the argument.  The top level is box_dist_pass on the world boxes with the
// world point: the same test with e = 0 and s2 = 1, which is how the shared loop states it (1 * lb and g + 0 are exact, lb is never NaN).
//   k_scene_closest_point      : one per-lane LDS short stack shared by both levels (k_scene_intersect's structure), near child first by lower bound at both
//                                levels, leaf children whose box passes tested at once.  The forward matrix is re-loaded per leaf test from the scene's copy of
//                                the caller's records (12 floats that L2 serves; keeping them live across the BLAS walk would cost 12 VGPRs all the way).
//   k_scene_closest_point_deep : the marked queries, stackless: the top-level plan, and for every instance whose world box passes, that BLAS's plan.
// The box test (scene_box_dist_pass), the entry into an instance (enter_instance_point) and the world triangle (blas_world_tri) are scene_query.hpp's, shared
// with scene_knn.hip (the first two) and scene_radius.hip.
// Built without the SLP vectoriser (Makefile), as scene.o and point_query.o: the record update is the same tie-breaking pattern.
#include "scene_query.hpp"

namespace bvh {

// the best candidate so far: world closest point, world dist2, weights, prim and instance (INV: none)
struct SPBest { QF3 q; float d2, u, v; u32 prim, inst; };

// the candidate of (inst, prim): the world triangle's closest point to the world point w; the record update in the order (dist2, instance, prim).  best starts
// at {r2, INV, INV}, so the comparison is also the acceptance test d2 <= r2 (NaN fails both).  True when an any-hit query is done.
template <int QUERY>
__device__ __forceinline__ bool scene_leaf_point(const SceneQuery& a, const SceneBlas& B, u32 prim, u32 inst, QF3 w, SPBest& best) {
    if (prim >= B.n) return false;
    QF3 wa, wb, wc;
    blas_world_tri(a, B, prim, inst, wa, wb, wc);
    QF3 q; float u, v;
    const float d2 = tri_closest(wa, wb, wc, w, q, u, v);
    if (!(d2 < best.d2 || (d2 == best.d2 && (inst < best.inst || (inst == best.inst && prim < best.prim))))) return false;
    best.q = q; best.d2 = d2; best.u = u; best.v = v; best.prim = prim; best.inst = inst;
    return QUERY == BVH_QUERY_ANY;
}

__device__ __forceinline__ void scene_point_hit_store(void* hits, u32 i, const SPBest& b) {
    float4* h = reinterpret_cast<float4*>(hits) + 2 * (size_t)i;
    const bool hit = b.prim != INV;
    h[0] = hit ? make_float4(b.q.x, b.q.y, b.q.z, b.d2) : make_float4(0.0f, 0.0f, 0.0f, b.d2);
    h[1] = hit ? make_float4(b.u, b.v, __uint_as_float(b.prim), __uint_as_float(b.inst)) : make_float4(0.0f, 0.0f, __uint_as_float(INV), __uint_as_float(INV));
}

template <int QUERY>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_closest_point(SceneQuery a) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= a.n_rays) return;
    u32* const stack = s_stack + tid_x();
    QF3 w; float r2;
    const bool live = point_load(reinterpret_cast<const bvh_point_query*>(a.rays), i, w, r2);
    SPBest best{ { 0.0f, 0.0f, 0.0f }, r2, 0.0f, 0.0f, INV, INV };
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
            if (scene_box_dist_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), world, best.d2, lb)) { enter = 0; entering = true; } else pop = true;
        } else {
            const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(a.tnodes) + a.troot); nl = lr.x; nr = lr.y;
        }
        for (;;) {
            if (entering) {
                entering = false;
                const u32 k = enter;
                if (k < a.n_inst && enter_instance_point(a, k, w, c, B)) {
                    in_blas = true; inst = k; ni = B.n - 1; total = 2 * B.n - 1; bsteps = 0;
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
                if (nl < total) { rec_fetch_rt(layout, nodes, leaves, nl, ni, a0, a1, ba); ha = scene_box_dist_pass(ba, c, best.d2, la); }
                if (nr < total) { rec_fetch_rt(layout, nodes, leaves, nr, ni, b0, b1, bb); hb = scene_box_dist_pass(bb, c, best.d2, lb); }
                if (in_blas) {                                        // triangles at once; at the top level a leaf is an instance, entered like a node
                    bool done = false;
                    if (ha && nl >= ni) { done = scene_leaf_point<QUERY>(a, B, a0, inst, w, best); ha = false; }
                    if (hb && nr >= ni && !done) { done = scene_leaf_point<QUERY>(a, B, b0, inst, w, best); hb = false; }
                    if (done) break;
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
    if (deep) {
        const SPBest mark{ { 0.0f, 0.0f, 0.0f }, r2, 0.0f, 0.0f, QUERY_MARK, INV };
        scene_point_hit_store(a.hits, i, mark); atomicAdd(a.overflow, 1u);
    } else scene_point_hit_store(a.hits, i, best);
}

// stackless walk of instance k's BLAS (k_closest_point_deep's walk through the BLAS's plan); true when an any-hit query is done
template <int QUERY>
__device__ bool scene_point_walk_blas(const SceneQuery& a, u32 k, QF3 w, SPBest& best) {
    ScenePoint c; SceneBlas B;
    if (k >= a.n_inst || !enter_instance_point(a, k, w, c, B)) return false;
    const u32 ni = B.n - 1, total = 2 * B.n - 1;
    const u64 bound = 3ull * total + 3ull;
    u32 cur = B.root, last = INV;
    bool down = true;
    for (u64 steps = 0; cur < total && steps < bound; ++steps) {
        u32 w0, w1; Box b;
        if (down) {
            rec_fetch_rt((int)B.layout, B.nodes, B.leaves, cur, ni, w0, w1, b);
            float lb;
            const bool pass = scene_box_dist_pass(b, c, best.d2, lb);
            if (cur >= ni) {
                if (pass && scene_leaf_point<QUERY>(a, B, w0, k, w, best)) return true;
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
    return false;
}

template <int QUERY>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_closest_point_deep(SceneQuery a) {
    if (*a.overflow == 0u) return;
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 bound = 3ull * ttotal + 3ull;
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < a.n_rays; i += nbid_x() * QUERY_BLOCK) {
        if (reinterpret_cast<const u32*>(a.hits)[8 * (size_t)i + 6] != QUERY_MARK) continue;
        QF3 w; float r2;
        point_load(reinterpret_cast<const bvh_point_query*>(a.rays), i, w, r2);   // (a marked query passed the checks)
        const ScenePoint world{ w, 0.0f, 1.0f };
        SPBest best{ { 0.0f, 0.0f, 0.0f }, r2, 0.0f, 0.0f, INV, INV };
        if (a.n_inst == 1) {
            float lb;
            if (scene_box_dist_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), world, best.d2, lb)) scene_point_walk_blas<QUERY>(a, 0, w, best);
        } else {
            u32 cur = a.troot, last = INV;
            bool down = true;
            for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
                u32 w0, w1; Box b;
                if (down) {
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, cur, tni, w0, w1, b);
                    float lb;
                    if (!scene_box_dist_pass(b, world, best.d2, lb)) { last = cur; cur = a.tparent[cur]; down = false; continue; }
                    if (cur >= tni) {                                 // an instance whose world box passes
                        if (scene_point_walk_blas<QUERY>(a, w0, w, best)) break;
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
        scene_point_hit_store(a.hits, i, best);
    }
}

void launch_scene_closest_point(hipStream_t s, int query, const SceneQuery& q) {
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    { KernelScope ks(s, "k_scene_closest_point");
      if (query == BVH_QUERY_ANY) hipLaunchKernelGGL(k_scene_closest_point<BVH_QUERY_ANY>, dim3(blocks), dim3(QUERY_BLOCK), 0, s, q);
      else hipLaunchKernelGGL(k_scene_closest_point<BVH_QUERY_CLOSEST>, dim3(blocks), dim3(QUERY_BLOCK), 0, s, q); }
    { KernelScope ks(s, "k_scene_closest_point_deep");
      if (query == BVH_QUERY_ANY) hipLaunchKernelGGL(k_scene_closest_point_deep<BVH_QUERY_ANY>, dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q);
      else hipLaunchKernelGGL(k_scene_closest_point_deep<BVH_QUERY_CLOSEST>, dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q); }
}

void warm_scene_point() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_closest_point<BVH_QUERY_CLOSEST>)); }

} // namespace bvh
