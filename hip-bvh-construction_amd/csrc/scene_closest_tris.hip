// scene_closest_tris.hip — bvh_scene_closest_tris on gfx950: the nearest triangle of an instanced scene to each query triangle, and the squared distance between
// the two (no counterpart in the reference).  One query triangle per lane.  The candidate of (instance k, primitive j) is bvh_closest_tris's dist2(X, Y) and
// feature (tt_dist2, closest_tris.hpp) with Y the WORLD triangle — the BLAS's vertices mapped by the instance's forward matrix (st_world_tri, scene_map.hpp) —
// so dist2 and feature are world-space values that do not depend on the walk.  The walk itself runs in object space, as scene_point.hip's: inside instance k the
// three query vertices are mapped as x'_i = W_k x_i, and a node box is tested against
//   the componentwise min/max box of the x'_i, grown on every axis by QUERY_GROW * (its largest |coordinate|) + e,  e = the largest of the point queries' slack
//   (scene_slack, scene_query.hpp) over the three vertices;   the node box grown by QUERY_GROW * (its largest |coordinate|);   culled iff s2 * lb' * (1 - 2^-20) > best,
// with lb' the f32 sum of the squared per-axis gaps (box_box_dist_pass's), s2 the instance's scale bound and best the world dist2 so far, carried across
// instances.  DESIGN.md §8y has the argument (§8n's for every point of the query triangle: W is affine, so W x lies in the box of the W x_i).  The top level is
// box_box_dist_pass on the world boxes with the query's stage-E box grown once: the same test with s2 = 1, which is how the shared loop states it (1 * lb is
// exact and lb is never NaN).
//   query triangle i : QUERY mode: triangle i of the caller's world-space mesh.  INSTANCE mode: the world triangle of primitive i of instance t.inst, looked up
//                      on the device as scene_tris.hip does; that instance is skipped by index where the walk would enter it.
//   k_scene_closest_tris      : one per-lane LDS short stack shared by both levels (k_scene_closest_point's structure), near child first by lower bound at both
//                               levels, leaf children whose box passes tested at once through ONE copy of the leaf routine (closest_tris.hip's two-trip loop).
//                               The nine world query coordinates stay live; the object query box, e and s2 are recomputed when an instance is entered; the
//                               forward matrix and the BLAS descriptor are re-loaded per leaf test (the scene's copy of the caller's records, and 64 bytes
//                               that L2 serves); the query's world boxes are recomputed at the leaf and on the way back to the top level rather than held
//                               through the BLAS walk.
//   k_scene_closest_tris_deep : the marked queries (QUERY_MARK in prim_idx), stackless: the top-level plan, and for every instance whose world box passes, that
//                               BLAS's plan, with the same boxes and the same candidates.
// A leaf pair whose two WORLD stage-E boxes fail the flat rule against the current best is skipped before any term is computed.
// Built without the SLP vectoriser (Makefile), as both parents: the record update is the same tie-breaking pattern.
#include "scene_tris_query.hpp"

namespace bvh {

// the best candidate so far: world dist2, prim and instance (INV: none), feature
struct SCBest { float d2; u32 prim, feat, inst; };

// (the query side, the box test on both levels and the entry into an instance are scene_tris_query.hpp's, shared with scene_radius_tris.hip)
// the candidate of (inst, prim), prim < n of BLAS bl: dist2(X, world triangle) and the record update in the order (dist2, instance, prim).  best starts at
// {r2, INV, 0, INV}, so the comparison is also the acceptance test d2 <= r2 (NaN fails both).  True when an any-hit query is done.  The BLAS descriptor is
// re-loaded here, like the matrix: the walk keeps only what it reads at every step (SCWalk)
template <int QUERY>
__device__ __forceinline__ bool scene_leaf_tris(const SceneQuery& a, u32 bl, u32 prim, u32 inst, QF3 x1, QF3 x2, QF3 x3, bool xproper, SCBest& best) {
    const SceneBlas B = a.blas[bl];
    QF3 y1, y2, y3;
    st_world_tri(B, inst_load_m(a, inst), prim, y1, y2, y3);
    const Box xb = tt_box(x1, x2, x3), xg = box_grown(xb), yb = tt_box(y1, y2, y3);
    float lb;
    if (!box_box_dist_pass(yb, xg, best.d2, lb)) return false;    // the pair's own world boxes are already too far apart for the current best
    u32 feat;
    const float d2 = tt_dist2(x1, x2, x3, xproper, xb, y1, y2, y3, yb, feat);
    if (!(d2 < best.d2 || (d2 == best.d2 && (inst < best.inst || (inst == best.inst && prim < best.prim))))) return false;
    best.d2 = d2; best.prim = prim; best.feat = feat; best.inst = inst;
    return QUERY == BVH_QUERY_ANY;
}

__device__ __forceinline__ void scene_tri_hit_store(void* hits, u32 i, const SCBest& b) {
    reinterpret_cast<uint4*>(hits)[i] = make_uint4(__float_as_uint(b.d2), b.prim, b.feat, b.inst);
}

// amdgpu_waves_per_eu(2, 2): the closest-hit instances need 254-255 registers; left alone the allocator takes 254 VGPRs plus 8 AGPR copies, which is past the 256
// of two waves per SIMD (the 16 KiB stack allows no more than two anyway).  Held to two waves it fits in 255 VGPRs with no AGPR copy and no scratch
template <int QUERY, int MODE>
__global__ __launch_bounds__(QUERY_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_scene_closest_tris(SceneQuery a, SCQuery t) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= a.n_rays) return;
    u32* const stack = s_stack + tid_x();
    QF3 x1{}, x2{}, x3{}; float r2;
    const bool live = sc_query_load<MODE>(a, t, i, x1, x2, x3, r2);
    SCBest best{ r2, INV, 0u, INV };
    bool deep = false;
    if (live) {
        const bool xproper = tt_proper(x1, x2, x3);
        SCBox c = sc_world_box(x1, x2, x3);
        SCWalk B{};
        const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
        u32 ni = tni, total = ttotal;                                 // of the level the query is on
        bool in_blas = false, pop = false, entering = false;         // entering: instance `enter` is entered at the top of the next step
        u32 inst = INV, enter = INV;
        u32 nl = INV, nr = INV, top = 0, tsteps = 0, bsteps = 0;
        if (a.n_inst == 1) {                                          // no top-level tree: the instance's world box, then the instance
            float lb;
            if (scene_box_box_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), c, best.d2, lb)) { enter = 0; entering = true; } else pop = true;
        } else {
            const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(a.tnodes) + a.troot); nl = lr.x; nr = lr.y;
        }
        for (;;) {
            if (entering) {
                entering = false;
                const u32 k = enter;
                SceneBlas D; u32 bl;
                if (sc_may_enter<MODE>(a, t, k) && enter_instance_tris(a, k, x1, x2, x3, c, D, bl)) {
                    B = { D.nodes, D.leaves, D.n, D.layout, bl };
                    in_blas = true; inst = k; ni = B.n - 1; total = 2 * B.n - 1; bsteps = 0;
                    const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(D.nodes) + D.root); nl = lr.x; nr = lr.y;
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
                if (nl < total) { rec_fetch_rt(layout, nodes, leaves, nl, ni, a0, a1, ba); ha = scene_box_box_pass(ba, c, best.d2, la); }
                if (nr < total) { rec_fetch_rt(layout, nodes, leaves, nr, ni, b0, b1, bb); hb = scene_box_box_pass(bb, c, best.d2, lb); }
                if (in_blas) {                                        // triangles at once; at the top level a leaf is an instance, entered like a node
                    u32 pa = INV, pb = INV;                           // the leaf children that passed: their primitives, left first (out of range: never followed)
                    if (ha && nl >= ni) { if (a0 < B.n) pa = a0; ha = false; }
                    if (hb && nr >= ni) { if (b0 < B.n) pb = b0; hb = false; }
                    if (pa == INV) { pa = pb; pb = INV; }
                    bool done = false;
#pragma unroll 1
                    while (pa != INV) {
                        done = scene_leaf_tris<QUERY>(a, B.bl, pa, inst, x1, x2, x3, xproper, best);
                        if (done) break;
                        pa = pb; pb = INV;
                    }
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
                    if (in_blas) { c = sc_world_box(x1, x2, x3); in_blas = false; ni = tni; total = ttotal; }   // back to the top level: the world box
                    u32 w0, w1; Box b;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, e, tni, w0, w1, b);
                    if (e < tni) { nl = w0; nr = w1; } else { enter = w0; entering = true; }
                }
            }
        }
    }
    if (deep) {
        const SCBest mark{ r2, QUERY_MARK, 0u, INV };
        scene_tri_hit_store(a.hits, i, mark); atomicAdd(a.overflow, 1u);
    } else scene_tri_hit_store(a.hits, i, best);
}

// stackless walk of instance k's BLAS (k_closest_tris_deep's walk through the BLAS's plan); true when an any-hit query is done
template <int QUERY, int MODE>
__device__ bool scene_tris_dist_walk_blas(const SceneQuery& a, const SCQuery& t, u32 k, QF3 x1, QF3 x2, QF3 x3, bool xproper, SCBest& best) {
    SCBox c; SceneBlas B; u32 bl;
    if (!sc_may_enter<MODE>(a, t, k) || !enter_instance_tris(a, k, x1, x2, x3, c, B, bl)) return false;
    const u32 ni = B.n - 1, total = 2 * B.n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    u32 cur = B.root, last = INV;
    bool down = true;
    for (u64 steps = 0; cur < total && steps < bound; ++steps) {
        u32 w0, w1; Box b;
        if (down) {
            rec_fetch_rt((int)B.layout, B.nodes, B.leaves, cur, ni, w0, w1, b);
            float lb;
            const bool pass = scene_box_box_pass(b, c, best.d2, lb);
            if (cur >= ni) {
                if (pass && w0 < B.n && scene_leaf_tris<QUERY>(a, bl, w0, k, x1, x2, x3, xproper, best)) return true;
                last = cur; cur = B.parent[cur]; down = false;
                continue;
            }
            if (!pass) { last = cur; cur = B.parent[cur]; down = false; continue; }
            if (w0 < total) { cur = w0; continue; }
            last = w0; down = false;                              // (a left link out of range: as if its subtree were done)
            continue;
        }
        if (cur >= ni) break;                                     // (parent links are internal nodes or INVALID)
        const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(B.nodes) + cur);
        if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
        last = cur; cur = B.parent[cur];
    }
    return false;
}

template <int QUERY, int MODE>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_closest_tris_deep(SceneQuery a, SCQuery t) {
    if (*a.overflow == 0u) return;
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 bound = 3ull * ttotal + 3ull;
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < a.n_rays; i += nbid_x() * QUERY_BLOCK) {
        if (reinterpret_cast<const u32*>(a.hits)[4 * (size_t)i + 1] != QUERY_MARK) continue;
        QF3 x1{}, x2{}, x3{}; float r2;
        sc_query_load<MODE>(a, t, i, x1, x2, x3, r2);             // (a marked query passed the checks)
        const bool xproper = tt_proper(x1, x2, x3);
        const SCBox world = sc_world_box(x1, x2, x3);
        SCBest best{ r2, INV, 0u, INV };
        if (a.n_inst == 1) {
            float lb;
            if (scene_box_box_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), world, best.d2, lb))
                scene_tris_dist_walk_blas<QUERY, MODE>(a, t, 0, x1, x2, x3, xproper, best);
        } else {
            u32 cur = a.troot, last = INV;
            bool down = true;
            for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
                u32 w0, w1; Box b;
                if (down) {
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, cur, tni, w0, w1, b);
                    float lb;
                    if (!scene_box_box_pass(b, world, best.d2, lb)) { last = cur; cur = a.tparent[cur]; down = false; continue; }
                    if (cur >= tni) {                                 // an instance whose world box passes
                        if (scene_tris_dist_walk_blas<QUERY, MODE>(a, t, w0, x1, x2, x3, xproper, best)) break;
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
        scene_tri_hit_store(a.hits, i, best);
    }
}

namespace {
template <int QUERY, int MODE> void scene_closest_tris_launch(hipStream_t s, const SceneQuery& q, const SCQuery& t) {
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    { KernelScope ks(s, "k_scene_closest_tris");
      hipLaunchKernelGGL((k_scene_closest_tris<QUERY, MODE>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, q, t); }
    { KernelScope ks(s, "k_scene_closest_tris_deep");
      hipLaunchKernelGGL((k_scene_closest_tris_deep<QUERY, MODE>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q, t); }
}
} // namespace

void launch_scene_closest_tris(hipStream_t s, int query, float radius, const SceneQuery& q, const SceneTris& st) {
    const TrisMesh& m = st.queries;
    const SCQuery t{ TriSrc{ m.d_tris, (const float*)m.d_vertices, (const u32*)m.d_indices, m.n_vertices }, m.tri_format, st.query_instance, radius };
    const bool any = query == BVH_QUERY_ANY;
    if (st.mode == BVH_SCENE_TRIS_INSTANCE) {
        if (any) scene_closest_tris_launch<BVH_QUERY_ANY, BVH_SCENE_TRIS_INSTANCE>(s, q, t);
        else scene_closest_tris_launch<BVH_QUERY_CLOSEST, BVH_SCENE_TRIS_INSTANCE>(s, q, t);
    } else {
        if (any) scene_closest_tris_launch<BVH_QUERY_ANY, BVH_SCENE_TRIS_QUERY>(s, q, t);
        else scene_closest_tris_launch<BVH_QUERY_CLOSEST, BVH_SCENE_TRIS_QUERY>(s, q, t);
    }
}

void warm_scene_closest_tris() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_closest_tris<BVH_QUERY_CLOSEST, BVH_SCENE_TRIS_QUERY>));
}

} // namespace bvh
