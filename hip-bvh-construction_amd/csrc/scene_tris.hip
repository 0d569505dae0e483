// scene_tris.hip — bvh_scene_intersect_tris on gfx950: which triangles of which active instances does each query triangle properly cross (no counterpart in
// the reference).  bvh_scene_overlap's two-level walk (scene_overlap.hip: one query per lane, one LDS short stack shared by both levels, of two passing
// children the left one is entered and the right one pushed, count -> scan -> fill with the fill decided on the device, the MAPPED box of every record below a
// BLAS root, scene_map.hpp) with bvh_intersect_tris's exact narrow phase (tri_cross.hpp) run at the leaf, so no pair list travels through HBM.
//   query triangle i : QUERY mode: triangle i of the caller's world-space mesh, its format switched once per lane before the loop.  INSTANCE mode: the world
//                      triangle of primitive i of instance t.inst's BLAS — the BLAS index is read from the scene's instance array ON THE DEVICE, so the call
//                      needs no read-back; a row at or beyond that BLAS's n, and every row of an inactive instance, is empty; instance t.inst itself is
//                      skipped by index where the walk would enter it.
//   its box          : stage E's box of the three world vertices (tt_box), tested with box_overlap at the top level and against mapped(M_k, b) inside
//                      instance k (sov_box_pass) — the forward matrix stays in registers while the walk is inside an instance, the inverse is never read.
//   a passing leaf   : its BLAS triangle in the BLAS's format (switched at run time: lanes of one wave are in different instances), its three vertices mapped
//                      as V.r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 in f32 without contraction (the header's world triangle: a value that does not depend
//                      on the walk), then proper() and crosses() in f64 on those f32 values.  Both children's leaves go through ONE copy of the predicate (a
//                      two-trip loop that is not unrolled, as k_tris_walk).
//   k_scene_tris_walk : count pass (FILL = false) and fill pass (FILL = true); marks as k_scene_overlap_walk (count pass: the count word; fill pass: the
//                       prim_idx of the slice's first record — a query with an empty slice is not walked).
//   k_scene_tris_deep : after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked query from its start, stackless
//                       through the top-level plan and each entered BLAS's plan, left child first.  Both walks test the SAME boxes and the same triangles,
//                       so count and fill agree on a query's set whichever walk served it.
// Exactness: a vertex inside an object box maps into that box's mapped box as values (rounded products lie between the fminf and the fmaxf of
// the two end products, the sums are formed in the same association), so the mapped leaf box contains the world triangle; two crossing triangles share a
// point, so the query's box overlaps it; §8r carries the pair up both levels.
// Compiled WITHOUT the SLP vectoriser (Makefile), like both parents.
#include "query.hpp"
#include "tri_cross.hpp"
#include "scene_map.hpp"
#include "kernels.hpp"

namespace bvh {

// the query side of a launch: the caller's mesh and its format (QUERY mode), or the instance whose triangles ask (INSTANCE mode)
struct STQuery { TriSrc src; int fmt; u32 inst; };

// query triangle i; false: the row is empty (INSTANCE mode: an inactive or out-of-range query instance, a row at or beyond its BLAS's n)
template <int MODE>
__device__ __forceinline__ bool st_query(const SceneQuery& a, const STQuery& t, u32 i, QF3& x1, QF3& x2, QF3& x3) {
    if (MODE == BVH_SCENE_TRIS_QUERY) { tri_fetch_rt(t.fmt, t.src, i, x1, x2, x3); return true; }
    SOMat M; SceneBlas B;
    if (t.inst >= a.n_inst || !sov_enter_instance(a, t.inst, M, B) || i >= B.n) return false;
    st_world_tri(B, M, i, x1, x2, x3);
    return true;
}

// may the walk enter instance k?  (INSTANCE mode: the query's own instance is skipped by index; a second instance of the same BLAS is another instance)
template <int MODE> __device__ __forceinline__ bool st_may_enter(const SceneQuery& a, const STQuery& t, u32 k) {
    return k < a.n_inst && (MODE != BVH_SCENE_TRIS_INSTANCE || k != t.inst);
}

template <bool FILL, bool SORTED, int MODE>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_tris_walk(SceneQuery a, SceneHits h, STQuery t) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 tot = *h.total; if (tot > h.capacity || tot > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= a.n_rays) return;
    SceneOverlapSink<FILL, SORTED> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = h.offsets[i], end = h.offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = reinterpret_cast<uint2*>(h.hits) + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    QF3 x1{}, x2{}, x3{};
    const bool asked = st_query<MODE>(a, t, i, x1, x2, x3);
    const Box q = tt_box(x1, x2, x3);
    bool deep = false;
    if (asked && box_valid(q) && tt_proper(x1, x2, x3)) {         // (a query triangle that is not proper crosses nothing; an inverted box overlaps nothing)
        SOMat M{};
        SceneBlas B{};
        const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
        u32 ni = tni, total = ttotal;                                 // of the level the query is on
        bool in_blas = false, pop = false, entering = false;         // entering: instance `enter` is entered at the top of the next step
        u32 inst = INV, enter = INV;
        u32 nl = INV, nr = INV, top = 0, tsteps = 0, bsteps = 0;
        if (a.n_inst == 1) {                                          // no top-level tree: the instance's world box, then the instance
            if (box_overlap(q, box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)))) { enter = 0; entering = true; } else pop = true;
        } else {
            const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(a.tnodes) + a.troot); nl = lr.x; nr = lr.y;
        }
        for (;;) {
            if (entering) {
                entering = false;
                const u32 k = enter;
                if (st_may_enter<MODE>(a, t, k) && sov_enter_instance(a, k, M, B)) {
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
                bool ha = false, hb = false;
                if (nl < total) { rec_fetch_rt(layout, nodes, leaves, nl, ni, a0, a1, ba); ha = in_blas ? sov_box_pass(q, M, ba) : box_overlap(q, ba); }
                if (nr < total) { rec_fetch_rt(layout, nodes, leaves, nr, ni, b0, b1, bb); hb = in_blas ? sov_box_pass(q, M, bb) : box_overlap(q, bb); }
                if (in_blas) {                                        // triangles at once; at the top level a leaf is an instance, entered like a node
                    u32 pa = INV, pb = INV;                           // the leaf children that passed: their primitives, left first
                    if (ha && nl >= ni) { if (a0 < B.n) pa = a0; ha = false; }
                    if (hb && nr >= ni) { if (b0 < B.n) pb = b0; hb = false; }
                    if (pa == INV) { pa = pb; pb = INV; }
#pragma unroll 1
                    while (pa != INV) {
                        QF3 y1, y2, y3;
                        st_world_tri(B, M, pa, y1, y2, y3);
                        if (tt_proper(y1, y2, y3) && tt_crosses(x1, x2, x3, y1, y2, y3)) sink.put(pa, inst);
                        pa = pb; pb = INV;
                    }
                }
                if (ha || hb) {
                    if (ha && hb) {                                   // every passing subtree is visited: left first, right pushed
                        if (top == (u32)QUERY_STACK) { deep = true; break; }
                        stack[top * QUERY_BLOCK] = nr | (in_blas ? SCENE_BLAS_ENTRY : 0u); ++top;
                    }
                    const u32 n = ha ? nl : nr, c0 = ha ? a0 : b0, c1 = ha ? a1 : b1;
                    if (in_blas || n < tni) { nl = c0; nr = c1; }
                    else { enter = c0; entering = true; }             // a top-level leaf: its instance
                } else pop = true;
            }
            if (pop) {
                pop = false;
                if (top == 0) break;
                const u32 e = stack[--top * QUERY_BLOCK];
                if (e & SCENE_BLAS_ENTRY) {
                    const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(B.nodes) + (e & ~SCENE_BLAS_ENTRY)); nl = lr.x; nr = lr.y;
                } else {
                    if (in_blas) { in_blas = false; ni = tni; total = ttotal; }   // back to the top level
                    u32 w0, w1; Box b;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, e, tni, w0, w1, b);
                    if (e < tni) { nl = w0; nr = w1; } else { enter = w0; entering = true; }
                }
            }
        }
    }
    if (deep) atomicAdd(a.overflow, 1u);
    if (FILL) { if (deep) sink.out[0].x = QUERY_MARK; }
    else h.offsets[i] = deep ? QUERY_MARK : sink.k;
}

// stackless walk of instance k's BLAS through its plan (sov_walk_blas's arithmetic: the BLAS root's own box is not tested, every other record's is)
template <bool FILL, bool SORTED, int MODE>
__device__ void st_walk_blas(const SceneQuery& a, const STQuery& t, u32 k, const Box& q, QF3 x1, QF3 x2, QF3 x3, SceneOverlapSink<FILL, SORTED>& sink) {
    SOMat M; SceneBlas B;
    if (!st_may_enter<MODE>(a, t, k) || !sov_enter_instance(a, k, M, B)) return;
    const u32 ni = B.n - 1, total = 2 * B.n - 1;
    const u64 bound = 3ull * total + 3ull;
    u32 cur = B.root, last = INV;
    bool down = true;
    for (u64 steps = 0; cur < total && steps < bound; ++steps) {
        if (down) {
            u32 w0, w1; Box b;
            rec_fetch_rt((int)B.layout, B.nodes, B.leaves, cur, ni, w0, w1, b);
            if (cur >= ni) {
                if (sov_box_pass(q, M, b) && w0 < B.n) {
                    QF3 y1, y2, y3;
                    st_world_tri(B, M, w0, y1, y2, y3);
                    if (tt_proper(y1, y2, y3) && tt_crosses(x1, x2, x3, y1, y2, y3)) sink.put(w0, k);
                }
                last = cur; cur = B.parent[cur]; down = false;
                continue;
            }
            if (cur != B.root && !sov_box_pass(q, M, b)) { last = cur; cur = B.parent[cur]; down = false; continue; }   // (the BLAS root's own box: as the stack walk, not tested)
            if (w0 < total) { cur = w0; continue; }
            last = w0; down = false;                              // (a left link out of range: as if its subtree were done)
            continue;
        }
        if (cur >= ni) break;                                     // (parent links are internal nodes or INVALID)
        const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(B.nodes) + cur);
        if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
        last = cur; cur = B.parent[cur];
    }
}

// the stackless re-walk of the marked queries: the top-level plan, and for every instance whose world box passes, that BLAS's plan; left child first
template <bool FILL, bool SORTED, int MODE>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_tris_deep(SceneQuery a, SceneHits h, STQuery t) {
    if (*a.overflow == 0u) return;
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 bound = 3ull * ttotal + 3ull;
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < a.n_rays; i += nbid_x() * QUERY_BLOCK) {
        SceneOverlapSink<FILL, SORTED> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = h.offsets[i], end = h.offsets[i + 1];
            if (end <= base) continue;
            uint2* const out = reinterpret_cast<uint2*>(h.hits) + base;
            if (out[0].x != QUERY_MARK) continue;
            sink.out = out; sink.room = end - base;
        } else if (h.offsets[i] != QUERY_MARK) continue;
        QF3 x1{}, x2{}, x3{};
        if (!st_query<MODE>(a, t, i, x1, x2, x3)) continue;       // (never: a marked query was asked, and passed box_valid and tt_proper)
        const Box q = tt_box(x1, x2, x3);
        if (a.n_inst == 1) {
            if (box_overlap(q, box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)))) st_walk_blas<FILL, SORTED, MODE>(a, t, 0, q, x1, x2, x3, sink);
        } else {
            u32 cur = a.troot, last = INV;
            bool down = true;
            for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
                if (down) {
                    u32 w0, w1; Box b;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, cur, tni, w0, w1, b);
                    if (cur != a.troot && !box_overlap(q, b)) { last = cur; cur = a.tparent[cur]; down = false; continue; }   // (the root's own box: as the stack walk, not tested)
                    if (cur >= tni) {                                 // an instance whose world box passes
                        st_walk_blas<FILL, SORTED, MODE>(a, t, w0, q, x1, x2, x3, sink);
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
        if (!FILL) h.offsets[i] = sink.k;
    }
}

namespace {
template <bool FILL, bool SORTED, int MODE> void scene_tris_launch(hipStream_t s, const SceneQuery& q, const SceneHits& h, const STQuery& t) {
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    { KernelScope ks(s, FILL ? "k_scene_tris_fill" : "k_scene_tris_count");
      hipLaunchKernelGGL((k_scene_tris_walk<FILL, SORTED, MODE>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, q, h, t); }
    { KernelScope ks(s, "k_scene_tris_deep");                     // (the fill's overflow word stays 0 when the fill returned at once)
      hipLaunchKernelGGL((k_scene_tris_deep<FILL, SORTED, MODE>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q, h, t); }
}
template <bool FILL, bool SORTED> void scene_tris_pass(hipStream_t s, const SceneQuery& q, const SceneHits& h, const SceneTris& st) {
    const TrisMesh& m = st.queries;
    const STQuery t{ TriSrc{ m.d_tris, (const float*)m.d_vertices, (const u32*)m.d_indices, m.n_vertices }, m.tri_format, st.query_instance };
    if (st.mode == BVH_SCENE_TRIS_INSTANCE) scene_tris_launch<FILL, SORTED, BVH_SCENE_TRIS_INSTANCE>(s, q, h, t);
    else scene_tris_launch<FILL, SORTED, BVH_SCENE_TRIS_QUERY>(s, q, h, t);
}
} // namespace

void launch_scene_tris_count(hipStream_t s, const SceneQuery& q, const SceneHits& h, const SceneTris& t, uint64_t* d_sums, uint64_t* d_total) {
    scene_tris_pass<false, false>(s, q, h, t);
    launch_overlap_scan(s, h.offsets, q.n_rays, d_sums, d_total);
}

void launch_scene_tris_fill(hipStream_t s, int sorted, const SceneQuery& q, const SceneHits& h, const SceneTris& t) {
    if (sorted) scene_tris_pass<true, true>(s, q, h, t); else scene_tris_pass<true, false>(s, q, h, t);
}

void warm_scene_tris() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_tris_walk<false, false, BVH_SCENE_TRIS_QUERY>));
}

} // namespace bvh
