// scene_overlap.hip — bvh_scene_overlap on gfx950: which triangles' leaf boxes of which active instances does each WORLD-space query box touch (no counterpart
// in the reference).  The two-level walk is scene_radius.hip's (one query per lane, one LDS short stack shared by both levels, of two passing children the left
// one is entered and the right one pushed, count -> scan -> fill with the fill decided on the device) and the test is bvh_overlap's closed, comparisons-only
// box_overlap — at the top level on the top-level nodes and the instances' world boxes, inside instance k on the MAPPED box of every record below the BLAS root:
//   mapped(M, {lo, hi}), row r:  a_c = m_rc * lo.c, b_c = m_rc * hi.c,  min.r = ((fminf(a_0, b_0) + fminf(a_1, b_1)) + fminf(a_2, b_2)) + m_r3,  max.r with fmaxf
// in f32 without contraction (the file is built with -ffp-contract=off).  Rounded multiplication by a fixed factor and rounded addition are monotone, so the
// mapped box of a parent contains its children's mapped boxes as values whenever every mapped value is finite, and the instance's world box (the 8 mapped
// corners of the BLAS root box: the same values) contains them all: the walk reaches every passing leaf and the answer is exact on EVERY query.
// A record whose OBJECT box is not valid (a min above its max, a NaN) fails before it is mapped: fminf / fmaxf would turn an inverted box into a valid one.
//   k_scene_overlap_walk : count pass (FILL = false: d_offsets[i] = query i's number of passing (instance, prim) pairs) and fill pass (FILL = true: the
//                          8-byte records go to the query's slice).  A query whose push would overflow, or whose walk is longer than its level's node count, is
//                          marked and bumps the pass's overflow word.  Count pass: the mark is the count word (a count saturates at QUERY_MARK - 1).  Fill pass: a
//                          query with an empty slice is not walked, so a marked query has a record and the mark is the prim_idx of its slice's first record.
//   k_scene_overlap_deep : launched after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked query from its start,
//                          stackless through the top-level plan and each entered BLAS's plan, left child first.  Both walks test the SAME boxes — every record
//                          below a root, and neither the top-level root's own box nor a BLAS root's own box (the instance's world box stands for it) — so count
//                          and fill agree on a query's set whichever walk served it, and the answer does not depend on QUERY_STACK.
// Fill: a lane writes whole 8-byte records (one uint2) into its own slice and never past it; no atomics.  SORTED: the slice is kept in ascending
// (instance, prim) order by comparing and shifting whole records from its tail on the u64 key (instance << 32) | prim.  The insertion is quadratic in the
// slice's length.
// Compiled WITHOUT the SLP vectoriser (Makefile), like its scene siblings: the mapped box is 18 products, 18 adds and 18 min/max that it would pack into v_pk_*.
// The forward matrix, the mapped box, the instance entry and the record sink live in scene_map.hpp, which scene_tris.hip shares.
#include "query.hpp"
#include "scene_map.hpp"
#include "kernels.hpp"

namespace bvh {

template <bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_overlap_walk(SceneQuery a, SceneHits h) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 t = *h.total; if (t > h.capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= a.n_rays) return;
    SceneOverlapSink<FILL, SORTED> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = h.offsets[i], end = h.offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = reinterpret_cast<uint2*>(h.hits) + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    const Box q = box_load_u(reinterpret_cast<const bvh_aabb*>(a.rays) + i);
    bool deep = false;
    if (box_valid(q)) {                                           // (NaN or inverted: overlaps nothing)
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
                if (k < a.n_inst && sov_enter_instance(a, k, M, B)) {
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
                    if (ha && nl >= ni) { if (a0 < B.n) sink.put(a0, inst); ha = false; }
                    if (hb && nr >= ni) { if (b0 < B.n) sink.put(b0, inst); hb = false; }
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

// stackless walk of instance k's BLAS through its plan (srad_walk_blas's arithmetic: the BLAS root's own box is not tested, every other record's is)
template <bool FILL, bool SORTED>
__device__ void sov_walk_blas(const SceneQuery& a, u32 k, const Box& q, SceneOverlapSink<FILL, SORTED>& sink) {
    SOMat M; SceneBlas B;
    if (k >= a.n_inst || !sov_enter_instance(a, k, M, B)) return;
    const u32 ni = B.n - 1, total = 2 * B.n - 1;
    const u64 bound = 3ull * total + 3ull;
    u32 cur = B.root, last = INV;
    bool down = true;
    for (u64 steps = 0; cur < total && steps < bound; ++steps) {
        if (down) {
            u32 w0, w1; Box b;
            rec_fetch_rt((int)B.layout, B.nodes, B.leaves, cur, ni, w0, w1, b);
            if (cur >= ni) {
                if (sov_box_pass(q, M, b) && w0 < B.n) sink.put(w0, k);
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
template <bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_overlap_deep(SceneQuery a, SceneHits h) {
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
        const Box q = box_load_u(reinterpret_cast<const bvh_aabb*>(a.rays) + i);   // (a marked query passed box_valid)
        if (a.n_inst == 1) {
            if (box_overlap(q, box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)))) sov_walk_blas(a, 0, q, sink);
        } else {
            u32 cur = a.troot, last = INV;
            bool down = true;
            for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
                if (down) {
                    u32 w0, w1; Box b;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, cur, tni, w0, w1, b);
                    if (cur != a.troot && !box_overlap(q, b)) { last = cur; cur = a.tparent[cur]; down = false; continue; }   // (the root's own box: as the stack walk, not tested)
                    if (cur >= tni) {                                 // an instance whose world box passes
                        sov_walk_blas(a, w0, q, sink);
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
template <bool FILL, bool SORTED> void scene_overlap_pass(hipStream_t s, const SceneQuery& q, const SceneHits& h) {
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    { KernelScope ks(s, FILL ? "k_scene_overlap_fill" : "k_scene_overlap_count");
      hipLaunchKernelGGL((k_scene_overlap_walk<FILL, SORTED>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, q, h); }
    { KernelScope ks(s, "k_scene_overlap_deep");                  // (the fill's overflow word stays 0 when the fill returned at once)
      hipLaunchKernelGGL((k_scene_overlap_deep<FILL, SORTED>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q, h); }
}
} // namespace

void launch_scene_overlap_count(hipStream_t s, const SceneQuery& q, const SceneHits& h, uint64_t* d_sums, uint64_t* d_total) {
    scene_overlap_pass<false, false>(s, q, h);
    launch_overlap_scan(s, h.offsets, q.n_rays, d_sums, d_total);
}

void launch_scene_overlap_fill(hipStream_t s, int sorted, const SceneQuery& q, const SceneHits& h) {
    if (sorted) scene_overlap_pass<true, true>(s, q, h); else scene_overlap_pass<true, false>(s, q, h);
}

void warm_scene_overlap() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_overlap_walk<false, false>)); }

} // namespace bvh
