// scene_radius_tris.hip — bvh_scene_radius_tris on gfx950: EVERY triangle of an instanced scene within a distance of each query triangle, with its squared
// distance and feature pair (no counterpart in the reference).  One query triangle per lane.  Nothing here is new arithmetic: the candidate of (instance k,
// primitive j) is bvh_closest_tris's dist2(X, Y) and feature (tt_dist2, closest_tris.hpp) with Y the WORLD triangle (st_world_tri, scene_map.hpp); the query
// side, the two-level object-space walk and its box test are scene_closest_tris.hip's (scene_tris_query.hpp); the count -> scan -> fill scheme, the
// marks and the sorted insertion are scene_radius.hip's and radius_tris.hip's.  What differs from k_scene_closest_tris is what differs between
// k_radius_tris_walk and k_closest_tris: the bound never shrinks — every box test runs against r2 for the whole walk — so every passing subtree is visited, of
// two passing children the left one is entered and the right one pushed (near-first ordering buys nothing), and the answer is a set of
// {dist2, prim, feature, instance} records.  DESIGN.md §8za.
//   k_scene_radius_tris_walk : count pass (FILL = false: d_offsets[i] = query i's number of accepted candidates) and fill pass (FILL = true: the records go to
//                              the query's slice).  One per-lane LDS short stack shared by both levels; leaf children whose box passes are tested at once
//                              through ONE copy of the leaf routine (the two-trip loop that is not unrolled).  The nine world query coordinates stay live;
//                              the object query box and s2 are recomputed when an instance is entered; the forward matrix and the BLAS descriptor are
//                              re-loaded per leaf test; the query's world boxes are recomputed at the leaf and on the way back to the top level.  A query
//                              whose push would overflow, or whose walk is longer than its level's node count, is marked and bumps the pass's overflow word.
//                              Count pass: the mark is the count word (a count saturates at QUERY_MARK - 1, so the mark is never a count).  Fill pass: a
//                              query with an empty slice is not walked, so a marked query has a record and the mark is the prim_idx of its slice's first
//                              record.
//   k_scene_radius_tris_deep : launched after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked query from its
//                              start, stackless through the top-level plan and each entered BLAS's plan, left child first.  Both walks test the SAME boxes —
//                              every record below a root, and neither the top-level root's own box nor a BLAS root's own box (the instance's world box
//                              stands for it) — so count and fill agree on a query's set whichever walk served it, and the answer does not depend on
//                              QUERY_STACK.
// The leaf: the world triangle; the pair's own two WORLD stage-E boxes against r2 (the flat rule) before any term; then tt_dist2 and the acceptance
// dist2 <= r2 (a NaN dist2 fails).  Identical in count and fill.
// Fill: a lane writes whole 16-byte records (one uint4) into its own slice and never past it; no atomics.  SORTED: the slice is kept in ascending
// (dist2, instance, prim) order by comparing and shifting whole records from its tail, on the u64 key (float_as_uint(dist2) << 32) | instance and then the
// prim: an accepted dist2 is 0 or a sum of squares, never negative and never NaN, so that is the contract's lexicographic order.  The insertion is quadratic in
// the slice's length.
// Built WITHOUT the SLP vectoriser (Makefile), like scene_closest_tris.hip (the leaf's 15 terms are stated operation for operation) and scene_radius.hip (the
// sorted insertion compares and replaces records).
#include "scene_tris_query.hpp"

namespace bvh {

static_assert(sizeof(bvh_instance_tri_hit) == sizeof(uint4), "a record leaves in one 16-byte store");

// where a walk's records go (scene_radius.hip's SceneRadiusSink for bvh_instance_tri_hit records {dist2 bits, prim, feature, instance})
template <bool FILL, bool SORTED> struct SceneRadiusTrisSink {
    uint4* out; u32 room, k = 0;
    __device__ __forceinline__ void put(float d2, u32 prim, u32 feat, u32 inst) {
        if (FILL) {
            if (k < room) {
                u32 j = k;
                const u32 db = __float_as_uint(d2);
                if (SORTED) {
                    const u64 key = ((u64)db << 32) | inst;
                    while (j > 0) {                               // (records above (dist2, inst, prim) move up by one; the slice below j + 1 stays sorted)
                        const uint4 p = out[j - 1];
                        const u64 pk = ((u64)p.x << 32) | p.w;
                        if (pk < key || (pk == key && p.y < prim)) break;
                        out[j] = p; --j;
                    }
                }
                out[j] = make_uint4(db, prim, feat, inst);
            }
        }
        if (k < QUERY_MARK - 1u) ++k;                             // (many instances of one BLAS can answer: the counter saturates below the mark)
    }
};

// the candidate of (inst, prim), prim < n of BLAS bl: dist2(X, world triangle), accepted iff dist2 <= r2 (a NaN dist2 fails).  The BLAS descriptor and the
// forward matrix are re-loaded here and the query's two world boxes recomputed (scene_leaf_tris, scene_closest_tris.hip): none of them lives across the walk
template <bool FILL, bool SORTED>
__device__ __forceinline__ void srt_leaf(const SceneQuery& a, u32 bl, u32 prim, u32 inst, QF3 x1, QF3 x2, QF3 x3, bool xproper, float r2,
                                         SceneRadiusTrisSink<FILL, SORTED>& sink) {
    const SceneBlas B = a.blas[bl];
    QF3 y1, y2, y3;
    st_world_tri(B, inst_load_m(a, inst), prim, y1, y2, y3);
    const Box xb = tt_box(x1, x2, x3), xg = box_grown(xb), yb = tt_box(y1, y2, y3);
    float lb;
    if (!box_box_dist_pass(yb, xg, r2, lb)) return;               // the pair's own world boxes are already too far apart
    u32 feat;
    const float d2 = tt_dist2(x1, x2, x3, xproper, xb, y1, y2, y3, yb, feat);
    if (d2 <= r2) sink.put(d2, prim, feat, inst);
}

// amdgpu_waves_per_eu(2, 2): as k_scene_closest_tris — the 16 KiB stack allows no more than two waves per SIMD anyway, and held to two the allocator has all
// 256 registers before it makes AGPR copies or spills
template <int MODE, bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_scene_radius_tris_walk(SceneQuery a, SCQuery t, SceneHits h) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 tot = *h.total; if (tot > h.capacity || tot > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= a.n_rays) return;
    SceneRadiusTrisSink<FILL, SORTED> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = h.offsets[i], end = h.offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = reinterpret_cast<uint4*>(h.hits) + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    QF3 x1{}, x2{}, x3{}; float r2;
    const bool live = sc_query_load<MODE>(a, t, i, x1, x2, x3, r2);
    bool deep = false;
    if (live) {                                                   // (a row that is not asked, a NaN coordinate, a NaN or negative radius: accepts nothing)
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
            if (scene_box_box_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), c, r2, lb)) { enter = 0; entering = true; } else pop = true;
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
                float la, lb;
                bool ha = false, hb = false;
                if (nl < total) { rec_fetch_rt(layout, nodes, leaves, nl, ni, a0, a1, ba); ha = scene_box_box_pass(ba, c, r2, la); }
                if (nr < total) { rec_fetch_rt(layout, nodes, leaves, nr, ni, b0, b1, bb); hb = scene_box_box_pass(bb, c, r2, lb); }
                if (in_blas) {                                        // triangles at once; at the top level a leaf is an instance, entered like a node
                    u32 pa = INV, pb = INV;                           // the leaf children that passed: their primitives, left first (out of range: never followed)
                    if (ha && nl >= ni) { if (a0 < B.n) pa = a0; ha = false; }
                    if (hb && nr >= ni) { if (b0 < B.n) pb = b0; hb = false; }
                    if (pa == INV) { pa = pb; pb = INV; }
#pragma unroll 1
                    while (pa != INV) {
                        srt_leaf(a, B.bl, pa, inst, x1, x2, x3, xproper, r2, sink);
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
                    if (in_blas) { c = sc_world_box(x1, x2, x3); in_blas = false; ni = tni; total = ttotal; }   // back to the top level: the world box
                    u32 w0, w1; Box b;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, e, tni, w0, w1, b);
                    if (e < tni) { nl = w0; nr = w1; } else { enter = w0; entering = true; }
                }
            }
        }
    }
    if (deep) atomicAdd(a.overflow, 1u);
    if (FILL) { if (deep) sink.out[0].y = QUERY_MARK; }
    else h.offsets[i] = deep ? QUERY_MARK : sink.k;
}

// stackless walk of instance k's BLAS through its plan (srad_walk_blas's structure, scene_radius.hip: the BLAS root's own box is not tested, every other
// record's is)
template <int MODE, bool FILL, bool SORTED>
__device__ void srt_walk_blas(const SceneQuery& a, const SCQuery& t, u32 k, QF3 x1, QF3 x2, QF3 x3, bool xproper, float r2, SceneRadiusTrisSink<FILL, SORTED>& sink) {
    SCBox c; SceneBlas B; u32 bl;
    if (!sc_may_enter<MODE>(a, t, k) || !enter_instance_tris(a, k, x1, x2, x3, c, B, bl)) return;
    const u32 ni = B.n - 1, total = 2 * B.n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    u32 cur = B.root, last = INV;
    bool down = true;
    for (u64 steps = 0; cur < total && steps < bound; ++steps) {
        if (down) {
            u32 w0, w1; Box b; float lb;
            rec_fetch_rt((int)B.layout, B.nodes, B.leaves, cur, ni, w0, w1, b);
            if (cur >= ni) {
                if (scene_box_box_pass(b, c, r2, lb) && w0 < B.n) srt_leaf(a, bl, w0, k, x1, x2, x3, xproper, r2, sink);
                last = cur; cur = B.parent[cur]; down = false;
                continue;
            }
            if (cur != B.root && !scene_box_box_pass(b, c, r2, lb)) { last = cur; cur = B.parent[cur]; down = false; continue; }   // (the BLAS root's own box: as the stack walk, not tested)
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
template <int MODE, bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_radius_tris_deep(SceneQuery a, SCQuery t, SceneHits h) {
    if (*a.overflow == 0u) return;
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 bound = 3ull * ttotal + 3ull;
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < a.n_rays; i += nbid_x() * QUERY_BLOCK) {
        SceneRadiusTrisSink<FILL, SORTED> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = h.offsets[i], end = h.offsets[i + 1];
            if (end <= base) continue;
            uint4* const out = reinterpret_cast<uint4*>(h.hits) + base;
            if (out[0].y != QUERY_MARK) continue;
            sink.out = out; sink.room = end - base;
        } else if (h.offsets[i] != QUERY_MARK) continue;
        QF3 x1{}, x2{}, x3{}; float r2;
        sc_query_load<MODE>(a, t, i, x1, x2, x3, r2);             // (a marked query passed the checks)
        const bool xproper = tt_proper(x1, x2, x3);
        const SCBox world = sc_world_box(x1, x2, x3);
        float lb;
        if (a.n_inst == 1) {
            if (scene_box_box_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), world, r2, lb)) srt_walk_blas<MODE>(a, t, 0, x1, x2, x3, xproper, r2, sink);
        } else {
            u32 cur = a.troot, last = INV;
            bool down = true;
            for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
                if (down) {
                    u32 w0, w1; Box b;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, cur, tni, w0, w1, b);
                    if (cur != a.troot && !scene_box_box_pass(b, world, r2, lb)) { last = cur; cur = a.tparent[cur]; down = false; continue; }   // (the root's own box: as the stack walk, not tested)
                    if (cur >= tni) {                                 // an instance whose world box passes
                        srt_walk_blas<MODE>(a, t, w0, x1, x2, x3, xproper, r2, sink);
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
template <int MODE, bool FILL, bool SORTED> void scene_radius_tris_launch(hipStream_t s, const SceneQuery& q, const SCQuery& t, const SceneHits& h) {
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    { KernelScope ks(s, "k_scene_radius_tris_walk");
      hipLaunchKernelGGL((k_scene_radius_tris_walk<MODE, FILL, SORTED>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, q, t, h); }
    { KernelScope ks(s, "k_scene_radius_tris_deep");              // (the fill's overflow word stays 0 when the fill returned at once)
      hipLaunchKernelGGL((k_scene_radius_tris_deep<MODE, FILL, SORTED>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q, t, h); }
}

template <bool FILL, bool SORTED> void scene_radius_tris_pass(hipStream_t s, float radius, const SceneQuery& q, const SceneHits& h, const SceneTris& st) {
    const TrisMesh& m = st.queries;
    const SCQuery t{ TriSrc{ m.d_tris, (const float*)m.d_vertices, (const u32*)m.d_indices, m.n_vertices }, m.tri_format, st.query_instance, radius };
    if (st.mode == BVH_SCENE_TRIS_INSTANCE) scene_radius_tris_launch<BVH_SCENE_TRIS_INSTANCE, FILL, SORTED>(s, q, t, h);
    else scene_radius_tris_launch<BVH_SCENE_TRIS_QUERY, FILL, SORTED>(s, q, t, h);
}
} // namespace

void launch_scene_radius_tris_count(hipStream_t s, float radius, const SceneQuery& q, const SceneHits& h, const SceneTris& t, uint64_t* d_sums, uint64_t* d_total) {
    scene_radius_tris_pass<false, false>(s, radius, q, h, t);
    launch_overlap_scan(s, h.offsets, q.n_rays, d_sums, d_total);
}

void launch_scene_radius_tris_fill(hipStream_t s, int sorted, float radius, const SceneQuery& q, const SceneHits& h, const SceneTris& t) {
    if (sorted) scene_radius_tris_pass<true, true>(s, radius, q, h, t); else scene_radius_tris_pass<true, false>(s, radius, q, h, t);
}

void warm_scene_radius_tris() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_radius_tris_walk<BVH_SCENE_TRIS_QUERY, false, false>));
}

} // namespace bvh
