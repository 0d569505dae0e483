// scene_radius.hip — bvh_scene_radius_search on gfx950: EVERY triangle within the radius of each query point, over all active instances of a scene (no
// counterpart in the reference).  The two-level point walk is scene_knn.hip's (one query per lane, one LDS short stack shared by both levels, the candidate of
// (instance k, primitive j) is tri_closest on the WORLD triangle, the walk inside an instance runs in object space against the mapped point p' = W_k p with the
// box grown by QUERY_GROW * (its largest |coordinate|) + e and culled iff s2 * lb' * (1 - 2^-20) > bound: DESIGN.md §8n, scene_query.hpp), the count -> scan -> fill scheme is
// radius.hip's and scene_multihit.hip's, and what differs from k_scene_knn is what differs between k_radius_walk and k_knn: the bound never shrinks — the box
// test runs against r2 for the whole walk — so every passing subtree is visited, of two passing children the left one is entered and the right one pushed, and
// the answer is a set of {dist2, prim, instance} records.  DESIGN.md §8q.
//   k_scene_radius_walk : count pass (FILL = false: d_offsets[i] = query i's number of accepted candidates) and fill pass (FILL = true: the records go to the
//                         query's slice).  A query whose push would overflow, or whose walk is longer than its level's node count, is marked and bumps the
//                         pass's overflow word.  Count pass: the mark is the count word (a count saturates at QUERY_MARK - 1, so the mark is never a count).
//                         Fill pass: a query with an empty slice is not walked, so a marked query has a record and the mark is the prim_idx of its slice's
//                         first record.
//   k_scene_radius_deep : launched after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked query from its start,
//                         stackless through the top-level plan and each entered BLAS's plan, left child first.  Both walks test the SAME boxes — every record
//                         below a root, and neither the top-level root's own box nor a BLAS root's own box (the instance's world box stands for it) — so count
//                         and fill agree on a query's set whichever walk served it, and the answer does not depend on QUERY_STACK.
// Fill: a lane writes whole 16-byte records (one uint4) into its own slice and never past it; no atomics.  SORTED: the slice is kept in ascending
// (dist2, instance, prim) order by comparing and shifting whole records from its tail, on scene_knn.hip's u64 key (float_as_uint(dist2) << 32) | instance and
// then the prim: an accepted dist2 is a sum of squares, never negative and never NaN, so that is the contract's lexicographic order.  The insertion is quadratic
// in the slice's length.
// Compiled WITHOUT the SLP vectoriser (Makefile), like scene_knn.hip and scene_multihit.hip: the sorted insertion compares and replaces records.
#include "scene_query.hpp"

namespace bvh {

static_assert(sizeof(bvh_instance_knn_hit) == sizeof(uint4), "a record leaves in one 16-byte store");

// where a walk's records go (radius.hip's RadiusSink for bvh_instance_knn_hit records {dist2 bits, prim, instance, 0})
template <bool FILL, bool SORTED> struct SceneRadiusSink {
    uint4* out; u32 room, k = 0;
    __device__ __forceinline__ void put(float d2, u32 prim, u32 inst) {
        if (FILL) {
            if (k < room) {
                u32 j = k;
                const u32 db = __float_as_uint(d2);
                if (SORTED) {
                    const u64 key = ((u64)db << 32) | inst;
                    while (j > 0) {                               // (records above (dist2, inst, prim) move up by one; the slice below j + 1 stays sorted)
                        const uint4 p = out[j - 1];
                        const u64 pk = ((u64)p.x << 32) | p.z;
                        if (pk < key || (pk == key && p.y < prim)) break;
                        out[j] = p; --j;
                    }
                }
                out[j] = make_uint4(db, prim, inst, 0u);
            }
        }
        if (k < QUERY_MARK - 1u) ++k;                             // (many instances of one BLAS can answer: the counter saturates below the mark)
    }
};

// the candidate of (inst, prim): the world triangle's squared distance to the world point w, accepted iff dist2 <= r2 (a NaN dist2 fails).  The forward
// matrix is re-loaded per leaf test (blas_world_tri): it never lives across the walk
template <bool FILL, bool SORTED>
__device__ __forceinline__ void srad_leaf(const SceneQuery& a, const SceneBlas& B, u32 prim, u32 inst, QF3 w, float r2, SceneRadiusSink<FILL, SORTED>& sink) {
    if (prim >= B.n) return;
    QF3 wa, wb, wc;
    blas_world_tri(a, B, prim, inst, wa, wb, wc);
    QF3 q; float u, v;
    const float d2 = tri_closest(wa, wb, wc, w, q, u, v);
    if (d2 <= r2) sink.put(d2, prim, inst);
}

template <bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_radius_walk(SceneQuery a, SceneHits h) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 t = *h.total; if (t > h.capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= a.n_rays) return;
    SceneRadiusSink<FILL, SORTED> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = h.offsets[i], end = h.offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = reinterpret_cast<uint4*>(h.hits) + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    QF3 w{ 0.0f, 0.0f, 0.0f }; float r2 = 0.0f;
    const bool live = point_load(reinterpret_cast<const bvh_point_query*>(a.rays), i, w, r2);
    bool deep = false;
    if (live) {                                                   // (a NaN coordinate, a NaN or negative radius: accepts nothing)
        const ScenePoint world{ w, 0.0f, 1.0f };
        ScenePoint c = world;
        SceneBlas B{};
        const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
        u32 ni = tni, total = ttotal;                                 // of the level the query is on
        bool in_blas = false, pop = false, entering = false;         // entering: instance `enter` is entered at the top of the next step
        u32 inst = INV, enter = INV;
        u32 nl = INV, nr = INV, top = 0, tsteps = 0, bsteps = 0;
        if (a.n_inst == 1) {                                          // no top-level tree: the instance's world box, then the instance
            if (scene_box_dist_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), world, r2)) { enter = 0; entering = true; } else pop = true;
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
                bool ha = false, hb = false;
                if (nl < total) { rec_fetch_rt(layout, nodes, leaves, nl, ni, a0, a1, ba); ha = scene_box_dist_pass(ba, c, r2); }
                if (nr < total) { rec_fetch_rt(layout, nodes, leaves, nr, ni, b0, b1, bb); hb = scene_box_dist_pass(bb, c, r2); }
                if (in_blas) {                                        // triangles at once; at the top level a leaf is an instance, entered like a node
                    if (ha && nl >= ni) { srad_leaf(a, B, a0, inst, w, r2, sink); ha = false; }
                    if (hb && nr >= ni) { srad_leaf(a, B, b0, inst, w, r2, sink); hb = false; }
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
                    if (in_blas) { c = world; in_blas = false; ni = tni; total = ttotal; }   // back to the top level: the world point
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

// stackless walk of instance k's BLAS through its plan (sknn_walk_blas's arithmetic with the tests where k_scene_hits_deep has them: the BLAS root's own box
// is not tested, every other record's is)
template <bool FILL, bool SORTED>
__device__ void srad_walk_blas(const SceneQuery& a, u32 k, QF3 w, float r2, SceneRadiusSink<FILL, SORTED>& sink) {
    ScenePoint c; SceneBlas B;
    if (k >= a.n_inst || !enter_instance_point(a, k, w, c, B)) return;
    const u32 ni = B.n - 1, total = 2 * B.n - 1;
    const u64 bound = 3ull * total + 3ull;
    u32 cur = B.root, last = INV;
    bool down = true;
    for (u64 steps = 0; cur < total && steps < bound; ++steps) {
        if (down) {
            u32 w0, w1; Box b;
            rec_fetch_rt((int)B.layout, B.nodes, B.leaves, cur, ni, w0, w1, b);
            if (cur >= ni) {
                if (scene_box_dist_pass(b, c, r2)) srad_leaf(a, B, w0, k, w, r2, sink);
                last = cur; cur = B.parent[cur]; down = false;
                continue;
            }
            if (cur != B.root && !scene_box_dist_pass(b, c, r2)) { last = cur; cur = B.parent[cur]; down = false; continue; }   // (the BLAS root's own box: as the stack walk, not tested)
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
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_radius_deep(SceneQuery a, SceneHits h) {
    if (*a.overflow == 0u) return;
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 bound = 3ull * ttotal + 3ull;
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < a.n_rays; i += nbid_x() * QUERY_BLOCK) {
        SceneRadiusSink<FILL, SORTED> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = h.offsets[i], end = h.offsets[i + 1];
            if (end <= base) continue;
            uint4* const out = reinterpret_cast<uint4*>(h.hits) + base;
            if (out[0].y != QUERY_MARK) continue;
            sink.out = out; sink.room = end - base;
        } else if (h.offsets[i] != QUERY_MARK) continue;
        QF3 w; float r2;
        point_load(reinterpret_cast<const bvh_point_query*>(a.rays), i, w, r2);   // (a marked query passed the checks)
        const ScenePoint world{ w, 0.0f, 1.0f };
        if (a.n_inst == 1) {
            if (scene_box_dist_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), world, r2)) srad_walk_blas(a, 0, w, r2, sink);
        } else {
            u32 cur = a.troot, last = INV;
            bool down = true;
            for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
                if (down) {
                    u32 w0, w1; Box b;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, cur, tni, w0, w1, b);
                    if (cur != a.troot && !scene_box_dist_pass(b, world, r2)) { last = cur; cur = a.tparent[cur]; down = false; continue; }   // (the root's own box: as the stack walk, not tested)
                    if (cur >= tni) {                                 // an instance whose world box passes
                        srad_walk_blas(a, w0, w, r2, sink);
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
template <bool FILL, bool SORTED> void scene_radius_pass(hipStream_t s, const SceneQuery& q, const SceneHits& h) {
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    { KernelScope ks(s, FILL ? "k_scene_radius_fill" : "k_scene_radius_count");
      hipLaunchKernelGGL((k_scene_radius_walk<FILL, SORTED>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, q, h); }
    { KernelScope ks(s, "k_scene_radius_deep");                   // (the fill's overflow word stays 0 when the fill returned at once)
      hipLaunchKernelGGL((k_scene_radius_deep<FILL, SORTED>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q, h); }
}
} // namespace

void launch_scene_radius_count(hipStream_t s, const SceneQuery& q, const SceneHits& h, uint64_t* d_sums, uint64_t* d_total) {
    scene_radius_pass<false, false>(s, q, h);
    launch_overlap_scan(s, h.offsets, q.n_rays, d_sums, d_total);
}

void launch_scene_radius_fill(hipStream_t s, int sorted, const SceneQuery& q, const SceneHits& h) {
    if (sorted) scene_radius_pass<true, true>(s, q, h); else scene_radius_pass<true, false>(s, q, h);
}

void warm_scene_radius() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_radius_walk<false, false>)); }

} // namespace bvh
