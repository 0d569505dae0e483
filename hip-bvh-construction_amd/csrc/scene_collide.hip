// scene_collide.hip — bvh_scene_collide on gfx950: the crossing triangle pairs of ALL instances of a scene in one call (no counterpart in the reference).
// bvh_scene_intersect_tris's INSTANCE mode (scene_tris.hip) asked for every instance at once: the rows are the triangles of all active instances in instance
// order, and the table that says which rows belong to which instance is made on the device from the scene's own instance array, so the host never needs to
// know which BLAS an instance places.
//   k_scene_collide_rows : one thread per instance writes n_leaves of the instance's BLAS (0: inactive) — the active flag and the BLAS index read as
//                          sov_enter_instance reads them — and launch_overlap_scan turns the counts into row_first[n_inst + 1]; its u64 total is n_rows, in a
//                          scratch word of its own (the count pass's scan writes the query total into another).
//   row r                : r >= n_rows: empty.  Otherwise (k, i) with row_first[k] <= r < row_first[k + 1], found by a binary search of row_first —
//                          consecutive lanes are almost always in the same instance, so the loads are uniform and cached — and the query triangle is the
//                          world triangle (k, i), st_world_tri's (scene_map.hpp), as BVH_SCENE_TRIS_INSTANCE defines it.
//   may the walk enter l : l > k, or with BVH_SCENE_COLLIDE_BOTH l != k (a run-time scalar, not a template parameter); k is a per-lane value here.
//   k_scene_collide_walk : k_scene_tris_walk's control flow (one row per lane, 64-lane workgroups, the shared LDS short stack, left child entered and right
//                          child pushed, the mapped box of every record below a BLAS root, the f64 predicate at the leaf); the grid covers row_capacity rows;
//                          the whole launch answers "no records" when n_rows > row_capacity.
//   k_scene_collide_deep : after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked row from its start, stackless
//                          through the top-level plan and each entered BLAS's plan.  Both walks test the SAME boxes and the same triangles.
// Exactness is §8u's on every row; the box test removes no crossing pair in either direction and crosses() is symmetric, so the default answer
// is the BOTH answer filtered to instance > k.
// Compiled WITHOUT the SLP vectoriser (Makefile), like scene_tris.hip.
#include "query.hpp"
#include "tri_cross.hpp"
#include "scene_map.hpp"
#include "kernels.hpp"

namespace bvh {

// the row table of a launch: row_first[n_inst + 1] and n_rows as k_scene_collide_rows and the scan left them, and BVH_SCENE_COLLIDE_BOTH
struct SCRows { const u32* row_first; const u64* n_rows; u32 both; };

__global__ __launch_bounds__(256) void k_scene_collide_rows(SceneQuery a, u32* __restrict__ row_first) {
    const u32 k = bid_x() * 256u + tid_x();
    if (k >= a.n_inst) return;
    const u32 bl = __float_as_uint(reinterpret_cast<const float4*>(a.inst + k)[3].x);
    row_first[k] = bl == INV ? 0u : a.blas[bl].n;
}

// the instance of row r (< n_rows = row_first[n_inst]): the k with row_first[k] <= r < row_first[k + 1]; instances without rows are stepped over
__device__ __forceinline__ u32 sc_instance_of(const u32* __restrict__ row_first, u32 n_inst, u32 r) {
    u32 lo = 0, hi = n_inst - 1;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (row_first[mid + 1] <= r) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// row r's query triangle and its instance; false: never for r < n_rows (an instance with rows is active and r - row_first[k] < its n_leaves)
__device__ __forceinline__ bool sc_query(const SceneQuery& a, const SCRows& t, u32 r, u32& own, QF3& x1, QF3& x2, QF3& x3) {
    own = sc_instance_of(t.row_first, a.n_inst, r);
    const u32 i = r - t.row_first[own];
    SOMat M; SceneBlas B;
    if (!sov_enter_instance(a, own, M, B) || i >= B.n) return false;
    st_world_tri(B, M, i, x1, x2, x3);
    return true;
}

// may the walk of a row of instance own enter instance l?  (by index: a second instance of the same BLAS is another instance)
__device__ __forceinline__ bool sc_may_enter(const SceneQuery& a, const SCRows& t, u32 own, u32 l) {
    return l < a.n_inst && (t.both ? l != own : l > own);
}

template <bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_collide_walk(SceneQuery a, SceneHits h, SCRows t) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 tot = *h.total; if (tot > h.capacity || tot > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 r = bid_x() * QUERY_BLOCK + tid_x();
    if (r >= a.n_rays) return;
    const u64 n_rows = *t.n_rows;
    if (n_rows > (u64)a.n_rays || (u64)r >= n_rows) {             // too many rows for row_capacity (uniform: nothing is walked), or a row behind the last one
        if (!FILL) h.offsets[r] = 0u;
        return;
    }
    SceneOverlapSink<FILL, SORTED> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = h.offsets[r], end = h.offsets[r + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = reinterpret_cast<uint2*>(h.hits) + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    QF3 x1{}, x2{}, x3{};
    u32 own = INV;
    const bool asked = sc_query(a, t, r, own, x1, x2, x3);
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
        if (a.n_inst == 1) pop = true;                                // no top-level tree and nobody else to cross
        else { const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(a.tnodes) + a.troot); nl = lr.x; nr = lr.y; }
        for (;;) {
            if (entering) {
                entering = false;
                const u32 l = enter;
                if (sc_may_enter(a, t, own, l) && sov_enter_instance(a, l, M, B)) {
                    in_blas = true; inst = l; ni = B.n - 1; total = 2 * B.n - 1; bsteps = 0;
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
    else h.offsets[r] = deep ? QUERY_MARK : sink.k;
}

// stackless walk of instance l's BLAS through its plan (st_walk_blas's arithmetic: the BLAS root's own box is not tested, every other record's is)
template <bool FILL, bool SORTED>
__device__ void sc_walk_blas(const SceneQuery& a, const SCRows& t, u32 own, u32 l, const Box& q, QF3 x1, QF3 x2, QF3 x3, SceneOverlapSink<FILL, SORTED>& sink) {
    SOMat M; SceneBlas B;
    if (!sc_may_enter(a, t, own, l) || !sov_enter_instance(a, l, M, B)) return;
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
                    if (tt_proper(y1, y2, y3) && tt_crosses(x1, x2, x3, y1, y2, y3)) sink.put(w0, l);
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

// the stackless re-walk of the marked rows: the top-level plan, and for every instance whose world box passes, that BLAS's plan; left child first
template <bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_collide_deep(SceneQuery a, SceneHits h, SCRows t) {
    if (*a.overflow == 0u) return;
    if (a.n_inst == 1) return;                                    // (never: one instance has nobody to cross, so nothing was marked)
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 bound = 3ull * ttotal + 3ull;
    for (u32 r = bid_x() * QUERY_BLOCK + tid_x(); r < a.n_rays; r += nbid_x() * QUERY_BLOCK) {
        SceneOverlapSink<FILL, SORTED> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = h.offsets[r], end = h.offsets[r + 1];
            if (end <= base) continue;
            uint2* const out = reinterpret_cast<uint2*>(h.hits) + base;
            if (out[0].x != QUERY_MARK) continue;
            sink.out = out; sink.room = end - base;
        } else if (h.offsets[r] != QUERY_MARK) continue;
        QF3 x1{}, x2{}, x3{};
        u32 own = INV;
        if ((u64)r >= *t.n_rows || !sc_query(a, t, r, own, x1, x2, x3)) continue;   // (never: a marked row was asked, and passed box_valid and tt_proper)
        const Box q = tt_box(x1, x2, x3);
        u32 cur = a.troot, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
            if (down) {
                u32 w0, w1; Box b;
                rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, cur, tni, w0, w1, b);
                if (cur != a.troot && !box_overlap(q, b)) { last = cur; cur = a.tparent[cur]; down = false; continue; }   // (the root's own box: as the stack walk, not tested)
                if (cur >= tni) {                                 // an instance whose world box passes
                    sc_walk_blas<FILL, SORTED>(a, t, own, w0, q, x1, x2, x3, sink);
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
        if (!FILL) h.offsets[r] = sink.k;
    }
}

namespace {
template <bool FILL, bool SORTED> void scene_collide_pass(hipStream_t s, const SceneQuery& q, const SceneHits& h, const SceneCollide& c) {
    const SCRows t{ c.d_row_first, c.d_n_rows, c.both ? 1u : 0u };
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    { KernelScope ks(s, FILL ? "k_scene_collide_fill" : "k_scene_collide_count");
      hipLaunchKernelGGL((k_scene_collide_walk<FILL, SORTED>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, q, h, t); }
    { KernelScope ks(s, "k_scene_collide_deep");                  // (the fill's overflow word stays 0 when the fill returned at once)
      hipLaunchKernelGGL((k_scene_collide_deep<FILL, SORTED>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q, h, t); }
}
} // namespace

void launch_scene_collide_rows(hipStream_t s, const SceneQuery& q, const SceneCollide& c, uint64_t* d_sums) {
    { KernelScope ks(s, "k_scene_collide_rows");
      hipLaunchKernelGGL(k_scene_collide_rows, dim3((q.n_inst + 255u) / 256u), dim3(256), 0, s, q, c.d_row_first); }
    launch_overlap_scan(s, c.d_row_first, q.n_inst, d_sums, c.d_n_rows);
}

void launch_scene_collide_count(hipStream_t s, const SceneQuery& q, const SceneHits& h, const SceneCollide& c, uint64_t* d_sums, uint64_t* d_total) {
    scene_collide_pass<false, false>(s, q, h, c);
    launch_overlap_scan(s, h.offsets, q.n_rays, d_sums, d_total);
}

void launch_scene_collide_fill(hipStream_t s, int sorted, const SceneQuery& q, const SceneHits& h, const SceneCollide& c) {
    if (sorted) scene_collide_pass<true, true>(s, q, h, c); else scene_collide_pass<true, false>(s, q, h, c);
}

void warm_scene_collide() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_collide_walk<false, false>));
}

} // namespace bvh
