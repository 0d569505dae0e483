// radius_tris.hip — bvh_radius_tris on gfx950: EVERY triangle of a built BVH2 within a distance of each triangle of another mesh (or of the tree's own mesh:
// BVH_RADIUS_TRIS_SELF), with its squared distance and feature pair (no counterpart in the reference).  The answer has a variable length, so the call is
// count -> scan -> fill as in radius.hip; count and fill are the SAME walk, templated on node layout, the TREE's triangle format, pass and order.  The query
// mesh's format is switched at run time (one fetch per lane, outside the loop), and so are the two self-mode rules (a kernel argument, uniform over the launch:
// two comparisons per leaf, not worth three times the kernels).  The candidate is bvh_closest_tris's (tt_dist2, closest_tris.hpp: not copied, not altered) and so
// is the box test (box_box_dist_pass on grown boxes, query.hpp); what differs from k_closest_tris is that the bound never shrinks — the test runs against r2 for
// the whole walk — so every passing subtree is visited and the answer is a set of {dist2, prim, feature, 0} records.
//   k_radius_tris_walk : one query triangle per lane, short per-lane stack in LDS (QUERY_STACK entries, query.hip's layout).  Per internal node both children's
//                        records are fetched and box-tested; leaf children that pass are tested at once — both through ONE copy of the leaf routine (a two-trip
//                        loop that is not unrolled, as in k_closest_tris: the routine is six point-triangle and nine segment-segment terms and, where the boxes
//                        overlap, up to 24 f64 determinants); of two passing internal children the left one is entered and the right one pushed, as
//                        k_radius_walk does (every passing subtree must be visited: near-first ordering buys nothing).  A query whose push would overflow (or
//                        whose walk exceeds the node count: arrays that are not a tree) is marked and bumps the pass's overflow word.  Count pass: the mark is
//                        the count word (QUERY_MARK is never a count: n < 2^30).  Fill pass: a query with an empty slice is not walked at all, so a marked query
//                        has a record and the mark is the prim_idx of its slice's first record (QUERY_MARK is never a primitive).
//   k_radius_tris_deep : launched after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked query from its start,
//                        stackless through the parent links of bvh_refit's plan (k_refit_plan), left child first.  Correct at any depth.  Both walks report
//                        exactly the accepted candidates of the leaves whose own box and every box above them (the root's excepted: neither walk tests it)
//                        pass, so count and fill agree whichever walk served a query.
// The leaf: primitive in range and, in self mode, above the query's own index (every unordered pair once); the pair's own two stage-E boxes against r2 before
// any term; BVH_RADIUS_TRIS_SKIP_SHARED's nine vertex comparisons (IEEE ==, so -0 equals +0 and a NaN equals nothing) before any term; then tt_dist2 and the
// acceptance dist2 <= r2 (a NaN dist2 fails).  Identical in count and fill.
// Fill: a lane writes whole 16-byte records into its own slice [d_offsets[i], d_offsets[i+1]) with vector stores and never past it; no atomics.  SORTED: the lane
// keeps the slice in ascending (dist2, prim) order as it goes, inserting each record by comparing and shifting whole records from the slice's tail (its own
// earlier stores, read back by the same lane) on radius.hip's u64 key (float_as_uint(dist2) << 32) | prim: an accepted dist2 is 0 or a sum of squares, never
// negative and never NaN, so the u64 order is the contract's lexicographic order.  The insertion is quadratic in the slice's length.
// The scan of the counts and the total word are bvh_overlap's (launch_overlap_scan, overlap.hip).  The fill decides ON THE DEVICE whether it runs.
// Built WITHOUT the SLP vectoriser (Makefile), like closest_tris.hip (the 15 terms are stated operation for operation) and radius.hip (the sorted insertion
// compares and replaces records).
#include <type_traits>
#include "query.hpp"
#include "tri_cross.hpp"
#include "closest_tris.hpp"
#include "kernels.hpp"

namespace bvh {

// where a walk's records go.  Count pass: a counter.  Fill pass: the query's slice [out, out + room) of d_hits as {dist2 bits, prim, feature, 0} words, never
// written past its end (a walk of arrays that are not a tree may find more than the count pass did only if the arrays changed in between; the bound keeps that
// in the slice)
template <bool FILL, bool SORTED> struct RadiusTrisSink {
    uint4* out; u32 room, k = 0;
    __device__ __forceinline__ void put(float d2, u32 prim, u32 feat) {
        if (FILL) {
            if (k < room) {
                u32 j = k;
                const u32 db = __float_as_uint(d2);
                if (SORTED) {
                    const u64 key = ((u64)db << 32) | prim;
                    while (j > 0) {                               // (records above the key move up by one; the slice below j + 1 stays sorted)
                        const uint4 p = out[j - 1];
                        if (!((((u64)p.x << 32) | p.y) > key)) break;
                        out[j] = p; --j;
                    }
                }
                out[j] = make_uint4(db, prim, feat, 0u);
            }
        }
        ++k;
    }
};

// a leaf child's primitive: in range (never followed otherwise) and, in self mode, above the query's own index (every unordered pair once)
__device__ __forceinline__ bool rt_prim_ok(u32 prim, u32 n, u32 i, u32 flags) { return prim < n && (!(flags & BVH_RADIUS_TRIS_SELF) || prim > i); }

// BVH_RADIUS_TRIS_SKIP_SHARED: does vertex p equal one of a, b, c on all three coordinates under IEEE == (-0 equals +0, a NaN equals nothing)
__device__ __forceinline__ bool rt_same(QF3 p, QF3 q) { return p.x == q.x && p.y == q.y && p.z == q.z; }
__device__ __forceinline__ bool rt_vertex_of(QF3 p, QF3 a, QF3 b, QF3 c) { return rt_same(p, a) || rt_same(p, b) || rt_same(p, c); }

// the candidate of prim and its acceptance dist2 <= r2 (a NaN dist2 fails).  xg: the query's grown box (box_grown(xb))
template <int TFMT, bool FILL, bool SORTED>
__device__ __forceinline__ void radius_tris_leaf(const TriSrc& tsrc, u32 prim, QF3 x1, QF3 x2, QF3 x3, bool xproper, const Box& xb, const Box& xg, float r2, u32 flags,
                                                 RadiusTrisSink<FILL, SORTED>& sink) {
    QF3 y1, y2, y3; tri_fetch<TFMT>(tsrc, prim, y1, y2, y3);
    const Box yb = tt_box(y1, y2, y3);
    float lb;
    if (!box_box_dist_pass(yb, xg, r2, lb)) return;               // the pair's own boxes are already too far apart
    if ((flags & BVH_RADIUS_TRIS_SKIP_SHARED) && (rt_vertex_of(x1, y1, y2, y3) || rt_vertex_of(x2, y1, y2, y3) || rt_vertex_of(x3, y1, y2, y3))) return;
    u32 feat;
    const float d2 = tt_dist2(x1, x2, x3, xproper, xb, y1, y2, y3, yb, feat);
    if (d2 <= r2) sink.put(d2, prim, feat);
}

template <int LAYOUT, int TFMT, bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_radius_tris_walk(TriSrc qsrc, int qfmt, u32 n_queries, float radius, u32 flags, const bvh2_node* __restrict__ nodes,
                                                                  const bvh_primref* __restrict__ leaves, TriSrc tsrc, u32 n, u32 root, u32* __restrict__ offsets,
                                                                  uint4* hits, const u64* __restrict__ total_word, u64 capacity, u32* __restrict__ overflow) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 t = *total_word; if (t > capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= n_queries) return;
    RadiusTrisSink<FILL, SORTED> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = offsets[i], end = offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = hits + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    QF3 x1, x2, x3; float r2;
    const bool live = tris_query_load(qfmt, qsrc, i, radius, x1, x2, x3, r2);
    bool deep = false;
    if (live) {                                                   // (a NaN coordinate, a NaN or negative radius: accepts nothing)
        const Box xb = tt_box(x1, x2, x3), xg = box_grown(xb);
        const bool xproper = tt_proper(x1, x2, x3);
        const u32 ni = n - 1, total = 2 * n - 1;
        u32 nl, nr; { const uint2 lr = *reinterpret_cast<const uint2*>(nodes + root); nl = lr.x; nr = lr.y; }
        u32 top = 0, steps = 0;
        for (;;) {
            if (++steps > n) { deep = true; break; }              // more expansions than internal nodes: not a tree (a tree never gets here)
            u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
            Box ba, bb;
            float la, lb;
            bool ha = false, hb = false;
            if (nl < total) { rec_fetch<LAYOUT>(nodes, leaves, nl, ni, a0, a1, ba); ha = box_box_dist_pass(ba, xg, r2, la); }
            if (nr < total) { rec_fetch<LAYOUT>(nodes, leaves, nr, ni, b0, b1, bb); hb = box_box_dist_pass(bb, xg, r2, lb); }
            u32 pa = INV, pb = INV;                               // the leaf children that passed: their primitives, left first
            if (ha && nl >= ni) { if (rt_prim_ok(a0, n, i, flags)) pa = a0; ha = false; }
            if (hb && nr >= ni) { if (rt_prim_ok(b0, n, i, flags)) pb = b0; hb = false; }
            if (pa == INV) { pa = pb; pb = INV; }
#pragma unroll 1
            while (pa != INV) {
                radius_tris_leaf<TFMT>(tsrc, pa, x1, x2, x3, xproper, xb, xg, r2, flags, sink);
                pa = pb; pb = INV;
            }
            if (ha || hb) {
                if (ha && hb) {
                    if (top == (u32)QUERY_STACK) { deep = true; break; }
                    stack[top * QUERY_BLOCK] = nr; ++top;
                }
                nl = ha ? a0 : b0; nr = ha ? a1 : b1;             // (selects of values, not branches to them: overlap.hip)
            } else {
                if (top == 0) break;
                const u32 node = stack[--top * QUERY_BLOCK];
                const uint2 lr = *reinterpret_cast<const uint2*>(nodes + node);
                nl = lr.x; nr = lr.y;
            }
        }
    }
    if (deep) atomicAdd(overflow, 1u);
    if (FILL) { if (deep) sink.out[0].y = QUERY_MARK; }
    else offsets[i] = deep ? QUERY_MARK : sink.k;
}

// the stackless re-walk of the marked queries: parent links of the plan, left child first
template <int LAYOUT, int TFMT, bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_radius_tris_deep(TriSrc qsrc, int qfmt, u32 n_queries, float radius, u32 flags, const bvh2_node* __restrict__ nodes,
                                                                  const bvh_primref* __restrict__ leaves, TriSrc tsrc, u32 n, u32 root, u32* __restrict__ offsets,
                                                                  uint4* hits, const u32* __restrict__ overflow, const u32* __restrict__ parent) {
    if (*overflow == 0u) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < n_queries; i += nbid_x() * QUERY_BLOCK) {
        RadiusTrisSink<FILL, SORTED> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = offsets[i], end = offsets[i + 1];
            if (end <= base || hits[base].y != QUERY_MARK) continue;
            sink.out = hits + base; sink.room = end - base;
        } else if (offsets[i] != QUERY_MARK) continue;
        QF3 x1, x2, x3; float r2;
        tris_query_load(qfmt, qsrc, i, radius, x1, x2, x3, r2);   // (a marked query passed the checks)
        const Box xb = tt_box(x1, x2, x3), xg = box_grown(xb);
        const bool xproper = tt_proper(x1, x2, x3);
        u32 cur = root, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < total && steps < bound; ++steps) {
            if (down) {
                u32 w0, w1; Box b; float lb;
                rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                if (cur >= ni) {
                    if (box_box_dist_pass(b, xg, r2, lb) && rt_prim_ok(w0, n, i, flags))
                        radius_tris_leaf<TFMT>(tsrc, w0, x1, x2, x3, xproper, xb, xg, r2, flags, sink);
                    last = cur; cur = parent[cur]; down = false;
                    continue;
                }
                if (cur != root && !box_box_dist_pass(b, xg, r2, lb)) { last = cur; cur = parent[cur]; down = false; continue; }   // (the root's own box: as k_radius_tris_walk, not tested)
                if (w0 < total) { cur = w0; continue; }
                last = w0; down = false;                          // (a left link out of range: as if its subtree were done)
                continue;
            }
            if (cur >= ni) break;                                 // (parent links are internal nodes or INVALID)
            const uint2 lr = *reinterpret_cast<const uint2*>(nodes + cur);
            if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
            last = cur; cur = parent[cur];
        }
        if (!FILL) offsets[i] = sink.k;
    }
}

namespace {
struct RadiusTrisArgs {
    hipStream_t s; TriSrc qsrc; int qfmt; u32 n_queries; float radius; u32 flags; const bvh2_node* nodes; const bvh_primref* leaves; TriSrc tsrc; u32 n, root;
    u32* offsets; uint4* hits; const u64* total; u64 capacity; u32* overflow; const u32* parent;
};

template <bool FILL, bool SORTED> void radius_tris_pass(const RadiusTrisArgs& a, int layout, int tri_format) {
    const u32 blocks = (a.n_queries + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    auto go = [&](auto L, auto F) {
        constexpr int LA = decltype(L)::value, FM = decltype(F)::value;
        { KernelScope ks(a.s, "k_radius_tris_walk");
          hipLaunchKernelGGL((k_radius_tris_walk<LA, FM, FILL, SORTED>), dim3(blocks), dim3(QUERY_BLOCK), 0, a.s, a.qsrc, a.qfmt, a.n_queries, a.radius, a.flags, a.nodes,
                             a.leaves, a.tsrc, a.n, a.root, a.offsets, a.hits, a.total, a.capacity, a.overflow); }
        { KernelScope ks(a.s, "k_radius_tris_deep");              // (the fill's overflow word stays 0 when the fill returned at once)
          hipLaunchKernelGGL((k_radius_tris_deep<LA, FM, FILL, SORTED>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, a.s, a.qsrc, a.qfmt, a.n_queries, a.radius, a.flags,
                             a.nodes, a.leaves, a.tsrc, a.n, a.root, a.offsets, a.hits, (const u32*)a.overflow, a.parent); }
    };
    auto by_fmt = [&](auto L) {
        switch (tri_format) {
            case BVH_TRI_PADDED64: go(L, std::integral_constant<int, BVH_TRI_PADDED64>{}); break;
            case BVH_TRI_PACKED36: go(L, std::integral_constant<int, BVH_TRI_PACKED36>{}); break;
            default:               go(L, std::integral_constant<int, BVH_TRI_INDEXED>{}); break;
        }
    };
    if (layout == 0) by_fmt(std::integral_constant<int, 0>{}); else by_fmt(std::integral_constant<int, 1>{});
}

TriSrc tri_src(const TrisMesh& m) { return TriSrc{ m.d_tris, (const float*)m.d_vertices, (const u32*)m.d_indices, m.n_vertices }; }
} // namespace

static_assert(sizeof(bvh_tri_hit) == sizeof(uint4), "a record is four words: dist2's bits, prim_idx, feature, reserved");

void launch_radius_tris_count(hipStream_t s, int layout, uint32_t flags, const TrisMesh& tree_tris, const TrisMesh& queries, uint32_t n_queries, float radius,
                              const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, uint32_t* d_overflow,
                              const uint32_t* d_parent, uint64_t* d_sums, uint64_t* d_total) {
    const RadiusTrisArgs a{ s, tri_src(queries), queries.tri_format, n_queries, radius, flags, (const bvh2_node*)d_nodes, (const bvh_primref*)d_leaves,
                            tri_src(tree_tris), n, root, d_offsets, nullptr, nullptr, 0, d_overflow, d_parent };
    radius_tris_pass<false, false>(a, layout, tree_tris.tri_format);
    launch_overlap_scan(s, d_offsets, n_queries, d_sums, d_total);
}

void launch_radius_tris_fill(hipStream_t s, int layout, uint32_t flags, const TrisMesh& tree_tris, const TrisMesh& queries, uint32_t n_queries, float radius,
                             const void* d_nodes, const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, void* d_hits, uint64_t capacity,
                             const uint64_t* d_total, uint32_t* d_overflow, const uint32_t* d_parent) {
    const RadiusTrisArgs a{ s, tri_src(queries), queries.tri_format, n_queries, radius, flags, (const bvh2_node*)d_nodes, (const bvh_primref*)d_leaves,
                            tri_src(tree_tris), n, root, d_offsets, (uint4*)d_hits, d_total, capacity, d_overflow, d_parent };
    if (flags & BVH_RADIUS_TRIS_SORTED) radius_tris_pass<true, true>(a, layout, tree_tris.tri_format);
    else radius_tris_pass<true, false>(a, layout, tree_tris.tri_format);
}

void warm_radius_tris() {
    hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_radius_tris_walk<0, BVH_TRI_PADDED64, false, false>));
}

} // namespace bvh
