// scene_multihit.hip — bvh_scene_intersect_all on gfx950: EVERY accepted hit along each ray over all active instances of a scene (no counterpart in the
// reference).  The two-level walk is scene.hip's (one ray per lane, one LDS short stack shared by both levels, the BLAS's layout and format dispatched at run
// time from its descriptor, entered through scene_query.hpp's enter_instance_ray), the count -> scan -> fill scheme is multihit.hip's, and the differences from k_scene_intersect are those between k_hits_walk and
// k_intersect: box_pass runs against the ray's tmax for the whole walk, a passing BLAS leaf child is hit-tested at once and handed to the sink, and of two
// passing children the left one is entered and the right one pushed.  DESIGN.md §8o.
//   k_scene_hits_walk : count pass (FILL = false: d_offsets[i] = ray i's number of accepted hits) and fill pass (FILL = true: the records go to the ray's slice).
//                       A ray whose push would overflow, or whose walk is longer than its level's node count, is marked and bumps the pass's overflow word.
//                       Count pass: the mark is the count word (a count saturates at QUERY_MARK - 1, so the mark is never a count).  Fill pass: a ray with an
//                       empty slice is not walked, so a marked ray has a record and the mark is the prim_idx of its slice's first record.
//   k_scene_hits_deep : launched after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked ray from its start,
//                       stackless through the top-level plan and each entered BLAS's plan, left child first.  Both walks test the SAME boxes — every record
//                       below a root, and neither the top-level root's own box nor a BLAS root's own box (the instance's world box stands for it) — so count
//                       and fill agree on a ray's set whichever walk served it, and the answer does not depend on QUERY_STACK.
// Fill: a lane writes whole 32-byte records (two float4) into its own slice and never past it; no atomics.  SORTED: the slice is kept in ascending
// (t, instance, prim) order by comparing and shifting whole records from its tail; inside one instance the earlier hits of that instance are already there and
// across instances the keys interleave, so the instance index takes part in the comparison.
// Compiled WITHOUT the SLP vectoriser (Makefile), like scene.hip and multihit.hip: the sorted insertion compares and replaces records.
#include "scene_query.hpp"

namespace bvh {

// where a walk's hits go (multihit.hip's HitSink for bvh_instance_hit records): record j of the slice is out[2j], out[2j + 1]
template <bool FILL, bool SORTED> struct SceneHitSink {
    float4* out; u32 room, k = 0;
    __device__ __forceinline__ void put(float it, float iu, float iv, u32 prim, u32 inst) {
        if (FILL) {
            if (k < room) {
                u32 j = k;
                if (SORTED) {
                    while (j > 0) {                               // (records above (it, inst, prim) move up by one; the slice below j + 1 stays sorted)
                        const float4 p = out[2 * (size_t)(j - 1)];
                        const u32 pi = reinterpret_cast<const u32*>(out + 2 * (size_t)(j - 1) + 1)[0], pp = __float_as_uint(p.w);
                        if (!(p.x > it || (p.x == it && (pi > inst || (pi == inst && pp > prim))))) break;
                        out[2 * (size_t)j] = p; out[2 * (size_t)j + 1] = make_float4(__uint_as_float(pi), 0.0f, 0.0f, 0.0f); --j;
                    }
                }
                out[2 * (size_t)j] = make_float4(it, iu, iv, __uint_as_float(prim));
                out[2 * (size_t)j + 1] = make_float4(__uint_as_float(inst), 0.0f, 0.0f, 0.0f);
            }
        }
        if (k < QUERY_MARK - 1u) ++k;                             // (a scene ray can cross many instances of one BLAS: the counter saturates below the mark)
    }
};

// the candidate prim's test with the BLAS's format chosen at run time: in range (never followed otherwise) and an accepted hit
template <bool FILL, bool SORTED>
__device__ __forceinline__ void scene_hit_leaf(const SceneBlas& B, u32 prim, u32 inst, const QRay& r, SceneHitSink<FILL, SORTED>& sink) {
    if (prim >= B.n) return;
    QF3 a, b, c;
    blas_tri_fetch(B, prim, a, b, c);
    float it = 0.0f, iu = 0.0f, iv = 0.0f;
    if (tri_hit(a, b, c, r, it, iu, iv) && r.tmin < it && it < r.tmax) sink.put(it, iu, iv, prim, inst);
}

template <bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_hits_walk(SceneQuery a, SceneHits h) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 t = *h.total; if (t > h.capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= a.n_rays) return;
    SceneHitSink<FILL, SORTED> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = h.offsets[i], end = h.offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = reinterpret_cast<float4*>(h.hits) + 2 * (size_t)base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    QRay w;
    const bool live = ray_load(reinterpret_cast<const bvh_ray*>(a.rays), i, w);
    bool deep = false;
    if (live) {                                                   // (a NaN component or !(tmin < tmax): accepts nothing)
        QRay r = w;
        SceneBlas B{};
        const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
        u32 ni = tni, total = ttotal;                                 // of the level the ray is on
        bool in_blas = false, pop = false, entering = false;         // entering: instance `enter` is entered at the top of the next step
        u32 inst = INV, enter = INV;
        u32 nl = INV, nr = INV, top = 0, tsteps = 0, bsteps = 0;
        if (a.n_inst == 1) {                                          // no top-level tree: the instance's world box, then the instance
            float tn;
            if (box_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), w, w.tmax, tn)) { enter = 0; entering = true; } else pop = true;
        } else {
            const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(a.tnodes) + a.troot); nl = lr.x; nr = lr.y;
        }
        for (;;) {
            if (entering) {
                entering = false;
                const u32 k = enter;
                if (k < a.n_inst && enter_instance_ray(a, k, w, r, B)) {
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
                float ta = 0.0f, tb = 0.0f;
                bool ha = false, hb = false;
                if (nl < total) { rec_fetch_rt(layout, nodes, leaves, nl, ni, a0, a1, ba); ha = box_pass(ba, r, w.tmax, ta); }
                if (nr < total) { rec_fetch_rt(layout, nodes, leaves, nr, ni, b0, b1, bb); hb = box_pass(bb, r, w.tmax, tb); }
                if (in_blas) {                                        // triangles at once; at the top level a leaf is an instance, entered like a node
                    if (ha && nl >= ni) { scene_hit_leaf(B, a0, inst, r, sink); ha = false; }
                    if (hb && nr >= ni) { scene_hit_leaf(B, b0, inst, r, sink); hb = false; }
                }
                if (ha || hb) {
                    if (ha && hb) {                                   // every passing subtree is visited: left first, right pushed
                        if (top == (u32)QUERY_STACK) { deep = true; break; }
                        stack[top * QUERY_BLOCK] = nr | (in_blas ? SCENE_BLAS_ENTRY : 0u); ++top;
                    }
                    const u32 c = ha ? nl : nr, c0 = ha ? a0 : b0, c1 = ha ? a1 : b1;
                    if (in_blas || c < tni) { nl = c0; nr = c1; }
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
                    if (in_blas) { r = w; in_blas = false; ni = tni; total = ttotal; }   // back to the top level: the world ray
                    u32 w0, w1; Box b;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, e, tni, w0, w1, b);
                    if (e < tni) { nl = w0; nr = w1; } else { enter = w0; entering = true; }
                }
            }
        }
    }
    if (deep) atomicAdd(a.overflow, 1u);
    if (FILL) { if (deep) reinterpret_cast<u32*>(sink.out)[3] = QUERY_MARK; }
    else h.offsets[i] = deep ? QUERY_MARK : sink.k;
}

// stackless walk of instance k's BLAS through its plan (k_hits_deep's walk: the root's own box is not tested, every other record's is)
template <bool FILL, bool SORTED>
__device__ void scene_hits_walk_blas(const SceneQuery& a, u32 k, const QRay& w, SceneHitSink<FILL, SORTED>& sink) {
    QRay r; SceneBlas B;
    if (k >= a.n_inst || !enter_instance_ray(a, k, w, r, B)) return;
    const u32 ni = B.n - 1, total = 2 * B.n - 1;
    const u64 bound = 3ull * total + 3ull;
    u32 cur = B.root, last = INV;
    bool down = true;
    for (u64 steps = 0; cur < total && steps < bound; ++steps) {
        if (down) {
            u32 w0, w1; Box b; float tn;
            rec_fetch_rt((int)B.layout, B.nodes, B.leaves, cur, ni, w0, w1, b);
            if (cur >= ni) {
                if (box_pass(b, r, w.tmax, tn)) scene_hit_leaf(B, w0, k, r, sink);
                last = cur; cur = B.parent[cur]; down = false;
                continue;
            }
            if (cur != B.root && !box_pass(b, r, w.tmax, tn)) { last = cur; cur = B.parent[cur]; down = false; continue; }   // (the BLAS root's own box: as the stack walk, not tested)
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

// the stackless re-walk of the marked rays: the top-level plan, and for every instance whose world box passes, that BLAS's plan; left child first
template <bool FILL, bool SORTED>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_hits_deep(SceneQuery a, SceneHits h) {
    if (*a.overflow == 0u) return;
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 bound = 3ull * ttotal + 3ull;
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < a.n_rays; i += nbid_x() * QUERY_BLOCK) {
        SceneHitSink<FILL, SORTED> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = h.offsets[i], end = h.offsets[i + 1];
            if (end <= base) continue;
            float4* const out = reinterpret_cast<float4*>(h.hits) + 2 * (size_t)base;
            if (__float_as_uint(out[0].w) != QUERY_MARK) continue;
            sink.out = out; sink.room = end - base;
        } else if (h.offsets[i] != QUERY_MARK) continue;
        QRay w;
        ray_load(reinterpret_cast<const bvh_ray*>(a.rays), i, w);     // (a marked ray passed the checks)
        if (a.n_inst == 1) {
            float tn;
            if (box_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), w, w.tmax, tn)) scene_hits_walk_blas(a, 0, w, sink);
        } else {
            u32 cur = a.troot, last = INV;
            bool down = true;
            for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
                if (down) {
                    u32 w0, w1; Box b; float tn;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, cur, tni, w0, w1, b);
                    if (cur != a.troot && !box_pass(b, w, w.tmax, tn)) { last = cur; cur = a.tparent[cur]; down = false; continue; }   // (the root's own box: as the stack walk, not tested)
                    if (cur >= tni) {                                 // an instance whose world box passes
                        scene_hits_walk_blas(a, w0, w, sink);
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
template <bool FILL, bool SORTED> void scene_hits_pass(hipStream_t s, const SceneQuery& q, const SceneHits& h) {
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    { KernelScope ks(s, FILL ? "k_scene_hits_fill" : "k_scene_hits_count");
      hipLaunchKernelGGL((k_scene_hits_walk<FILL, SORTED>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, q, h); }
    { KernelScope ks(s, "k_scene_hits_deep");                     // (the fill's overflow word stays 0 when the fill returned at once)
      hipLaunchKernelGGL((k_scene_hits_deep<FILL, SORTED>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q, h); }
}
} // namespace

void launch_scene_hits_count(hipStream_t s, const SceneQuery& q, const SceneHits& h, uint64_t* d_sums, uint64_t* d_total) {
    scene_hits_pass<false, false>(s, q, h);
    launch_overlap_scan(s, h.offsets, q.n_rays, d_sums, d_total);
}

void launch_scene_hits_fill(hipStream_t s, int sorted, const SceneQuery& q, const SceneHits& h) {
    if (sorted) scene_hits_pass<true, true>(s, q, h); else scene_hits_pass<true, false>(s, q, h);
}

void warm_scene_multihit() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_hits_walk<false, false>)); }

} // namespace bvh
