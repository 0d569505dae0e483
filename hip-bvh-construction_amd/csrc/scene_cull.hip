// scene_cull.hip — bvh_scene_cull on gfx950: which triangles' leaf boxes of which active instances pass each WORLD-space convex volume (up to
// BVH_CULL_MAX_PLANES half-spaces), on an instanced scene and after bvh_scene_update alone (no counterpart in the reference).  bvh_cull's test (cull.hpp) on
// both levels: at the top level on the top-level nodes and the instances' world boxes against the WORLD planes, inside instance k on every record below the
// BLAS root against the OBJECT planes of (volume, k), made once on entry from the caller's forward matrix m_rc = object_to_world[4r + c]:
//   a' = (a m00 + b m10) + c m20, b' and c' with columns 1 and 2, d' = ((a m03 + b m13) + c m23) + d
// every product and sum one round-to-nearest f32 operation.  A plane maps to a plane under an affine map, so the instance is tested as its oriented box and no
// inverse is used.  Inside an instance the object planes are fixed numbers and cull.hpp's test is monotone under containment, so every box above a passing leaf
// passes and the answer is exact for EVERY volume.  bvh_scene_overlap's call shape: count -> scan (overlap.hip's) -> fill, count and fill the
// SAME walk, templated on the pass; the node layout is chosen at run time (rec_fetch_rt).  Three kernels:
//   k_scene_cull_walk  : one volume per lane, k_scene_overlap_walk's two-level loop — one LDS short stack of QUERY_STACK entries for both levels
//                        (SCENE_BLAS_ENTRY tags a BLAS node), of two passing children the left entered and the right pushed, step bounds that end arrays which
//                        are not a tree.  World and object planes both stay in registers (64 VGPRs).
//   k_scene_cull_group : one volume per workgroup of CULL_GROUP_BLOCK = 256 threads, k_cull_group's fixed schedule on two levels.  The work stack is two u32
//                        columns {instance, node} of BVH_SCENE_CULL_GROUP_STACK entries in LDS; instance == INV marks a top-level entry.  Each round takes the
//                        m = min(top, 256) entries at the top, thread t entry top - m + t.  A thread on a top-level entry tests both children with the world
//                        planes (a workgroup-uniform address: SGPRs); a passing internal child is pushed, a passing leaf whose instance is active is pushed as
//                        {k, that BLAS's root}.  A thread on a BLAS entry makes its instance's object planes (per thread and per round), tests both children,
//                        emits leaf survivors and pushes internal ones.  Slots come from k_cull_group's workgroup-wide exclusive prefix — ballots, popcounts
//                        below the lane, the four waves' partial sums through LDS, thread order, left before right —: no atomics, two barriers per round.
//   k_scene_cull_deep  : launched after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked volume from its start, one
//                        per lane, stackless through the top-level plan and each entered BLAS's plan, left child first (k_scene_overlap_deep's shape).
// All three test the SAME boxes — every record below a root, and neither the top-level root's own box nor a BLAS root's own box (the instance's world box stands
// for it) —, so count and fill agree on a volume's set whichever walk served it.
// Marks: count pass, the count word (a count saturates at QUERY_MARK - 1); fill pass, the prim word of the slice's first record (a volume with an empty slice is
// not walked; QUERY_MARK is never a primitive).  A record is 16 bytes {prim, instance, straddle, 0} and leaves in one store.
// Built with -ffp-contract=off and without the SLP vectoriser (Makefile), as cull.o and scene_overlap.o.
#include "cull.hpp"
#include "scene_map.hpp"
#include "kernels.hpp"

namespace bvh {

constexpr u32 SCULL_GROUP_STACK = BVH_SCENE_CULL_GROUP_STACK;
constexpr int SCULL_GROUP_WAVES = CULL_GROUP_BLOCK / WAVE;
static_assert(SCULL_GROUP_WAVES == 4, "k_scene_cull_group adds up four waves' partial sums");
static_assert(sizeof(bvh_scene_cull_hit) == sizeof(uint4), "a record leaves in one 16-byte store");

// the header's object planes of world planes W in the instance whose forward matrix is M (planes at and above np keep the padding values: never tested)
__device__ __forceinline__ Planes scull_object_planes(const Planes& W, u32 np, const SOMat& M) {
    Planes O;
#pragma unroll
    for (int k = 0; k < CULL_PLANES; ++k) {
        const bool on = (u32)k < np;
        const float a = W.a[k], b = W.b[k], c = W.c[k], d = W.d[k];
        O.a[k] = on ? __fadd_rn(__fadd_rn(__fmul_rn(a, M.r0.x), __fmul_rn(b, M.r1.x)), __fmul_rn(c, M.r2.x)) : 0.0f;
        O.b[k] = on ? __fadd_rn(__fadd_rn(__fmul_rn(a, M.r0.y), __fmul_rn(b, M.r1.y)), __fmul_rn(c, M.r2.y)) : 0.0f;
        O.c[k] = on ? __fadd_rn(__fadd_rn(__fmul_rn(a, M.r0.z), __fmul_rn(b, M.r1.z)), __fmul_rn(c, M.r2.z)) : 0.0f;
        O.d[k] = on ? __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, M.r0.w), __fmul_rn(b, M.r1.w)), __fmul_rn(c, M.r2.w)), d) : 1.0f;
    }
    planes_pick(O);
    return O;
}

// where a lane's records go (CullSink for bvh_scene_cull_hit records; the counter saturates below the mark: many instances of one BLAS can answer)
template <bool FILL> struct SceneCullSink {
    uint4* out; u32 room, k = 0;
    __device__ __forceinline__ void put(u32 prim, u32 inst, const Planes& O, u32 np, const Box& b) {
        if (FILL) { if (k < room) out[k] = make_uint4(prim, inst, cull_straddle(O, np, b), 0u); }
        if (k < QUERY_MARK - 1u) ++k;
    }
};

template <bool FILL>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_cull_walk(SceneQuery a, SceneHits h, u32 np) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 t = *h.total; if (t > h.capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= a.n_rays) return;
    SceneCullSink<FILL> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = h.offsets[i], end = h.offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = reinterpret_cast<uint4*>(h.hits) + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    const Planes W = planes_load(reinterpret_cast<const float*>(a.rays) + (size_t)i * np * 4u, np);
    bool deep = false;
    {
        Planes O = W;                                                 // the entered instance's object planes
        SceneBlas B{};
        const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
        u32 ni = tni, total = ttotal;                                 // of the level the volume is on
        bool in_blas = false, pop = false, entering = false;         // entering: instance `enter` is entered at the top of the next step
        u32 inst = INV, enter = INV;
        u32 nl = INV, nr = INV, top = 0, tsteps = 0, bsteps = 0;
        if (a.n_inst == 1) {                                          // no top-level tree: the instance's world box, then the instance
            if (cull_pass(W, np, box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)))) { enter = 0; entering = true; } else pop = true;
        } else {
            const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(a.tnodes) + a.troot); nl = lr.x; nr = lr.y;
        }
        for (;;) {
            if (entering) {
                entering = false;
                const u32 k = enter;
                SOMat M{};
                if (k < a.n_inst && sov_enter_instance(a, k, M, B)) {
                    O = scull_object_planes(W, np, M);
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
                if (nl < total) { rec_fetch_rt(layout, nodes, leaves, nl, ni, a0, a1, ba); ha = in_blas ? cull_pass(O, np, ba) : cull_pass(W, np, ba); }
                if (nr < total) { rec_fetch_rt(layout, nodes, leaves, nr, ni, b0, b1, bb); hb = in_blas ? cull_pass(O, np, bb) : cull_pass(W, np, bb); }
                if (in_blas) {                                        // triangles at once; at the top level a leaf is an instance, entered like a node
                    if (ha && nl >= ni) { if (a0 < B.n) sink.put(a0, inst, O, np, ba); ha = false; }
                    if (hb && nr >= ni) { if (b0 < B.n) sink.put(b0, inst, O, np, bb); hb = false; }
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
template <bool FILL>
__device__ void scull_walk_blas(const SceneQuery& a, u32 k, const Planes& W, u32 np, SceneCullSink<FILL>& sink) {
    SOMat M; SceneBlas B;
    if (k >= a.n_inst || !sov_enter_instance(a, k, M, B)) return;
    const Planes O = scull_object_planes(W, np, M);
    const u32 ni = B.n - 1, total = 2 * B.n - 1;
    const u64 bound = 3ull * total + 3ull;
    u32 cur = B.root, last = INV;
    bool down = true;
    for (u64 steps = 0; cur < total && steps < bound; ++steps) {
        if (down) {
            u32 w0, w1; Box b;
            rec_fetch_rt((int)B.layout, B.nodes, B.leaves, cur, ni, w0, w1, b);
            if (cur >= ni) {
                if (cull_pass(O, np, b) && w0 < B.n) sink.put(w0, k, O, np, b);
                last = cur; cur = B.parent[cur]; down = false;
                continue;
            }
            if (cur != B.root && !cull_pass(O, np, b)) { last = cur; cur = B.parent[cur]; down = false; continue; }   // (the BLAS root's own box: as the stack walks, not tested)
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

// the stackless re-walk of the marked volumes, whichever walk marked them: the top-level plan, and for every instance whose world box passes, that BLAS's plan
template <bool FILL>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_cull_deep(SceneQuery a, SceneHits h, u32 np) {
    if (*a.overflow == 0u) return;
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 bound = 3ull * ttotal + 3ull;
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < a.n_rays; i += nbid_x() * QUERY_BLOCK) {
        SceneCullSink<FILL> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = h.offsets[i], end = h.offsets[i + 1];
            if (end <= base) continue;
            uint4* const out = reinterpret_cast<uint4*>(h.hits) + base;
            if (out[0].x != QUERY_MARK) continue;
            sink.out = out; sink.room = end - base;
        } else if (h.offsets[i] != QUERY_MARK) continue;
        const Planes W = planes_load(reinterpret_cast<const float*>(a.rays) + (size_t)i * np * 4u, np);
        if (a.n_inst == 1) {
            if (cull_pass(W, np, box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)))) scull_walk_blas(a, 0, W, np, sink);
        } else {
            u32 cur = a.troot, last = INV;
            bool down = true;
            for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
                if (down) {
                    u32 w0, w1; Box b;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, cur, tni, w0, w1, b);
                    if (cur != a.troot && !cull_pass(W, np, b)) { last = cur; cur = a.tparent[cur]; down = false; continue; }   // (the root's own box: as the stack walks, not tested)
                    if (cur >= tni) {                                 // an instance whose world box passes
                        scull_walk_blas(a, w0, W, np, sink);
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

// one volume per workgroup.  Every quantity that steers the loop (top, emitted, popped, the partial sums) is the same in all 256 threads, so every break is
// taken by the whole workgroup and the barriers always meet.  max_pops: more expansions than the scene has internal nodes (the host's bound: n_instances
// top-level nodes and, per instance, the largest BLAS) — arrays that are not a tree
template <bool FILL>
__global__ __launch_bounds__(CULL_GROUP_BLOCK) void k_scene_cull_group(SceneQuery a, SceneHits h, u32 np, u64 max_pops) {
    __shared__ u32 s_inst[SCULL_GROUP_STACK];
    __shared__ u32 s_node[SCULL_GROUP_STACK];
    __shared__ u32 s_part[SCULL_GROUP_WAVES][2];                  // per wave: leaf survivors, pushed survivors of the round
    if (FILL) { const u64 t = *h.total; if (t > h.capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x(), t = tid_x(), wave = t / WAVE;
    u32 base = 0, room = 0;
    if (FILL) {
        base = h.offsets[i]; const u32 end = h.offsets[i + 1];
        if (end <= base) return;                                  // an empty slice (uniform: the whole workgroup returns)
        room = end - base;
    }
    uint4* const hits = reinterpret_cast<uint4*>(h.hits);
    const Planes W = planes_load(reinterpret_cast<const float*>(a.rays) + (size_t)i * np * 4u, np);   // a workgroup-uniform address: scalar loads, SGPRs
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 below = lanemask_lt();
    u32 top = 0;
    if (a.n_inst == 1) {                                          // no top-level tree: the instance's world box, then {0, its BLAS's root} (all uniform)
        const u32 bl = __float_as_uint(reinterpret_cast<const float4*>(a.inst)[3].x);
        if (bl != INV && cull_pass(W, np, box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)))) {
            if (t == 0) { s_inst[0] = 0u; s_node[0] = a.blas[bl].root; }
            top = 1;
        }
    } else {
        if (t == 0) { s_inst[0] = INV; s_node[0] = a.troot; }
        top = 1;
    }
    __syncthreads();
    u32 emitted = 0;
    u64 popped = 0;
    bool deep = false;
    while (top > 0) {
        const u32 m = top < (u32)CULL_GROUP_BLOCK ? top : (u32)CULL_GROUP_BLOCK, first = top - m;
        popped += m;
        if (popped > max_pops) { deep = true; break; }            // (a tree never gets here)
        u32 k = INV, nl = INV, nr = INV, ni = tni, total = ttotal, nprim = a.n_inst;
        int layout = (int)a.tlayout;
        const void* nodes = a.tnodes; const void* leaves = a.tleaves;
        Planes T = W;                                             // the planes this thread's entry is tested with
        if (t < m) {
            k = s_inst[first + t];
            const u32 node = s_node[first + t];
            if (k != INV) {                                       // a BLAS entry of instance k (active: checked when it was pushed)
                SOMat M; SceneBlas B;
                if (k < a.n_inst && sov_enter_instance(a, k, M, B)) {
                    T = scull_object_planes(W, np, M);
                    nodes = B.nodes; leaves = B.leaves; layout = (int)B.layout; nprim = B.n; ni = B.n - 1; total = 2 * B.n - 1;
                    if (node < ni) { const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(nodes) + node); nl = lr.x; nr = lr.y; }
                }
            } else if (node < tni) { const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(nodes) + node); nl = lr.x; nr = lr.y; }
        }
        const bool in_blas = k != INV;
        u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
        Box ba, bb;
        bool ea = false, eb = false, pa = false, pb = false;      // emit / push the left (a) and the right (b) child
        u32 ia = k, ib = k, na = nl, nb = nr;                     // what a push of the child stores
        if (nl < total) {
            rec_fetch_rt(layout, nodes, leaves, nl, ni, a0, a1, ba);
            if (cull_pass(T, np, ba)) { if (nl < ni) pa = true; else if (a0 < nprim) { if (in_blas) ea = true; else pa = true; } }
        }
        if (nr < total) {
            rec_fetch_rt(layout, nodes, leaves, nr, ni, b0, b1, bb);
            if (cull_pass(T, np, bb)) { if (nr < ni) pb = true; else if (b0 < nprim) { if (in_blas) eb = true; else pb = true; } }
        }
        if (!in_blas) {                                           // a passing top-level leaf: its instance, if active, as {k, that BLAS's root}
            if (pa && nl >= tni) { const u32 bl = __float_as_uint(reinterpret_cast<const float4*>(a.inst + a0)[3].x); pa = bl != INV; if (pa) { ia = a0; na = a.blas[bl].root; } }
            if (pb && nr >= tni) { const u32 bl = __float_as_uint(reinterpret_cast<const float4*>(a.inst + b0)[3].x); pb = bl != INV; if (pb) { ib = b0; nb = a.blas[bl].root; } }
        }
        const u64 m_ea = __builtin_amdgcn_ballot_w64(ea), m_eb = __builtin_amdgcn_ballot_w64(eb);
        const u64 m_pa = __builtin_amdgcn_ballot_w64(pa), m_pb = __builtin_amdgcn_ballot_w64(pb);
        if ((t & (WAVE - 1u)) == 0u) { s_part[wave][0] = __popcll(m_ea) + __popcll(m_eb); s_part[wave][1] = __popcll(m_pa) + __popcll(m_pb); }
        __syncthreads();                                          // (every thread has read its entry: the pushes below may overwrite the round's slots)
        u32 e_at = __popcll(m_ea & below) + __popcll(m_eb & below), p_at = __popcll(m_pa & below) + __popcll(m_pb & below), e_all = 0, p_all = 0;
#pragma unroll
        for (u32 w = 0; w < (u32)SCULL_GROUP_WAVES; ++w) {
            const u32 e = s_part[w][0], p = s_part[w][1];
            if (w < wave) { e_at += e; p_at += p; }
            e_all += e; p_all += p;
        }
        if (first + p_all > SCULL_GROUP_STACK) { deep = true; break; }
        if (FILL) {
            u32 slot = emitted + e_at;                            // (< 2^32: the fill runs only when the total is)
            if (ea) { if (slot < room) hits[base + slot] = make_uint4(a0, k, cull_straddle(T, np, ba), 0u); ++slot; }
            if (eb) { if (slot < room) hits[base + slot] = make_uint4(b0, k, cull_straddle(T, np, bb), 0u); }
        }
        u32 at = first + p_at;
        if (pa) { s_inst[at] = ia; s_node[at] = na; ++at; }
        if (pb) { s_inst[at] = ib; s_node[at] = nb; }
        top = first + p_all;
        { const u64 e = (u64)emitted + e_all; emitted = e < (u64)(QUERY_MARK - 1u) ? (u32)e : QUERY_MARK - 1u; }   // (the counter saturates below the mark)
        __syncthreads();
    }
    if (t == 0) {
        if (deep) {
            atomicAdd(a.overflow, 1u);
            if (FILL) hits[base].x = QUERY_MARK; else h.offsets[i] = QUERY_MARK;
        } else if (!FILL) h.offsets[i] = emitted;
    }
}

namespace {
// one pass: the chosen walk, then the stackless kernel on the same overflow word
template <bool FILL> void scene_cull_pass(hipStream_t s, bool group, const SceneQuery& q, const SceneHits& h, u32 np, u64 max_pops) {
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    if (group) {
        KernelScope ks(s, "k_scene_cull_group");
        hipLaunchKernelGGL((k_scene_cull_group<FILL>), dim3(q.n_rays), dim3(CULL_GROUP_BLOCK), 0, s, q, h, np, max_pops);
    } else {
        KernelScope ks(s, "k_scene_cull_walk");
        hipLaunchKernelGGL((k_scene_cull_walk<FILL>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, q, h, np);
    }
    { KernelScope ks(s, "k_scene_cull_deep");                     // (the fill's overflow word stays 0 when the fill returned at once)
      hipLaunchKernelGGL((k_scene_cull_deep<FILL>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q, h, np); }
}
} // namespace

void launch_scene_cull_count(hipStream_t s, bool group, const SceneQuery& q, const SceneHits& h, uint32_t planes, uint64_t max_pops, uint64_t* d_sums,
                             uint64_t* d_total) {
    scene_cull_pass<false>(s, group, q, h, planes, max_pops);
    launch_overlap_scan(s, h.offsets, q.n_rays, d_sums, d_total);
}

void launch_scene_cull_fill(hipStream_t s, bool group, const SceneQuery& q, const SceneHits& h, uint32_t planes, uint64_t max_pops) {
    scene_cull_pass<true>(s, group, q, h, planes, max_pops);
}

void warm_scene_cull() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_cull_walk<false>)); }

} // namespace bvh
