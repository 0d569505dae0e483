// cull.hip — bvh_cull on gfx950: which primitives' leaf boxes lie inside or across each convex volume (up to BVH_CULL_MAX_PLANES half-spaces: a view frustum, a
// tile or cluster volume, a shadow cascade), against a built BVH2 in either node layout (no counterpart in the reference).  bvh_overlap's call shape: count -> scan
// (overlap.hip's, shared) -> fill, count and fill the SAME walk, templated on node layout and pass.  Two walks serve a volume:
//   k_cull_walk  : one volume per lane, k_overlap_walk's shape — short per-lane stack in LDS (QUERY_STACK entries), both children fetched and tested per internal
//                  node, a passing leaf child counted / stored at once, of two passing internal children the left entered and the right pushed; a volume whose push
//                  would overflow (or whose walk exceeds the node count: arrays that are not a tree) is marked and bumps the pass's overflow word.  The lane's
//                  planes stay in registers (at most 32 VGPRs); a popped node restarts with all planes: no mask travels with an entry.
//   k_cull_group : one volume per workgroup of CULL_GROUP_BLOCK = 256 threads, for the few-volumes-on-a-big-tree calls that would otherwise run on a handful of
//                  lanes.  The volume's planes are read through a workgroup-uniform address (SGPRs).  The work stack is an LDS array of BVH_CULL_GROUP_STACK
//                  internal node indices.  Each round takes the m = min(top, 256) entries at the top, thread t entry top - m + t; the thread fetches and tests
//                  both children; leaf survivors are emitted and internal survivors pushed (from slot top - m on), both in thread order, left child before right.
//                  Slots come from a workgroup-wide exclusive prefix — ballot and mbcnt within a wave, the four waves' partial sums through LDS —, so emission
//                  uses no atomics and a slice's bytes do not depend on timing.  A round whose pushes would exceed the stack marks the volume as the lane walk
//                  does.  Two barriers per round: after the partial sums (every entry of the round has been read by then) and after the pushes.
//   k_cull_deep  : launched after each pass, returns at once while that pass's overflow word is 0; otherwise redoes every marked volume from its start, one per
//                  lane, stackless through the parent links of bvh_refit's plan, left child first (k_overlap_deep's shape).  Correct at any depth.
// Marks: count pass, the count word (QUERY_MARK is never a count: n < 2^30); fill pass, the prim word of the slice's first record (a volume with an empty slice is
// not walked at all; QUERY_MARK is never a primitive).  All three walks report exactly the leaves whose own box and every box above them (the root's excepted:
// no walk tests it) pass the volume, so count and fill agree whichever walk served a volume.
// The box test is the header's, operation for operation: every product and sum one round-to-nearest f32 operation (__fmul_rn / __fadd_rn: never contracted),
// monotone under box containment in rounded f32, so the answer is exact for every volume.  Built without the SLP vectoriser (Makefile).
#include <type_traits>
#include "cull.hpp"
#include "kernels.hpp"

namespace bvh {

constexpr u32 CULL_GROUP_STACK = BVH_CULL_GROUP_STACK;
constexpr int CULL_GROUP_WAVES = CULL_GROUP_BLOCK / WAVE;
static_assert(CULL_GROUP_WAVES == 4, "k_cull_group adds up four waves' partial sums");

// Planes, planes_load, plane_s, cull_pass and cull_straddle — the header's test — live in cull.hpp, which scene_cull.hip shares

// where a lane's results go.  Count pass: a counter.  Fill pass: the volume's slice [base, base + room) of d_hits, never written past its end (overlap.hip's Sink);
// the straddle mask is only worked out where it is stored
template <bool FILL> struct CullSink {
    bvh_cull_hit* out; u32 room, k = 0;
    __device__ __forceinline__ void put(u32 prim, const Planes& P, u32 np, const Box& b) {
        if (FILL) { if (k < room) { out[k].prim = prim; out[k].straddle = cull_straddle(P, np, b); } }
        ++k;
    }
};

template <int LAYOUT, bool FILL>
__global__ __launch_bounds__(QUERY_BLOCK) void k_cull_walk(const float* __restrict__ planes, u32 n_volumes, u32 np, const bvh2_node* __restrict__ nodes,
                                                           const bvh_primref* __restrict__ leaves, u32 n, u32 root, u32* __restrict__ offsets,
                                                           bvh_cull_hit* __restrict__ hits, const u64* __restrict__ total_word, u64 capacity,
                                                           u32* __restrict__ overflow) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    if (FILL) { const u64 t = *total_word; if (t > capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= n_volumes) return;
    CullSink<FILL> sink{ nullptr, 0u };
    if (FILL) {
        const u32 base = offsets[i], end = offsets[i + 1];
        if (end <= base) return;                                  // an empty slice: nothing to find, nowhere to put a mark
        sink.out = hits + base; sink.room = end - base;
    }
    u32* const stack = s_stack + tid_x();
    const Planes P = planes_load(planes + (size_t)i * np * 4u, np);
    bool deep = false;
    {
        const u32 ni = n - 1, total = 2 * n - 1;
        u32 nl, nr; { const uint2 lr = *reinterpret_cast<const uint2*>(nodes + root); nl = lr.x; nr = lr.y; }
        u32 top = 0, steps = 0;
        for (;;) {
            if (++steps > n) { deep = true; break; }              // more expansions than internal nodes: not a tree (a tree never gets here)
            u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
            Box ba, bb;
            bool ha = false, hb = false;
            if (nl < total) { rec_fetch<LAYOUT>(nodes, leaves, nl, ni, a0, a1, ba); ha = cull_pass(P, np, ba); }
            if (nr < total) { rec_fetch<LAYOUT>(nodes, leaves, nr, ni, b0, b1, bb); hb = cull_pass(P, np, bb); }
            if (ha && nl >= ni) { if (a0 < n) sink.put(a0, P, np, ba); ha = false; }
            if (hb && nr >= ni) { if (b0 < n) sink.put(b0, P, np, bb); hb = false; }
            if (ha || hb) {
                if (ha && hb) {
                    if (top == (u32)QUERY_STACK) { deep = true; break; }
                    stack[top * QUERY_BLOCK] = nr; ++top;
                }
                nl = ha ? a0 : b0; nr = ha ? a1 : b1;             // (selects of values, as k_overlap_walk)
            } else {
                if (top == 0) break;
                const u32 node = stack[--top * QUERY_BLOCK];
                const uint2 lr = *reinterpret_cast<const uint2*>(nodes + node);
                nl = lr.x; nr = lr.y;
            }
        }
    }
    if (deep) atomicAdd(overflow, 1u);
    if (FILL) { if (deep) sink.out[0].prim = QUERY_MARK; }
    else offsets[i] = deep ? QUERY_MARK : sink.k;
}

// the stackless re-walk of the marked volumes, whichever walk marked them: parent links of the plan, left child first
template <int LAYOUT, bool FILL>
__global__ __launch_bounds__(QUERY_BLOCK) void k_cull_deep(const float* __restrict__ planes, u32 n_volumes, u32 np, const bvh2_node* __restrict__ nodes,
                                                           const bvh_primref* __restrict__ leaves, u32 n, u32 root, u32* __restrict__ offsets,
                                                           bvh_cull_hit* __restrict__ hits, const u32* __restrict__ overflow, const u32* __restrict__ parent) {
    if (*overflow == 0u) return;
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < n_volumes; i += nbid_x() * QUERY_BLOCK) {
        CullSink<FILL> sink{ nullptr, 0u };
        if (FILL) {
            const u32 base = offsets[i], end = offsets[i + 1];
            if (end <= base || hits[base].prim != QUERY_MARK) continue;
            sink.out = hits + base; sink.room = end - base;
        } else if (offsets[i] != QUERY_MARK) continue;
        const Planes P = planes_load(planes + (size_t)i * np * 4u, np);
        u32 cur = root, last = INV;
        bool down = true;
        for (u64 steps = 0; cur < total && steps < bound; ++steps) {
            if (down) {
                u32 w0, w1; Box b;
                rec_fetch<LAYOUT>(nodes, leaves, cur, ni, w0, w1, b);
                if (cur >= ni) {
                    if (cull_pass(P, np, b) && w0 < n) sink.put(w0, P, np, b);
                    last = cur; cur = parent[cur]; down = false;
                    continue;
                }
                if (cur != root && !cull_pass(P, np, b)) { last = cur; cur = parent[cur]; down = false; continue; }   // (the root's own box: as the other walks, not tested)
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

// one volume per workgroup.  Every quantity that steers the loop (top, emitted, popped, the partial sums) is the same in all 256 threads, so every break is
// taken by the whole workgroup and the barriers always meet
template <int LAYOUT, bool FILL>
__global__ __launch_bounds__(CULL_GROUP_BLOCK) void k_cull_group(const float* __restrict__ planes, u32 np, const bvh2_node* __restrict__ nodes,
                                                                 const bvh_primref* __restrict__ leaves, u32 n, u32 root, u32* __restrict__ offsets,
                                                                 bvh_cull_hit* __restrict__ hits, const u64* __restrict__ total_word, u64 capacity,
                                                                 u32* __restrict__ overflow) {
    __shared__ u32 s_stack[CULL_GROUP_STACK];
    __shared__ u32 s_part[CULL_GROUP_WAVES][2];                   // per wave: leaf survivors, internal survivors of the round
    if (FILL) { const u64 t = *total_word; if (t > capacity || t > 0xFFFFFFFFull) return; }      // (uniform: the whole launch returns)
    const u32 i = bid_x(), t = tid_x(), wave = t / WAVE;
    u32 base = 0, room = 0;
    if (FILL) {
        base = offsets[i]; const u32 end = offsets[i + 1];
        if (end <= base) return;                                  // an empty slice (uniform: the whole workgroup returns)
        room = end - base;
    }
    const Planes P = planes_load(planes + (size_t)i * np * 4u, np);   // a workgroup-uniform address: scalar loads, the planes stay in SGPRs
    const u32 ni = n - 1, total = 2 * n - 1;
    const u64 below = lanemask_lt();
    if (t == 0) s_stack[0] = root;
    __syncthreads();
    u32 top = 1, emitted = 0, popped = 0;
    bool deep = false;
    while (top > 0) {
        const u32 m = top < (u32)CULL_GROUP_BLOCK ? top : (u32)CULL_GROUP_BLOCK, first = top - m;
        popped += m;
        if (popped > n) { deep = true; break; }                   // more expansions than internal nodes: not a tree (a tree never gets here)
        u32 nl = INV, nr = INV;
        if (t < m) { const uint2 lr = *reinterpret_cast<const uint2*>(nodes + s_stack[first + t]); nl = lr.x; nr = lr.y; }
        u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
        Box ba, bb;
        bool ea = false, eb = false, pa = false, pb = false;      // emit / push the left (a) and the right (b) child
        if (nl < total) { rec_fetch<LAYOUT>(nodes, leaves, nl, ni, a0, a1, ba); if (cull_pass(P, np, ba)) { if (nl >= ni) ea = a0 < n; else pa = true; } }
        if (nr < total) { rec_fetch<LAYOUT>(nodes, leaves, nr, ni, b0, b1, bb); if (cull_pass(P, np, bb)) { if (nr >= ni) eb = b0 < n; else pb = true; } }
        const u64 m_ea = __builtin_amdgcn_ballot_w64(ea), m_eb = __builtin_amdgcn_ballot_w64(eb);
        const u64 m_pa = __builtin_amdgcn_ballot_w64(pa), m_pb = __builtin_amdgcn_ballot_w64(pb);
        if ((t & (WAVE - 1u)) == 0u) { s_part[wave][0] = __popcll(m_ea) + __popcll(m_eb); s_part[wave][1] = __popcll(m_pa) + __popcll(m_pb); }
        __syncthreads();                                          // (every thread has read its entry: the pushes below may overwrite the round's slots)
        u32 e_at = __popcll(m_ea & below) + __popcll(m_eb & below), p_at = __popcll(m_pa & below) + __popcll(m_pb & below), e_all = 0, p_all = 0;
#pragma unroll
        for (u32 w = 0; w < (u32)CULL_GROUP_WAVES; ++w) {
            const u32 e = s_part[w][0], p = s_part[w][1];
            if (w < wave) { e_at += e; p_at += p; }
            e_all += e; p_all += p;
        }
        if (first + p_all > CULL_GROUP_STACK) { deep = true; break; }
        if (FILL) {
            u32 slot = emitted + e_at;
            if (ea) { if (slot < room) { hits[base + slot].prim = a0; hits[base + slot].straddle = cull_straddle(P, np, ba); } ++slot; }
            if (eb) { if (slot < room) { hits[base + slot].prim = b0; hits[base + slot].straddle = cull_straddle(P, np, bb); } }
        }
        u32 at = first + p_at;
        if (pa) s_stack[at++] = nl;
        if (pb) s_stack[at] = nr;
        top = first + p_all; emitted += e_all;
        __syncthreads();
    }
    if (t == 0) {
        if (deep) {
            atomicAdd(overflow, 1u);
            if (FILL) hits[base].prim = QUERY_MARK; else offsets[i] = QUERY_MARK;
        } else if (!FILL) offsets[i] = emitted;
    }
}

// one pass: the chosen walk, then the stackless kernel on the same overflow word
template <bool FILL>
static void cull_pass_launch(hipStream_t s, int layout, bool group, const float* planes, u32 n_volumes, u32 np, const void* d_nodes, const void* d_leaves, u32 n,
                             u32 root, u32* d_offsets, bvh_cull_hit* d_hits, u64 capacity, const u64* d_total, u32* d_overflow, const u32* d_parent) {
    const u32 blocks = (n_volumes + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    const bvh2_node* nodes = (const bvh2_node*)d_nodes; const bvh_primref* leaves = (const bvh_primref*)d_leaves;
    auto go = [&](auto L) {
        constexpr int LA = decltype(L)::value;
        if (group) {
            KernelScope ks(s, "k_cull_group");
            hipLaunchKernelGGL((k_cull_group<LA, FILL>), dim3(n_volumes), dim3(CULL_GROUP_BLOCK), 0, s, planes, np, nodes, leaves, n, root, d_offsets, d_hits,
                               d_total, capacity, d_overflow);
        } else {
            KernelScope ks(s, "k_cull_walk");
            hipLaunchKernelGGL((k_cull_walk<LA, FILL>), dim3(blocks), dim3(QUERY_BLOCK), 0, s, planes, n_volumes, np, nodes, leaves, n, root, d_offsets, d_hits,
                               d_total, capacity, d_overflow);
        }
        { KernelScope ks(s, "k_cull_deep");                       // (a fill's overflow word stays 0 when the fill returned at once)
          hipLaunchKernelGGL((k_cull_deep<LA, FILL>), dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, planes, n_volumes, np, nodes, leaves, n, root, d_offsets, d_hits,
                             (const u32*)d_overflow, d_parent); }
    };
    if (layout == 0) go(std::integral_constant<int, 0>{}); else go(std::integral_constant<int, 1>{});
}

void launch_cull_count(hipStream_t s, int layout, bool group, const float* d_planes, uint32_t n_volumes, uint32_t planes, const void* d_nodes,
                       const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, uint32_t* d_overflow, const uint32_t* d_parent, uint64_t* d_sums,
                       uint64_t* d_total) {
    cull_pass_launch<false>(s, layout, group, d_planes, n_volumes, planes, d_nodes, d_leaves, n, root, d_offsets, nullptr, 0, nullptr, d_overflow, d_parent);
    launch_overlap_scan(s, d_offsets, n_volumes, d_sums, d_total);
}

void launch_cull_fill(hipStream_t s, int layout, bool group, const float* d_planes, uint32_t n_volumes, uint32_t planes, const void* d_nodes,
                      const void* d_leaves, uint32_t n, uint32_t root, uint32_t* d_offsets, void* d_hits, uint64_t capacity, const uint64_t* d_total,
                      uint32_t* d_overflow, const uint32_t* d_parent) {
    cull_pass_launch<true>(s, layout, group, d_planes, n_volumes, planes, d_nodes, d_leaves, n, root, d_offsets, (bvh_cull_hit*)d_hits, capacity, d_total,
                           d_overflow, d_parent);
}

} // namespace bvh
