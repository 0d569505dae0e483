// optimize.hip — bvh_optimize on gfx950: treelet restructuring (Karras & Aila, HPG 2013) of an existing BVH2, in place (no counterpart in the reference).
// One launch per round r (gamma = 7 << r), over the parent plan of refit.hip (k_refit_plan, index space {internal [0, n-1), leaf j at n-1+j}):
//   k_optimize : one thread per leaf climbs through parent[] with refit_climb's second-arriver exchange on the self-cleaning flags words — the exchanged
//                value is the arriving subtree's leaf count, so the second arriver knows its node's count.  A node reached with >= gamma leaves is a treelet
//                root; the lanes holding one are served one at a time by the WHOLE wave (ballot): formation of the 7-entry treelet (lane k holds entry k),
//                the 127 subset boxes (two per lane), the DP over subset sizes 2..7 in LDS (3.75 KB per wave), then one lane rebuilds the <= 6 nodes and
//                rewrites parent[] of their children, so the plan stays right for the next round and for bvh_refit / bvh_intersect.
// The treelet root's subtree is final when its second arriver gets there (every lower treelet was rebuilt before its own climb went on), so the result does
// not depend on scheduling.  Lanes of one wave hold disjoint subtrees: a wave never contends with itself; no workgroup ever waits for another.
// Nodes written in this launch are read with agent-scope loads and written write-through (node_store_agent), drained before the next exchange.  parent[] is
// read and written at agent scope too: with plain accesses the MI355X returned stale parent words (108 of 108 optimisations of 1 000-leaf trees correct with
// agent scope, 69 wrong with plain loads / stores).
// Compiled WITHOUT -fno-honor-nans / -mno-amdgpu-ieee (Makefile): the costs may be NaN or infinite and every comparison must stay an IEEE one.
#include "common.hpp"
#include "kernels.hpp"

namespace bvh {

constexpr int OPT_BLOCK = 256;
constexpr int OPT_WAVES = OPT_BLOCK / WAVE;
constexpr u32 TL_SIZE = 7;                        // leaves of a treelet
constexpr u32 TL_FULL = (1u << TL_SIZE) - 1u;    // the subset of all seven

struct TreeletLds {
    Box box[TL_FULL + 1];                          // B(S): union of the entries' boxes, in increasing bit order
    float cost[TL_FULL + 1];                       // c(S)
    unsigned char part[TL_FULL + 1];              // the winning P of S (the subset holding S's lowest bit)
    u32 entry[8];                                  // T[0..6]
    u32 stack_s[8], stack_i[8];                    // the rebuild's preorder walk
};

// every lane's LDS writes before the barrier are seen by every lane's reads after it
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ u32 rl(u32 v, u32 lane) { return (u32)__builtin_amdgcn_readlane((int)v, (int)lane); }
__device__ __forceinline__ float rl(float v, u32 lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)lane)); }
__device__ __forceinline__ Box rl(const Box& b, u32 lane) { return { rl(b.lx, lane), rl(b.ly, lane), rl(b.lz, lane), rl(b.hx, lane), rl(b.hy, lane), rl(b.hz, lane) }; }

// e[k] of five registers without a dynamic register index (which would put e in scratch memory)
__device__ __forceinline__ u32 pick5(const u32 (&e)[5], u32 k) { return k == 0u ? e[0] : k == 1u ? e[1] : k == 2u ? e[2] : k == 3u ? e[3] : e[4]; }

// the record of node i of the index space: child links (internal nodes) and box.  Internal nodes may have been rebuilt by another wave in this launch:
// agent-scope loads.  LAYOUT 1 leaves are PrimRefs (never written here).  An index outside the tree (never in a tree) reads node 0.
template <int LAYOUT>
__device__ __forceinline__ void entry_load(const bvh2_node* nodes, const bvh_primref* leaves, u32 i, u32 ni, u32& l, u32& r, Box& b) {
    if (LAYOUT == 1 && i >= ni) {
        const u32 j = i - ni;
        l = INV; r = INV; b = box_load_u(&leaves[j <= ni ? j : 0u].aabb);
    } else {
        rec_load_agent(nodes + (i < 2 * ni + 1 ? i : 0u), l, r, b);
    }
}

// restructure the treelet rooted at N (wave-uniform; all 64 lanes take part)
template <int LAYOUT>
__device__ void restructure(TreeletLds& L, u32 lane, u32 N, bvh2_node* nodes, const bvh_primref* leaves, u32* parent, u32 ni) {
    const u32 total = 2 * ni + 1;
    wave_sync();                                                                      // (the previous treelet of this wave is done with L)
    u32 nl, nr; Box nbox;
    rec_load_agent(nodes + N, nl, nr, nbox);
    // ---- formation: lane k < |T| holds entry k {index, child links, box}; lane k < 6 holds the treelet's internal node k (N, then E0 .. E4 in expansion order)
    u32 tidx = lane == 0u ? nl : nr, tl = INV, tr = INV; Box tbox = nbox;
    if (lane < 2u) entry_load<LAYOUT>(nodes, leaves, tidx, ni, tl, tr, tbox);
    u32 xidx = N, xl = nl, xr = nr; float xarea = box_area(nbox);
    for (u32 size = 2; size < TL_SIZE; ++size) {
        // the internal entry with the largest area, the earliest on ties (the first internal entry starts the scan, a later one must be strictly larger)
        const float ta = box_area(tbox);
        int pos = -1; float best = 0.0f;
        for (u32 k = 0; k < size; ++k) {
            const u32 ik = rl(tidx, k); const float ak = rl(ta, k);
            if (ik < ni && (pos < 0 || ak > best)) { pos = (int)k; best = ak; }
        }
        if (pos < 0) return;                                                        // (a root with >= 7 leaves always has one: not a tree otherwise)
        const u32 x = rl(tidx, (u32)pos), cl = rl(tl, (u32)pos), cr = rl(tr, (u32)pos);
        if (lane == size - 1u) { xidx = x; xl = cl; xr = cr; xarea = best; }
        if (lane == (u32)pos || lane == size) {                                     // the picked entry becomes its left child, its right child is appended
            tidx = lane == size ? cr : cl;
            entry_load<LAYOUT>(nodes, leaves, tidx, ni, tl, tr, tbox);
        }
    }
    // ---- current cost, deepest expansion first: c_cur(x) = area(x) + (c_cur(left x) + c_cur(right x)), 0 for the entries of T
    u32 xi[TL_SIZE - 1]; float cc[TL_SIZE - 1];
#pragma unroll
    for (int k = (int)TL_SIZE - 2; k >= 0; --k) {
        xi[k] = rl(xidx, (u32)k);
        const u32 l = rl(xl, (u32)k), r = rl(xr, (u32)k);
        float cl = 0.0f, cr = 0.0f;
#pragma unroll
        for (int k2 = k + 1; k2 < (int)TL_SIZE - 1; ++k2) { if (xi[k2] == l) cl = cc[k2]; if (xi[k2] == r) cr = cc[k2]; }
        cc[k] = rl(xarea, (u32)k) + (cl + cr);
    }
    // ---- subset boxes and areas: lane l owns S = l and S = l + 64
    Box tb[TL_SIZE];
#pragma unroll
    for (u32 i = 0; i < TL_SIZE; ++i) tb[i] = rl(tbox, i);
    if (lane < TL_SIZE) L.entry[lane] = tidx;
    float sa[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const u32 S = lane + 64u * (u32)h;
        Box acc = tb[0];
        bool first = true;
#pragma unroll
        for (u32 i = 0; i < TL_SIZE; ++i)
            if ((S >> i) & 1u) { acc = first ? tb[i] : box_union(acc, tb[i]); first = false; }
        sa[h] = box_area(acc);
        if (S != 0u) { L.box[S] = acc; if ((S & (S - 1u)) == 0u) L.cost[S] = 0.0f; }
    }
    wave_sync();
    // ---- DP by subset size: c(S) = area(B(S)) + min over P of (c(P) + c(S \ P)), P holding S's lowest bit, increasing mask order, first strict minimum
    for (int size = 2; size <= (int)TL_SIZE; ++size) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u32 S = lane + 64u * (u32)h;
            if (__popc(S) == size) {
                const u32 low = S & (0u - S), R = S ^ low;
                float best = L.cost[low] + L.cost[S ^ low];
                u32 bestP = low;
                for (u32 sub = (0u - R) & R; sub != R; sub = (sub - R) & R) {
                    const u32 P = low | sub;
                    const float v = L.cost[P] + L.cost[S ^ P];
                    if (v < best) { best = v; bestP = P; }
                }
                L.cost[S] = sa[h] + best;
                L.part[S] = (unsigned char)bestP;
            }
        }
        wave_sync();
    }
    // ---- decision: only a strictly cheaper topology is written (NaN / infinite costs keep the treelet byte for byte)
    if (!(L.cost[TL_FULL] < cc[0])) return;
    // ---- rebuild (one lane): preorder from N, P before Q; a subset of >= 2 entries takes the next of E's indices in ascending order, a singleton is its entry
    if (lane == 0u) {
        u32 e[TL_SIZE - 2];
#pragma unroll
        for (u32 k = 0; k < TL_SIZE - 2; ++k) e[k] = xi[k + 1];
#pragma unroll
        for (u32 a = 1; a < TL_SIZE - 2; ++a)                                       // (sorting network on five registers)
#pragma unroll
            for (u32 b = TL_SIZE - 3; b >= a; --b) { const u32 lo = min(e[b - 1], e[b]), hi = max(e[b - 1], e[b]); e[b - 1] = lo; e[b] = hi; }
        u32 next = 0;
        L.stack_s[0] = TL_FULL; L.stack_i[0] = N;
        u32 sp = 1;
        while (sp > 0u && sp <= 8u) {
            --sp;
            const u32 S = L.stack_s[sp], idx = L.stack_i[sp];
            const u32 P = L.part[S], Q = S ^ P;
            const bool p_leafy = (P & (P - 1u)) == 0u, q_leafy = (Q & (Q - 1u)) == 0u;
            u32 kp, kq;
            if (p_leafy) kp = L.entry[__ffs(P) - 1]; else { kp = pick5(e, next); ++next; }
            if (q_leafy) kq = L.entry[__ffs(Q) - 1]; else { kq = pick5(e, next); ++next; }
            Box box = L.box[S];
            if (idx == N) box = nbox;                                                  // (the treelet root keeps its box: its leaf set is unchanged)
            node_store_agent(nodes + idx, kp, kq, box);
            if (kp < total) st_agent(parent + kp, idx);                                // (agent scope: the next round may climb on another XCD)
            if (kq < total) st_agent(parent + kq, idx);
            if (!q_leafy && sp < 8u) { L.stack_s[sp] = Q; L.stack_i[sp] = kq; ++sp; }
            if (!p_leafy && sp < 8u) { L.stack_s[sp] = P; L.stack_i[sp] = kp; ++sp; }
        }
    }
    wave_sync();                                                                      // (the next treelet of this wave reuses L)
}

template <int LAYOUT>
__global__ __launch_bounds__(OPT_BLOCK) void k_optimize(bvh2_node* nodes, const bvh_primref* __restrict__ leaves, u32* parent, u32* flags, u32 n, u32 gamma) {
    __shared__ TreeletLds lds[OPT_WAVES];
    TreeletLds& L = lds[tid_x() / WAVE];
    const u32 lane = tid_x() % WAVE;
    const u32 j = bid_x() * OPT_BLOCK + tid_x();
    const u32 ni = n - 1;
    // no lane returns early: every treelet is restructured by all 64 lanes of the wave that reached it
    bool active = j < n;
    u32 cur = ni + j, cnt = 1;
    for (;;) {
        bool ready = false;
        if (active) {
            const u32 p = ld_agent(parent + cur);
            if (p >= ni) {
                active = false;
            } else {
                drain_stores();                         // this wave's rebuilds below are complete before the exchange publishes the subtree
                const u32 sib = __hip_atomic_exchange(flags + p, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (sib == INV) {
                    active = false;
                } else {
                    st_agent(flags + p, INV);
                    compiler_fence();
                    cnt += sib; cur = p;
                    ready = cnt >= gamma;
                }
            }
        }
        for (u64 todo = __ballot(ready); todo; todo &= todo - 1ull) {
            const u32 root = rl(cur, (u32)__builtin_ctzll(todo));
            restructure<LAYOUT>(L, lane, root, nodes, leaves, parent, ni);
        }
        if (__ballot(active) == 0ull) break;
    }
}

void launch_optimize(hipStream_t s, void* d_nodes, const void* d_leaves, int layout, uint32_t n, uint32_t gamma, uint32_t* d_parent, uint32_t* d_flags) {
    const u32 blocks = (n + OPT_BLOCK - 1) / OPT_BLOCK;
    KernelScope ks(s, "k_optimize");
    if (layout == 0) hipLaunchKernelGGL(k_optimize<0>, dim3(blocks), dim3(OPT_BLOCK), 0, s, (bvh2_node*)d_nodes, (const bvh_primref*)d_leaves, d_parent, d_flags, n, gamma);
    else             hipLaunchKernelGGL(k_optimize<1>, dim3(blocks), dim3(OPT_BLOCK), 0, s, (bvh2_node*)d_nodes, (const bvh_primref*)d_leaves, d_parent, d_flags, n, gamma);
}

void warm_optimize() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_optimize<0>)); }

} // namespace bvh
