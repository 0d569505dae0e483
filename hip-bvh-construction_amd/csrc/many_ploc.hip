// many_ploc.hip — bvh_build_many_ploc: the PLOC++ tree of every small mesh of a batch in one launch per size class (gfx950).
//
// many.hip's front (stage E box, extent, plan, code, rank sort: many_front.hpp) joined to the single-workgroup tail of the PLOC++ emit (ploc.hip: the tail branch of
// ploc_iter_body and ploc_tail_wave), which is what the ordinary build runs for a mesh of fewer than PLOC_CHUNK triangles.  A mesh of up to 64 triangles is one
// WAVE's work (several meshes share a workgroup, no workgroup barrier), a mesh of up to MANY_MAX triangles one workgroup's, one cluster per thread.
// One round is a pure function of the cluster list, so the bytes are the ordinary build's: nearest neighbour within +-8 list positions under the integer key
// {area bits of the union, position}, mutual pairs merge, the lower position owns the node, node index = c - 2 - (merges at lower positions), children
// {own id, neighbour id}, box = fminf / fmaxf union, survivors keep their order; leaf j is {svals[j], box} with cluster id (n - 1) + j.
//   list    : {id, box[6]} in LDS column arrays (a lane per column: conflict-free), compacted in place (read to registers, barrier, write to the rank)
//   search  : every pair (k, k + r), r = 1 .. 8, evaluated ONCE by thread k — 8 neighbour boxes read from LDS where reading both sides costs 16, the lever
//             ploc.hip's nn_pairs measured — the key minimised into the far end's word by an LDS atomic and into the own end's in registers (one atomic at the end).
//             Keys are compared as integers everywhere (ploc.hip keeps the own candidates as f64, which orders alike on the finite non-negative areas for which
//             identity is claimed): whatever an area's bits are, a round of c >= 2 clusters has a mutual pair — the lowest pair of the smallest key — and ends.
//   c <= 64 : the first wave finishes alone without barriers, ploc_tail_wave's scheme: neighbour boxes through a DPP wave_shl:1 chain, ballots for the ranks.
// No kernel waits on another wave or workgroup: inside a mesh only barriers (a wave-level fence on the wave path) and LDS atomics.
// Compiled with the default flags (Makefile), as many.hip: stage_e_box's clamp needs NaN semantics.  ploc.o is not (-fno-honor-nans -mno-amdgpu-ieee); the two
// agree on finite areas, which is where identity with the ordinary build is claimed.
#include "bvh_mi355x.h"
#include "common.hpp"
#include "kernels.hpp"
#include "many_front.hpp"

namespace bvh {

constexpr int MANY_PLOC_WAVES = 4;             // meshes per workgroup of the wave kernel
constexpr int MP_RADIUS = 8;                   // PlocRadius (ploc.hip PL_RADIUS)

// everything one mesh needs in LDS; T = most triangles.  T = 512: 22 752 bytes
template <int T> struct ManyPlocSmem {
    u64 aug[T];                    // {key : 32 | mesh-local index : 32} by primitive
    u64 nn[T];                     // per list position: nearest neighbour key {area bits : 32 | position : 32}
    float box[6][T];               // the cluster list: boxes ...
    u32 id[T];                     // ... and ids (leaf j: n - 1 + j, node i: i)
    float red[T / WAVE][6];        // extent: one row per wave
    u32 wsum[T / WAVE];            // block scan: one total per wave
};
static_assert(sizeof(ManyPlocSmem<MANY_MAX>) <= 65536, "the block kernel's LDS is static: at most 64 KB");
static_assert(2 * sizeof(ManyPlocSmem<MANY_MAX>) <= 160 * 1024, "two 512-thread workgroups fit a CU's 160 KB of LDS");

template <int T> __device__ __forceinline__ Box list_box(const ManyPlocSmem<T>& s, u32 k) { return { s.box[0][k], s.box[1][k], s.box[2][k], s.box[3][k], s.box[4][k], s.box[5][k] }; }
template <int T> __device__ __forceinline__ void list_set(ManyPlocSmem<T>& s, u32 k, u32 id, const Box& b) {
    s.id[k] = id; s.box[0][k] = b.lx; s.box[1][k] = b.ly; s.box[2][k] = b.lz; s.box[3][k] = b.hx; s.box[4][k] = b.hy; s.box[5][k] = b.hz;
}
__device__ __forceinline__ unsigned long long area_key(const Box& a, const Box& b) { return (unsigned long long)__float_as_uint(box_area(box_union(a, b))) << 32; }

// block-wide exclusive scan of a packed {merges << 16 | kept} per-thread count (ploc.hip block_scan); its first barrier also ends the round's reads of the list
template <int T> __device__ __forceinline__ u32 many_ploc_scan(u32* wsum, const u32 t, const u32 v, u32* total) {
    const u32 lane = t & (WAVE - 1), wave = t / WAVE;
    u32 inc = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) { const u32 u = (u32)__shfl_up((int)inc, off); if (lane >= (u32)off) inc += u; }
    __syncthreads();
    if (lane == WAVE - 1) wsum[wave] = inc;
    __syncthreads();
    u32 base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < T / WAVE; ++w) { const u32 c = wsum[w]; if ((u32)w < wave) base += c; tot += c; }
    *total = tot;
    return base + inc - v;
}

// The rounds of a list of c <= 64 clusters, one per lane of ONE wave, until a single cluster is left (ploc.hip ploc_tail_wave; own candidates as integers).
// The list in LDS is complete and ordered before the call.
template <int T>
__device__ __forceinline__ void many_ploc_wave_rounds(ManyPlocSmem<T>& s, u32 c, bvh2_node* __restrict__ nodes, const u32 lane) {
    u32 id = lane < c ? s.id[lane] : INV;
    Box b = lane < c ? list_box(s, lane) : box_empty();
    const u64 lt = lanemask_lt();
    while (c > 1u) {
        s.nn[lane] = ~0ull;
        many_sync<WAVE>();
        Box nb = b;
        unsigned long long own = ~0ull;
#pragma unroll
        for (int r = 1; r <= MP_RADIUS; ++r) {
            nb = box_shl1(nb);                             // box of position lane + r
            if (lane + r < c) {
                const unsigned long long key = area_key(nb, b);
                atomicMin(reinterpret_cast<unsigned long long*>(s.nn + lane + r), key | lane);
                const unsigned long long mine = key | (lane + r);
                own = mine < own ? mine : own;
            }
        }
        many_sync<WAVE>();
        const bool in = lane < c;
        const u64 left = s.nn[lane];
        const int nbr = in ? (int)(u32)(left < own ? left : own) : (int)lane;
        const bool mutual = in && (u32)__shfl(nbr, nbr) == lane;
        const bool merge = mutual && (int)lane < nbr, absorbed = mutual && (int)lane > nbr;
        const u32 id_nb = (u32)__shfl((int)id, nbr);
        const Box bn = shfl_box(b, nbr);
        const u64 mm = __ballot(merge);
        if (mm == 0ull) break;                             // (cannot happen, see above: end rather than spin if it ever did)
        if (merge) {
            b = box_union(b, bn);
            const u32 at = c - 2u - (u32)__popcll(mm & lt);
            node_store_plain(nodes + at, id, id_nb, b);
            id = at;
        }
        const bool keep = in && !absorbed;
        const u64 km = __ballot(keep);
        if (keep) list_set(s, (u32)__popcll(km & lt), id, b);
        c = (u32)__popcll(km);
        many_sync<WAVE>();
        id = lane < c ? s.id[lane] : INV;
        b = lane < c ? list_box(s, lane) : box_empty();
    }
}

// One mesh: triangles [it.x, it.x + it.y) of the input, output offset it.z, mesh id it.w.  t = the thread's index inside the mesh's team of T threads (T >= it.y).
template <int T, int FMT>
__device__ __forceinline__ void many_ploc_one(ManyPlocSmem<T>& sm, const ManyPlocArgs& a, const uint4 it, const u32 t) {
    const u32 n = it.y, off = it.z, m = it.w, ni = n - 1u;
    const bool act = t < n;
    // 1. stage E, 2. extent, 3. the mesh's bit plan, 4. the code (many_front.hpp)
    Box bx;
    const u64 mine = many_front<T, FMT>(a, sm.red, it, t, bx);
    if (act) sm.aug[t] = mine;
    sm.nn[t] = ~0ull;
    many_sync<T>();
    // 5. sort; the leaf of position `rank` holds primitive t: its PrimRef, and its entry of the first cluster list (SetupClusters: id = n - 1 + position)
    if (act) {
        const u32 rank = many_rank(sm.aug, n, mine);
        if (a.skeys) a.skeys[off + rank] = (u32)(mine >> 32);
        if (a.svals) a.svals[off + rank] = t;
        float* f = reinterpret_cast<float*>(a.leaves + off + rank);
        reinterpret_cast<u32*>(f)[0] = t;
        f[1] = bx.lx; f[2] = bx.ly; f[3] = bx.lz; f[4] = bx.hx; f[5] = bx.hy; f[6] = bx.hz;
        list_set(sm, rank, ni + rank, bx);
    }
    bvh2_node* const nodes = a.nodes + ((size_t)off - m);
    u32 c = n;
    if (T > WAVE) {
        // 6. rounds of the whole workgroup, thread t = list position t, while more than a wave's worth of clusters is left (ploc.hip:261-304)
        while (c > (u32)WAVE) {
            __syncthreads();                                                // the list is complete, every nn word is ~0
            const bool in = t < c;
            Box b = box_empty();
            if (in) {
                b = list_box(sm, t);
                unsigned long long own = ~0ull;
#pragma unroll
                for (u32 r = 1; r <= (u32)MP_RADIUS; ++r) {
                    if (t + r < c) {
                        const unsigned long long key = area_key(list_box(sm, t + r), b);
                        atomicMin(reinterpret_cast<unsigned long long*>(sm.nn + t + r), key | t);
                        const unsigned long long cand = key | (t + r);
                        own = cand < own ? cand : own;
                    }
                }
                if (t + 1u < c) atomicMin(reinterpret_cast<unsigned long long*>(sm.nn + t), own);
            }
            __syncthreads();
            bool mrg = false, keep = false;
            u32 cid = INV, pid = INV;
            if (in) {
                const u32 nb = (u32)sm.nn[t];
                const bool mutual = (u32)sm.nn[nb] == t;
                mrg = mutual && t < nb; keep = !mutual || mrg;
                cid = sm.id[t];
                if (mrg) { pid = sm.id[nb]; b = box_union(b, list_box(sm, nb)); }
            }
            u32 tot;
            const u32 ex = many_ploc_scan<T>(sm.wsum, t, ((u32)mrg << 16) + (u32)keep, &tot);
            if ((tot >> 16) == 0u) break;                                   // (cannot happen, see above; block-uniform)
            if (keep) {
                u32 id = cid;
                if (mrg) {
                    id = c - 2u - (ex >> 16);
                    node_store_plain(nodes + id, cid, pid, b);
                }
                list_set(sm, ex & 0xFFFFu, id, b);
            }
            sm.nn[t] = ~0ull;
            c = tot & 0xFFFFu;
        }
        __syncthreads();
        if (t >= (u32)WAVE || c > (u32)WAVE) return;
    } else many_sync<T>();
    // 7. the last rounds: one wave
    many_ploc_wave_rounds(sm, c, nodes, t);
}

// meshes of 2 .. 64 triangles: one wave each, MANY_PLOC_WAVES meshes per workgroup, no workgroup barrier
template <int FMT>
__global__ __launch_bounds__(MANY_PLOC_WAVES * WAVE) void k_many_ploc_wave(ManyPlocArgs a, const uint4* __restrict__ items, u32 n_items) {
    __shared__ ManyPlocSmem<WAVE> sm[MANY_PLOC_WAVES];
    const u32 w = threadIdx.x / WAVE, idx = blockIdx.x * MANY_PLOC_WAVES + w;
    if (idx >= n_items) return;                                             // (wave-uniform)
    many_ploc_one<WAVE, FMT>(sm[w], a, items[idx], threadIdx.x & (WAVE - 1));
}

// meshes of up to T triangles: one workgroup each
template <int T, int FMT>
__global__ __launch_bounds__(T) void k_many_ploc_block(ManyPlocArgs a, const uint4* __restrict__ items) {
    __shared__ ManyPlocSmem<T> sm;
    many_ploc_one<T, FMT>(sm, a, items[blockIdx.x], threadIdx.x);
}

template <int FMT>
static void launch_many_ploc_fmt(hipStream_t s, const ManyPlocArgs& a, const uint4* d_items, const uint32_t n_class[4]) {
    u32 at = 0;
    if (n_class[0]) {
        KernelScope ks(s, "k_many_ploc_wave");
        hipLaunchKernelGGL((k_many_ploc_wave<FMT>), dim3((n_class[0] + MANY_PLOC_WAVES - 1) / MANY_PLOC_WAVES), dim3(MANY_PLOC_WAVES * WAVE), 0, s, a, d_items, n_class[0]);
    }
    at += n_class[0];
    if (n_class[1]) { KernelScope ks(s, "k_many_ploc_block"); hipLaunchKernelGGL((k_many_ploc_block<128, FMT>), dim3(n_class[1]), dim3(128), 0, s, a, d_items + at); }
    at += n_class[1];
    if (n_class[2]) { KernelScope ks(s, "k_many_ploc_block"); hipLaunchKernelGGL((k_many_ploc_block<256, FMT>), dim3(n_class[2]), dim3(256), 0, s, a, d_items + at); }
    at += n_class[2];
    if (n_class[3]) { KernelScope ks(s, "k_many_ploc_block"); hipLaunchKernelGGL((k_many_ploc_block<MANY_MAX, FMT>), dim3(n_class[3]), dim3(MANY_MAX), 0, s, a, d_items + at); }
}

// d_items: as launch_many's
void launch_many_ploc(hipStream_t s, const ManyPlocArgs& a, int tri_format, const void* d_items, const uint32_t n_class[4]) {
    const uint4* items = (const uint4*)d_items;
    switch (tri_format) {
        case BVH_TRI_PADDED64: launch_many_ploc_fmt<BVH_TRI_PADDED64>(s, a, items, n_class); break;
        case BVH_TRI_PACKED36: launch_many_ploc_fmt<BVH_TRI_PACKED36>(s, a, items, n_class); break;
        default:               launch_many_ploc_fmt<BVH_TRI_INDEXED>(s, a, items, n_class); break;
    }
}

void warm_many_ploc() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_many_ploc_wave<BVH_TRI_PADDED64>)); }

} // namespace bvh
