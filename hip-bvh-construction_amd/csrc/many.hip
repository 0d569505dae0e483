// many.hip — bvh_build_many: the LBVH of every small mesh of a batch in one launch per size class (gfx950).
//
// What the reference's BatchedBuildKernelLbvh (src/BatchedBuildKernel.h:218-312) set out to be: one workgroup per mesh, extent, Morton code, sort and
// emit without leaving the CU.  Here a mesh of up to 64 triangles is one WAVE's work (several meshes share a workgroup, no workgroup barrier) and a mesh of
// up to MANY_MAX triangles one workgroup's; each tree is byte-identical to what the large-mesh pipeline (stage_em.hip, sort.hip, lbvh.hip) builds from that
// mesh alone, because every value is produced by the same device function: stage_e_box* (common.hpp), make_plan / encode (morton.hpp), plen (common.hpp).
//   sort  : rank of the 64-bit word {key, mesh-local index} among the mesh's words — the words are distinct, so the rank IS the position of the stable sort
//   emit  : k_lbvh_block's second-arriver climb (lbvh.hip) with the whole mesh as its one tile: a finished node parks its box in LDS and exchanges a word with
//           its sibling on the parent's gap; the second arriver goes on.  Node numbering as lbvh.hip:38-42, records rebuilt from LDS and stored whole (32 B).
// No kernel waits on another wave or workgroup: inside a mesh only barriers (a wave-level fence on the wave path) and LDS atomics.
// Compiled with the default flags (Makefile), as stage_em.hip: stage_e_box's clamp needs NaN semantics.
#include "bvh_mi355x.h"
#include "common.hpp"
#include "kernels.hpp"
#include "many_front.hpp"

namespace bvh {

constexpr int MANY_WAVES = 4;                   // meshes per workgroup of the wave kernel

// everything one mesh needs in LDS; T = most triangles.  T = 512: 50 368 bytes
template <int T> struct ManySmem {
    u64 aug[T];                    // {key : 32 | mesh-local index : 32} by primitive
    u64 slot[T];                   // per gap: hand-off word of the first arriver (slot_word), then the node's children {left | right << 32}
    u32 key[T];                    // sorted keys
    float pbox[6][T];              // stage E boxes by primitive
    float box[2][6][T];            // per gap: the box its left / right child parked
    unsigned short inv[T];         // two-pass numbering: node index -> gap whose node carries it
    float red[T / WAVE][6];        // extent: one row per wave
};

// One mesh: triangles [it.x, it.x + it.y) of the input, output offset it.z, mesh id it.w.  t = the thread's index inside the mesh's team of T threads (T >= it.y).
template <int T, int FMT, bool KARRAS>
__device__ __forceinline__ void many_build_one(ManySmem<T>& sm, const ManyArgs& a, const uint4 it, const u32 t) {
    const u32 n = it.y, off = it.z, m = it.w, ni = n - 1u;
    const bool act = t < n;
    // 1. stage E, 2. extent, 3. the mesh's bit plan, 4. the code (many_front.hpp)
    Box bx;
    const u64 mine = many_front<T, FMT>(a, sm.red, it, t, bx);
    if (act) {
        sm.pbox[0][t] = bx.lx; sm.pbox[1][t] = bx.ly; sm.pbox[2][t] = bx.lz; sm.pbox[3][t] = bx.hx; sm.pbox[4][t] = bx.hy; sm.pbox[5][t] = bx.hz;
        sm.aug[t] = mine;
    }
    sm.slot[t] = 0ull;
    many_sync<T>();
    // 5. sort: my position is the number of smaller words (every lane reads the same word: an LDS broadcast)
    if (act) {
        const u32 rank = many_rank(sm.aug, n, mine);
        sm.key[rank] = (u32)(mine >> 32);
        // the leaf of position `rank` holds primitive t.  (inv[] is the position -> primitive map until the climb starts)
        if (a.skeys) a.skeys[off + rank] = (u32)(mine >> 32);
        if (a.svals) a.svals[off + rank] = t;
        sm.inv[rank] = (unsigned short)t;
    }
    many_sync<T>();
    // 6. emit: thread t is the walker of the leaf at sorted position t
    bvh2_node* const nodes = a.nodes + (2ull * off - m);
    u32 prim = 0u;
    Box box = box_empty();
    if (act) {
        prim = sm.inv[t];
        box = { sm.pbox[0][prim], sm.pbox[1][prim], sm.pbox[2][prim], sm.pbox[3][prim], sm.pbox[4][prim], sm.pbox[5][prim] };
        node_store_plain(nodes + ni + t, prim, INV, box);                    // leaf record {left = primIdx, right = INVALID}
    }
    many_sync<T>();                                                         // (inv[] is reused by the two-pass numbering from here on)
    if (act) {
        u32 i = t, j = t + 1u, cur = ni + t, lc = 0u, rc = 0u;              // finished node `cur` covers sorted positions [i, j)
        bool leaf = true;
        while (true) {
            const bool root = i == 0u && j == n;
            bool as_left = true;                                            // findParent (src/SinglePassLbvhKernel.h:64-86); plen comparison == closer()
            if (!root) {
                if (i == 0u) as_left = true;
                else if (j == n) as_left = false;
                else as_left = plen(sm.key[j - 1u], j - 1u, sm.key[j], j) > plen(sm.key[i - 1u], i - 1u, sm.key[i], i);
            }
            if (KARRAS && !leaf) { const u32 gap = cur; cur = root ? 0u : (as_left ? j - 1u : i); sm.inv[cur] = (unsigned short)gap; }
            if (root) { a.roots[m] = cur; break; }
            const u32 p = as_left ? j - 1u : i - 1u;
            const int side = as_left ? 0 : 1;                               // park my box, then publish
            sm.box[side][0][p] = box.lx; sm.box[side][1][p] = box.ly; sm.box[side][2][p] = box.lz; sm.box[side][3][p] = box.hx; sm.box[side][4][p] = box.hy; sm.box[side][5][p] = box.hz;
            compiler_fence();
            const u64 other = atomicExch(reinterpret_cast<unsigned long long*>(&sm.slot[p]), (unsigned long long)(((u64)(cur + 1u) << 32) | (as_left ? i : j)));
            compiler_fence();
            if (other == 0ull) break;                                       // first arriver retires
            const u32 sib = (u32)(other >> 32) - 1u, far = (u32)other;
            const Box sb = { sm.box[1 - side][0][p], sm.box[1 - side][1][p], sm.box[1 - side][2][p], sm.box[1 - side][3][p], sm.box[1 - side][4][p], sm.box[1 - side][5][p] };
            box = box_union(box, sb);
            lc = as_left ? cur : sib; rc = as_left ? sib : cur; leaf = false;
            sm.slot[p] = (u64)lc | ((u64)rc << 32);                         // (the word has seen both arrivals: it now keeps the children)
            if (as_left) j = far; else i = far;
            cur = p;                                                        // (single-pass numbering; two-pass: decided next step)
        }
    }
    many_sync<T>();
    // 7. the internal records, one per thread in index order, whole 32-byte stores
    if (t < ni) {
        const u32 gap = KARRAS ? (u32)sm.inv[t] : t;
        const Box l = { sm.box[0][0][gap], sm.box[0][1][gap], sm.box[0][2][gap], sm.box[0][3][gap], sm.box[0][4][gap], sm.box[0][5][gap] };
        const Box r = { sm.box[1][0][gap], sm.box[1][1][gap], sm.box[1][2][gap], sm.box[1][3][gap], sm.box[1][4][gap], sm.box[1][5][gap] };
        const u64 ch = sm.slot[gap];
        node_store_plain(nodes + t, (u32)ch, (u32)(ch >> 32), box_union(l, r));
    }
}

// meshes of 2 .. 64 triangles: one wave each, MANY_WAVES meshes per workgroup, no workgroup barrier
template <int FMT, bool KARRAS>
__global__ __launch_bounds__(MANY_WAVES * WAVE) void k_many_wave(ManyArgs a, const uint4* __restrict__ items, u32 n_items) {
    __shared__ ManySmem<WAVE> sm[MANY_WAVES];
    const u32 w = threadIdx.x / WAVE, idx = blockIdx.x * MANY_WAVES + w;
    if (idx >= n_items) return;                                             // (wave-uniform)
    many_build_one<WAVE, FMT, KARRAS>(sm[w], a, items[idx], threadIdx.x & (WAVE - 1));
}

// meshes of up to T triangles: one workgroup each
template <int T, int FMT, bool KARRAS>
__global__ __launch_bounds__(T) void k_many_block(ManyArgs a, const uint4* __restrict__ items) {
    __shared__ ManySmem<T> sm;
    many_build_one<T, FMT, KARRAS>(sm, a, items[blockIdx.x], threadIdx.x);
}

static_assert(sizeof(ManySmem<MANY_MAX>) <= 65536, "the block kernel's LDS is static: at most 64 KB");

template <int FMT, bool KARRAS>
static void launch_many_fmt(hipStream_t s, const ManyArgs& a, const uint4* d_items, const uint32_t n_class[4]) {
    u32 at = 0;
    if (n_class[0]) {
        KernelScope ks(s, "k_many_wave");
        hipLaunchKernelGGL((k_many_wave<FMT, KARRAS>), dim3((n_class[0] + MANY_WAVES - 1) / MANY_WAVES), dim3(MANY_WAVES * WAVE), 0, s, a, d_items, n_class[0]);
    }
    at += n_class[0];
    if (n_class[1]) { KernelScope ks(s, "k_many_block"); hipLaunchKernelGGL((k_many_block<128, FMT, KARRAS>), dim3(n_class[1]), dim3(128), 0, s, a, d_items + at); }
    at += n_class[1];
    if (n_class[2]) { KernelScope ks(s, "k_many_block"); hipLaunchKernelGGL((k_many_block<256, FMT, KARRAS>), dim3(n_class[2]), dim3(256), 0, s, a, d_items + at); }
    at += n_class[2];
    if (n_class[3]) { KernelScope ks(s, "k_many_block"); hipLaunchKernelGGL((k_many_block<MANY_MAX, FMT, KARRAS>), dim3(n_class[3]), dim3(MANY_MAX), 0, s, a, d_items + at); }
}

// d_items: {first, count, out_off, mesh} records binned by the host — n_class[0] of at most 64 triangles, then n_class[1] of at most 128, n_class[2] of at most
// 256, n_class[3] of at most MANY_MAX.  karras: the two-pass builder's node numbering
void launch_many(hipStream_t s, const ManyArgs& a, int tri_format, bool karras, const void* d_items, const uint32_t n_class[4]) {
    const uint4* items = (const uint4*)d_items;
#define MANY_FMT(F) do { if (karras) launch_many_fmt<F, true>(s, a, items, n_class); else launch_many_fmt<F, false>(s, a, items, n_class); } while (0)
    switch (tri_format) {
        case BVH_TRI_PADDED64: MANY_FMT(BVH_TRI_PADDED64); break;
        case BVH_TRI_PACKED36: MANY_FMT(BVH_TRI_PACKED36); break;
        default:               MANY_FMT(BVH_TRI_INDEXED); break;
    }
#undef MANY_FMT
}

void warm_many() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_many_wave<BVH_TRI_PADDED64, true>)); }

} // namespace bvh
