// many_front.hpp — what the batched small-mesh kernels share (many.hip: LBVH emit, many_ploc.hip: PLOC++ emit): one mesh's stage E boxes, extent, bit plan and
// codes, and the rank sort of its {key, mesh-local index} words, all by a team of T threads (one wave, or one workgroup).  Every value comes from the device
// function the large-mesh pipeline uses — stage_e_box* (common.hpp), make_plan / encode (morton.hpp) — so the bytes are the pipeline's.
// Args: ManyArgs / ManyPlocArgs (kernels.hpp) — the fields read here are tris, verts, idx, n_verts, boxes, scenes.
#pragma once
#include "bvh_mi355x.h"
#include "common.hpp"
#include "morton.hpp"

namespace bvh {

// all threads of the mesh meet here: a workgroup barrier, or — one wave per mesh — nothing but ordering (a wave's LDS operations execute in order)
template <int T> __device__ __forceinline__ void many_sync() {
    if (T == WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else __syncthreads();
}

__device__ __forceinline__ Box wave_reduce_box_all(Box b) {           // every lane gets the union of the wave's boxes
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        b.lx = fminf(b.lx, __shfl_xor(b.lx, m)); b.ly = fminf(b.ly, __shfl_xor(b.ly, m)); b.lz = fminf(b.lz, __shfl_xor(b.lz, m));
        b.hx = fmaxf(b.hx, __shfl_xor(b.hx, m)); b.hy = fmaxf(b.hy, __shfl_xor(b.hy, m)); b.hz = fmaxf(b.hz, __shfl_xor(b.hz, m));
    }
    return b;
}

template <int FMT, class Args> __device__ __forceinline__ Box many_tri_box(const Args& a, u32 i) {
    if (FMT == BVH_TRI_PADDED64) return stage_e_box_padded((const float4*)a.tris, i);
    if (FMT == BVH_TRI_PACKED36) return stage_e_box9((const float*)a.tris + (size_t)i * 9);
    return stage_e_box_indexed((const float*)a.verts, (const u32*)a.idx, a.n_verts, i);
}

// Steps 1-4 of one mesh — triangles [it.x, it.x + it.y) of the input, output offset it.z, mesh id it.w; t = the thread's index inside the team (T >= it.y).
// Writes the thread's stage E box to a.boxes and (thread 0) the extent to a.scenes; bx = the box (the reset box for t >= it.y); returns the sort word
// {key : 32 | mesh-local index : 32} (0 for t >= it.y).  red: T / WAVE rows of LDS, one per wave (T > WAVE: holds a workgroup barrier).
template <int T, int FMT, class Args>
__device__ __forceinline__ u64 many_front(const Args& a, float (*red)[6], const uint4 it, const u32 t, Box& bx) {
    const u32 first = it.x, n = it.y, off = it.z, m = it.w;
    const bool act = t < n;
    // 1. stage E
    bx = box_empty();
    if (act) {
        bx = many_tri_box<FMT>(a, first + t);
        box_store(a.boxes + off + t, bx);
    }
    // 2. extent: fminf / fmaxf over the mesh's boxes, starting from the reset box (k_extents' atomics give the same value in any order)
    Box ext = wave_reduce_box_all(bx);
    if (T > WAVE) {
        const u32 w = t / WAVE;
        if ((t & (WAVE - 1)) == 0) { red[w][0] = ext.lx; red[w][1] = ext.ly; red[w][2] = ext.lz; red[w][3] = ext.hx; red[w][4] = ext.hy; red[w][5] = ext.hz; }
        many_sync<T>();
        ext = box_empty();
#pragma unroll
        for (int k = 0; k < T / WAVE; ++k) {
            const Box r = { red[k][0], red[k][1], red[k][2], red[k][3], red[k][4], red[k][5] };
            ext = box_union(ext, r);
        }
    }
    if (t == 0) box_store(a.scenes + m, ext);
    // 3. the mesh's bit plan (every lane evaluates the same values: as cheap as one lane doing it), 4. the code
    const float scene[6] = { ext.lx, ext.ly, ext.lz, ext.hx, ext.hy, ext.hz };
    MortonPlan mp; float lo[3], ex[3];
    make_plan(scene, mp, lo, ex);
    if (!act) return 0ull;
    const float p[3] = { ((bx.hx + bx.lx) * 0.5f - lo[0]) / ex[0], ((bx.hy + bx.ly) * 0.5f - lo[1]) / ex[1], ((bx.hz + bx.lz) * 0.5f - lo[2]) / ex[2] };   // k_morton's expression
    const u32 code = encode(mp, p[mp.axis[0]], p[mp.axis[1]], p[mp.axis[2]]);
    return ((u64)code << 32) | (u64)t;
}

// 5. sort: the position of `mine` is the number of smaller words among aug[0 .. n) — the words are distinct, so the rank IS the position of the stable sort
// (every lane reads the same word: an LDS broadcast)
__device__ __forceinline__ u32 many_rank(const u64* aug, const u32 n, const u64 mine) {
    u32 rank = 0u;
    for (u32 j = 0; j < n; ++j) rank += aug[j] < mine ? 1u : 0u;
    return rank;
}

} // namespace bvh
