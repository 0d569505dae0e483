// morton.hpp — the extended Morton code of stage M as device functions: the per-scene bit plan (make_plan) and the per-primitive quantise / interleave (encode).
// Shared by stage_em.hip (k_morton, k_morton64's plan) and many.hip (the batched small-mesh kernels), so that the codes of one mesh cannot differ between the two.
// Only for translation units compiled with the default flags (Makefile): no -fno-honor-nans, -ffp-contract=off.
#pragma once
#include "common.hpp"

namespace bvh {

struct MortonPlan { int axis[3]; int bits[3]; int pre[2]; int pre_sum; int swap; };

__device__ __forceinline__ int sat_f2i(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return (int)f;
}
__device__ __forceinline__ u32 sat_f2u(float f) {
    if (f != f) return 0u;
    if (f <= 0.0f) return 0u;
    if (f >= 4294967296.0f) return 0xFFFFFFFFu;
    return (u32)f;
}
__device__ __forceinline__ int lg_ratio(float num, float den) { return sat_f2i(log2f(num / den)); }

// NB: total bit budget of the code — 30 in the reference (:161); 60 for the u64 keys of SURVEY.md §8(f) row 3 (same arithmetic)
__device__ void make_plan(const float* __restrict__ scene, MortonPlan& m, float* lo, float* ext, const u32 NB = 30u) {
    lo[0] = scene[0]; lo[1] = scene[1]; lo[2] = scene[2];
    const float ex = scene[3] - scene[0], ey = scene[4] - scene[1], ez = scene[5] - scene[2];
    ext[0] = ex; ext[1] = ey; ext[2] = ez;
    int px, py, pz;
    // axis order by extent; the strict '<' chain of src/CommonBlocksKernel.h:167-250 decides ties
    if (ex < ey) {
        if (ex < ez) {
            if (ey < ez) { m.axis[0] = 2; m.axis[1] = 1; m.axis[2] = 0; px = lg_ratio(ez, ey); py = lg_ratio(ey, ex); pz = lg_ratio(ez, ex); }
            else         { m.axis[0] = 1; m.axis[1] = 2; m.axis[2] = 0; px = lg_ratio(ey, ez); py = lg_ratio(ez, ex); pz = lg_ratio(ey, ex); }
        } else           { m.axis[0] = 1; m.axis[1] = 0; m.axis[2] = 2; px = lg_ratio(ey, ex); py = lg_ratio(ex, ez); pz = lg_ratio(ey, ez); }
    } else {
        if (ey < ez) {
            if (ex < ez) { m.axis[0] = 2; m.axis[1] = 0; m.axis[2] = 1; px = lg_ratio(ez, ex); py = lg_ratio(ex, ey); pz = lg_ratio(ez, ey); }
            else         { m.axis[0] = 0; m.axis[1] = 2; m.axis[2] = 1; px = lg_ratio(ex, ez); py = lg_ratio(ez, ey); pz = lg_ratio(ex, ey); }
        } else           { m.axis[0] = 0; m.axis[1] = 1; m.axis[2] = 2; px = lg_ratio(ex, ey); py = lg_ratio(ey, ez); pz = lg_ratio(ex, ez); }
    }
    int swap = (int)((u32)pz - ((u32)px + (u32)py));                                   // :252
    px = (int)fmin((double)px, (double)NB);                                            // :254
    py = (int)(fmin((double)(int)((u32)py * 2u), (double)(NB - (u32)px)) / 2.0);       // :255
    int sum = (int)((u32)px + (u32)py * 2u);                                           // :257
    if (sum != (int)NB) sum = (int)((u32)sum + (u32)swap); else swap = 0;              // :259-262
    const int bz = (ext[m.axis[2]] != 0.0f) ? (int)fmax(0.0, (double)((NB - (u32)sum) / 3u)) : 0;   // :264
    int bx, by;
    if (swap > 0) { bx = (int)fmax(0.0, (double)((NB - (u32)bz - (u32)sum) / 2u + (u32)py + (u32)px + 1u)); by = (int)(NB - (u32)bx - (u32)bz); }   // :266-270
    else          { by = (int)fmax(0.0, (double)((NB - (u32)bz - (u32)sum) / 2u + (u32)py));                 bx = (int)(NB - (u32)by - (u32)bz); }   // :271-275
    m.bits[0] = bx; m.bits[1] = by; m.bits[2] = bz; m.pre[0] = px; m.pre[1] = py; m.pre_sum = sum; m.swap = swap;
}

__device__ __forceinline__ u32 spread2(u32 v) {   // morton2D, :139-147
    v &= 0x0000ffffu; v = (v ^ (v << 8)) & 0x00ff00ffu; v = (v ^ (v << 4)) & 0x0f0f0f0fu;
    v = (v ^ (v << 2)) & 0x33333333u; v = (v ^ (v << 1)) & 0x55555555u; return v;
}
__device__ __forceinline__ u32 spread3(u32 x) {   // morton3D, :149-156
    x = (x * 0x00010001u) & 0xFF0000FFu; x = (x * 0x00000101u) & 0x0F00F00Fu;
    x = (x * 0x00000011u) & 0xC30C30C3u; x = (x * 0x00000005u) & 0x49249249u; return x;
}
__device__ __forceinline__ u32 shl(u32 v, u32 s) { return s >= 32u ? 0u : v << s; }
__device__ __forceinline__ u32 shr(u32 v, u32 s) { return s >= 32u ? 0u : v >> s; }

__device__ __forceinline__ u32 encode(const MortonPlan& m, float p0, float p1, float p2) {   // :277-358; p_k = position on axis[k]
    int bx = m.bits[0], by = m.bits[1];
    const int bz = m.bits[2], px = m.pre[0], py = m.pre[1];
    u32 q0 = min(sat_f2u(fmaxf(p0 * (float)shl(1u, (u32)bx), 0.0f)), shl(1u, (u32)bx) - 1u);
    u32 q1 = min(sat_f2u(fmaxf(p1 * (float)shl(1u, (u32)by), 0.0f)), shl(1u, (u32)by) - 1u);
    u32 q2 = min(sat_f2u(fmaxf(p2 * (float)shl(1u, (u32)bz), 0.0f)), shl(1u, (u32)bz) - 1u);
    u32 code = 0, d0 = 0, d1 = 0;
    if (m.pre_sum > 0) {
        bx -= px;
        code = shr(q0 & shl(shl(1u, (u32)px) - 1u, (u32)bx), (u32)bx);
        code = shl(code, (u32)(py * 2));
        bx -= py; by -= py;
        const u32 t0 = spread2(shr(q0 & shl(shl(1u, (u32)py) - 1u, (u32)bx), (u32)bx));
        const u32 t1 = spread2(shr(q1 & shl(shl(1u, (u32)py) - 1u, (u32)by), (u32)by));
        code |= t0 * 2 + t1;
        if (m.swap > 0) { code <<= 1; bx -= 1; code |= shr(q0 & shl(1u, (u32)bx), (u32)bx); }
        code = shl(code, (u32)(bx + by + bz));
        q0 &= shl(1u, (u32)bx) - 1u;
        q1 &= shl(1u, (u32)by) - 1u;
        if (m.swap > 0) { d0 = (u32)(by - bx); q0 = shl(q0, d0); d1 = (u32)(by - bz); q2 = shl(q2, d1); }
        else            { d0 = (u32)(bx - by); q1 = shl(q1, d0); d1 = (u32)(bx - bz); q2 = shl(q2, d1); }
    }
    if (bz == 0) code |= spread2(q0) * 2 + spread2(q1);
    else {
        const u32 X = spread3(q0), Y = spread3(q1), Z = spread3(q2);
        code |= shr((m.swap > 0) ? (Y * 4 + X * 2 + Z) : (X * 4 + Y * 2 + Z), d0 + d1);
    }
    return code;
}

} // namespace bvh
