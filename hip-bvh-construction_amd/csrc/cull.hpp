// cull.hpp — what the convex-volume queries share (cull.hip: bvh_cull; scene_cull.hip: bvh_scene_cull): one volume's planes, and the header's box test against
// them, operation for operation: every product and sum one round-to-nearest f32 operation (__fmul_rn / __fadd_rn: never contracted), monotone under box
// containment in rounded f32, so the answer is exact for every volume.  Every file that includes this is built without the SLP vectoriser
// (Makefile).
#pragma once
#include "query.hpp"

namespace bvh {

constexpr int CULL_PLANES = BVH_CULL_MAX_PLANES;
static_assert(CULL_PLANES == 8, "the straddle mask has one bit per plane");

// one volume's planes, component-wise.  Planes at and above the call's planes_per_volume are never read and never tested (np is uniform over a launch: the
// unrolled loops below keep their `k < np` guards as scalar branches, and every array index is a constant, so nothing here lives in scratch)
// pa / pb / pc: which coordinate of a box each coefficient multiplies (plane_pick below), worked out once where the planes are made
struct Planes { float a[CULL_PLANES], b[CULL_PLANES], c[CULL_PLANES], d[CULL_PLANES], pa[CULL_PLANES], pb[CULL_PLANES], pc[CULL_PLANES]; };

// the p-vertex's pick of a coefficient, as a number for v_med3_f32 (see plane_s): +inf for a coefficient > 0, -inf for one < 0 or a NaN, 0 for +-0.  (The empty
// asm keeps ONE pick per coefficient: the n-vertex's negation then is a source modifier of v_med3_f32, not a second set of 24 selected values)
__device__ __forceinline__ float plane_pick(float coef) { float p = coef > 0.0f ? INFINITY : (coef == 0.0f ? 0.0f : -INFINITY); asm("" : "+v"(p)); return p; }
__device__ __forceinline__ void planes_pick(Planes& P) {
#pragma unroll
    for (int k = 0; k < CULL_PLANES; ++k) { P.pa[k] = plane_pick(P.a[k]); P.pb[k] = plane_pick(P.b[k]); P.pc[k] = plane_pick(P.c[k]); }
}

__device__ __forceinline__ Planes planes_load(const float* __restrict__ p, u32 np) {
    Planes P;
#pragma unroll
    for (int k = 0; k < CULL_PLANES; ++k) {
        const bool on = (u32)k < np;
        P.a[k] = on ? p[4 * k + 0] : 0.0f; P.b[k] = on ? p[4 * k + 1] : 0.0f; P.c[k] = on ? p[4 * k + 2] : 0.0f; P.d[k] = on ? p[4 * k + 3] : 1.0f;
    }
    planes_pick(P);
    return P;
}

// s(v) of the header: ((a x + b y) + c z) + d, four products and sums rounded one by one.  A coefficient of +-0 contributes a zero whatever the coordinate (0 * inf
// would be a NaN: padding and axis-aligned planes stay immune to infinite box planes); a NaN coefficient is not zero and still gives a NaN.
//
// The fast form, for a box with lo < +inf and hi > -inf on every axis (every box this library makes: stage E keeps lo <= FLT_MAX and hi >= -FLT_MAX): the vertex
// coordinate is v_med3_f32(lo, hi, pick) with pick = +inf for a coefficient > 0 (takes hi), -inf for one < 0 or a NaN (takes lo, as the select `coef >= 0 ? hi :
// lo` does) and 0 for a zero coefficient: the value of [lo, hi] nearest 0, which is finite there, so that the product is a zero (its sign never changes an
// `s >= 0`).  The n-vertex takes the negated pick.  One instruction per coordinate as the select was, and no lane mask per coefficient to keep in SGPRs.
// The plain form, for a box that lies at infinity on some axis (caller-filled arrays only): the select, and +0 in place of the product of a zero coefficient.
__device__ __forceinline__ bool box_at_infinity(const Box& b) {
    return b.lx == INFINITY || b.ly == INFINITY || b.lz == INFINITY || b.hx == -INFINITY || b.hy == -INFINITY || b.hz == -INFINITY;
}
// (the plain form reads every coefficient through an empty asm: its sign and zero tests then are the cold path's own work, not 48 loop-invariant lane masks
// that the walk would carry in SGPRs)
__device__ __forceinline__ float plane_opaque(float x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ float plane_term(float coef, float v) { return coef == 0.0f ? 0.0f : __fmul_rn(coef, v); }

template <bool PVERTEX> __device__ __forceinline__ float plane_s(const Planes& P, int k, const Box& b) {
    const float pa = P.pa[k], pb = P.pb[k], pc = P.pc[k];
    const float x = __builtin_amdgcn_fmed3f(b.lx, b.hx, PVERTEX ? pa : -pa);
    const float y = __builtin_amdgcn_fmed3f(b.ly, b.hy, PVERTEX ? pb : -pb);
    const float z = __builtin_amdgcn_fmed3f(b.lz, b.hz, PVERTEX ? pc : -pc);
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(P.a[k], x), __fmul_rn(P.b[k], y)), __fmul_rn(P.c[k], z)), P.d[k]);
}

template <bool PVERTEX> __device__ __forceinline__ float plane_s_plain(const Planes& P, int k, const Box& b) {
    const float pa = plane_opaque(P.a[k]), pb = plane_opaque(P.b[k]), pc = plane_opaque(P.c[k]);
    const float x = (pa >= 0.0f) == PVERTEX ? b.hx : b.lx, y = (pb >= 0.0f) == PVERTEX ? b.hy : b.ly, z = (pc >= 0.0f) == PVERTEX ? b.hz : b.lz;
    return __fadd_rn(__fadd_rn(__fadd_rn(plane_term(pa, x), plane_term(pb, y)), plane_term(pc, z)), P.d[k]);
}

// does box b pass the volume: valid, and s(p-vertex) >= 0 for every plane (a NaN fails: only inf - inf between nonzero terms, or a NaN input, makes one)
__device__ __forceinline__ bool cull_pass(const Planes& P, u32 np, const Box& b) {
    bool ok = box_valid(b);
    if (box_at_infinity(b)) {
#pragma unroll
        for (int k = 0; k < CULL_PLANES; ++k)
            if ((u32)k < np) ok = ok && plane_s_plain<true>(P, k, b) >= 0.0f;
        return ok;
    }
#pragma unroll
    for (int k = 0; k < CULL_PLANES; ++k)
        if ((u32)k < np) ok = ok && plane_s<true>(P, k, b) >= 0.0f;
    return ok;
}

// bit k: !(s(n-vertex of plane k) >= 0), the box is not wholly inside plane k.  Always from the box's own coordinates against all np planes
__device__ __forceinline__ u32 cull_straddle(const Planes& P, u32 np, const Box& b) {
    u32 m = 0;
    if (box_at_infinity(b)) {
#pragma unroll
        for (int k = 0; k < CULL_PLANES; ++k)
            if ((u32)k < np) m |= (plane_s_plain<false>(P, k, b) >= 0.0f ? 0u : 1u) << k;
        return m;
    }
#pragma unroll
    for (int k = 0; k < CULL_PLANES; ++k)
        if ((u32)k < np) m |= (plane_s<false>(P, k, b) >= 0.0f ? 0u : 1u) << k;
    return m;
}

} // namespace bvh
