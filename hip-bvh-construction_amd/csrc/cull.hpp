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
struct Planes { float a[CULL_PLANES], b[CULL_PLANES], c[CULL_PLANES], d[CULL_PLANES]; };

__device__ __forceinline__ Planes planes_load(const float* __restrict__ p, u32 np) {
    Planes P;
#pragma unroll
    for (int k = 0; k < CULL_PLANES; ++k) {
        const bool on = (u32)k < np;
        P.a[k] = on ? p[4 * k + 0] : 0.0f; P.b[k] = on ? p[4 * k + 1] : 0.0f; P.c[k] = on ? p[4 * k + 2] : 0.0f; P.d[k] = on ? p[4 * k + 3] : 1.0f;
    }
    return P;
}

// s(v) of the header: ((a x + b y) + c z) + d, four products and sums rounded one by one
__device__ __forceinline__ float plane_s(float a, float b, float c, float d, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)), __fmul_rn(c, z)), d);
}

// does box b pass the volume: valid, and s(p-vertex) >= 0 for every plane (a NaN fails)
__device__ __forceinline__ bool cull_pass(const Planes& P, u32 np, const Box& b) {
    bool ok = box_valid(b);
#pragma unroll
    for (int k = 0; k < CULL_PLANES; ++k)
        if ((u32)k < np) {
            const float s = plane_s(P.a[k], P.b[k], P.c[k], P.d[k], P.a[k] >= 0.0f ? b.hx : b.lx, P.b[k] >= 0.0f ? b.hy : b.ly, P.c[k] >= 0.0f ? b.hz : b.lz);
            ok = ok && s >= 0.0f;
        }
    return ok;
}

// bit k: !(s(n-vertex of plane k) >= 0), the box is not wholly inside plane k.  Always from the box's own coordinates against all np planes
__device__ __forceinline__ u32 cull_straddle(const Planes& P, u32 np, const Box& b) {
    u32 m = 0;
#pragma unroll
    for (int k = 0; k < CULL_PLANES; ++k)
        if ((u32)k < np) {
            const float s = plane_s(P.a[k], P.b[k], P.c[k], P.d[k], P.a[k] >= 0.0f ? b.lx : b.hx, P.b[k] >= 0.0f ? b.ly : b.hy, P.c[k] >= 0.0f ? b.lz : b.hz);
            m |= (s >= 0.0f ? 0u : 1u) << k;
        }
    return m;
}

} // namespace bvh
