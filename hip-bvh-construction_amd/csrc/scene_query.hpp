// scene_query.hpp — what the scene queries that walk an instance in OBJECT space share (scene.hip: bvh_scene_intersect; scene_multihit.hip:
// bvh_scene_intersect_all; scene_point.hip: bvh_scene_closest_point; scene_knn.hip: bvh_scene_knn; scene_radius.hip: bvh_scene_radius_search;
// scene_closest_tris.hip: bvh_scene_closest_tris; scene_winding.hip: bvh_scene_winding_number) and scene_map.hpp builds on: an instance's matrices, a BLAS's
// triangle and its world triangle, the entry of a ray or a point into an instance, and the point queries' conservative box test
//   a node box of instance k against the mapped point p' = W_k p: grown on every axis by box_grow + e,  e = 2^-20 max_i(((|w_i0||px| + |w_i1||py|) + |w_i2||pz|) + |w_i3|),
//   culled iff s2 * lb' * (1 - 2^-20) > bound.
// Every one is a numerical contract stated once: count and fill passes, and closest / knn / radius answers, agree because they run the same lines.  All in f32
// without contraction, in the order written (every file that includes this is built with -ffp-contract=off and without the SLP vectoriser, Makefile).
#pragma once
#include "query.hpp"
#include "kernels.hpp"

namespace bvh {

// three rows of a 3x4 matrix as loaded, and the same as the row-major float[12] that xf_point takes
struct SOMat { float4 r0, r1, r2; };
__device__ __forceinline__ void mat_rows(const SOMat& M, float* m) {
    m[0] = M.r0.x; m[1] = M.r0.y; m[2] = M.r0.z; m[3] = M.r0.w; m[4] = M.r1.x; m[5] = M.r1.y; m[6] = M.r1.z; m[7] = M.r1.w;
    m[8] = M.r2.x; m[9] = M.r2.y; m[10] = M.r2.z; m[11] = M.r2.w;
}
// the forward matrix of instance k (rows of object_to_world), from the scene's copy of the caller's records: 12 floats that L2 serves, re-loaded per leaf test
// by the walks that would otherwise keep 12 VGPRs live all the way
__device__ __forceinline__ SOMat inst_load_m(const SceneQuery& a, u32 k) {
    const float4* mq = reinterpret_cast<const float4*>(reinterpret_cast<const bvh_instance*>(a.inst_in) + k);
    return { mq[0], mq[1], mq[2] };
}

// tri_fetch with the BLAS's format chosen at run time (uniform per instance)
__device__ __forceinline__ void blas_tri_fetch(const SceneBlas& B, u32 prim, QF3& a, QF3& b, QF3& c) {
    const TriSrc src{ B.tris, reinterpret_cast<const float*>(B.tris), reinterpret_cast<const u32*>(B.idx), B.nv };
    tri_fetch_rt((int)B.fmt, src, prim, a, b, c);
}
// the world triangle of (inst, prim), prim < B.n: the BLAS's vertices mapped by the instance's forward matrix, in xf_point's order
__device__ __forceinline__ void blas_world_tri(const SceneQuery& a, const SceneBlas& B, u32 prim, u32 inst, QF3& wa, QF3& wb, QF3& wc) {
    QF3 v1, v2, v3;
    blas_tri_fetch(B, prim, v1, v2, v3);
    float m[12];
    mat_rows(inst_load_m(a, inst), m);
    wa = xf_point(m, v1.x, v1.y, v1.z); wb = xf_point(m, v2.x, v2.y, v2.z); wc = xf_point(m, v3.x, v3.y, v3.z);
}

// the world ray w in instance k's object space (tmin / tmax kept); false: inactive instance
__device__ __forceinline__ bool enter_instance_ray(const SceneQuery& a, u32 k, const QRay& w, QRay& r, SceneBlas& B) {
    const float4* q = reinterpret_cast<const float4*>(a.inst + k);
    const u32 bl = __float_as_uint(q[3].x);
    if (bl == INV) return false;
    float m[12];
    mat_rows({ q[0], q[1], q[2] }, m);
    B = a.blas[bl];
    r.o = xf_point(m, w.o.x, w.o.y, w.o.z);
    r.d = { (m[0] * w.d.x + m[1] * w.d.y) + m[2] * w.d.z, (m[4] * w.d.x + m[5] * w.d.y) + m[6] * w.d.z, (m[8] * w.d.x + m[9] * w.d.y) + m[10] * w.d.z };
    r.inv = { 1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z };
    r.nx = __float_as_uint(r.d.x) >> 31; r.ny = __float_as_uint(r.d.y) >> 31; r.nz = __float_as_uint(r.d.z) >> 31;
    r.tmin = w.tmin; r.tmax = w.tmax;
    return true;
}

// ---- point queries ------------------------------------------------------------------------------------------------------------------------------------------------
// the query point on the level the walk is on: the world point with e = 0, s2 = 1, or instance k's object-space point with its slack and scale bound
struct ScenePoint { QF3 p; float e, s2; };

// box_dist_pass on either level: at the top it is the same test with e = 0 and s2 = 1 (1 * lb and g + 0 are exact, lb is never NaN)
__device__ __forceinline__ bool scene_box_dist_pass(const Box& b, const ScenePoint& c, float bound, float& lb_out) {
    const float g = box_grow(b) + c.e;
    const float dx = fmaxf(fmaxf((b.lx - g) - c.p.x, c.p.x - (b.hx + g)), 0.0f);
    const float dy = fmaxf(fmaxf((b.ly - g) - c.p.y, c.p.y - (b.hy + g)), 0.0f);
    const float dz = fmaxf(fmaxf((b.lz - g) - c.p.z, c.p.z - (b.hz + g)), 0.0f);
    const float lb = (dx * dx + dy * dy) + dz * dz;
    lb_out = lb;
    return !((c.s2 * lb) * (1.0f - PQUERY_REL) > bound);         // (a NaN product never culls)
}
// ... for a walk that does not order its children by the lower bound
__device__ __forceinline__ bool scene_box_dist_pass(const Box& b, const ScenePoint& c, float bound) { float lb; return scene_box_dist_pass(b, c, bound, lb); }

// the slack e of one world point w against the rows of W (m = world_to_object): 2^-20 of the largest row of |W| (|w|, 1)
__device__ __forceinline__ float scene_slack(const float* m, QF3 w) {
    const float ax = fabsf(w.x), ay = fabsf(w.y), az = fabsf(w.z);
    const float r0 = ((fabsf(m[0]) * ax + fabsf(m[1]) * ay) + fabsf(m[2]) * az) + fabsf(m[3]);
    const float r1 = ((fabsf(m[4]) * ax + fabsf(m[5]) * ay) + fabsf(m[6]) * az) + fabsf(m[7]);
    const float r2 = ((fabsf(m[8]) * ax + fabsf(m[9]) * ay) + fabsf(m[10]) * az) + fabsf(m[11]);
    return 0x1p-20f * fmaxf(fmaxf(r0, r1), r2);
}

// the world point w in instance k's object space, with its slack, scale bound and BLAS; false: inactive instance
__device__ __forceinline__ bool enter_instance_point(const SceneQuery& a, u32 k, QF3 w, ScenePoint& c, SceneBlas& B) {
    const float4* q = reinterpret_cast<const float4*>(a.inst + k);
    const float4 q3 = q[3];
    const u32 bl = __float_as_uint(q3.x);
    if (bl == INV) return false;
    float m[12];
    mat_rows({ q[0], q[1], q[2] }, m);
    B = a.blas[bl];
    c.p = xf_point(m, w.x, w.y, w.z);
    c.e = scene_slack(m, w);
    c.s2 = q3.y;
    return true;
}

} // namespace bvh
