// closest_tris.hpp — what the mesh-to-mesh distance files share (closest_tris.hip: bvh_closest_tris; scene_closest_tris.hip: bvh_scene_closest_tris;
// radius_tris.hip: bvh_radius_tris, which takes tt_dist2 and tris_query_load and keeps records of its own): the
// exact candidate of a triangle pair (tt_dist2: the header's dist2(X, Y) and feature, restated in numpy by tests/test_closest_tris.py), the flat query's record
// and the load of one query triangle.  The candidate is a value of the two triangles alone, so the scene form gets it by passing the WORLD triangle as Y.
// Every file that includes this is built with -ffp-contract=off and without the SLP vectoriser (Makefile): the formulas are stated operation for operation.
#pragma once
#include "query.hpp"
#include "tri_cross.hpp"

namespace bvh {

// the best candidate so far: dist2, prim (INV: none), feature
struct TBest { float d2; u32 prim, feat; };

__device__ __forceinline__ QF3 tt_pick(u32 k, QF3 a, QF3 b, QF3 c) { return k == 0u ? a : (k == 1u ? b : c); }
__device__ __forceinline__ bool tt_numbers(QF3 a, QF3 b, QF3 c) {
    return a.x == a.x && a.y == a.y && a.z == a.z && b.x == b.x && b.y == b.y && b.z == b.z && c.x == c.x && c.y == c.y && c.z == c.z;
}
__device__ __forceinline__ float tt_clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }    // (Ericson's Clamp: a NaN passes through)

// Ericson's ClosestPtSegmentSegment (Real-Time Collision Detection, 5.1.9) for the segments (p1, q1) and (p2, q2), operation for operation (file built with
// -ffp-contract=off), the EPSILON tests as exact tests against 0: returns the squared distance between the two clamped points
__device__ __forceinline__ float seg_seg_dist2(QF3 p1, QF3 q1, QF3 p2, QF3 q2) {
    const QF3 d1 = qsub(q1, p1), d2 = qsub(q2, p2), r = qsub(p1, p2);
    const float a = qdot(d1, d1), e = qdot(d2, d2), f = qdot(d2, r);
    float s = 0.0f, t = 0.0f;
    if (a <= 0.0f && e <= 0.0f) { }                               // both segments are points
    else if (a <= 0.0f) t = tt_clamp01(f / e);                    // the first is a point
    else {
        const float c = qdot(d1, r);
        if (e <= 0.0f) s = tt_clamp01(-c / a);                    // the second is a point
        else {
            const float b = qdot(d1, d2);
            const float denom = a * e - b * b;
            if (denom != 0.0f) s = tt_clamp01((b * f - c * e) / denom);
            t = (b * s + f) / e;
            if (t < 0.0f) { t = 0.0f; s = tt_clamp01(-c / a); }
            else if (t > 1.0f) { t = 1.0f; s = tt_clamp01((b - c) / a); }
        }
    }
    const float wx = (p1.x + d1.x * s) - (p2.x + d2.x * t), wy = (p1.y + d1.y * s) - (p2.y + d2.y * t), wz = (p1.z + d1.z * s) - (p2.z + d2.z * t);
    return (wx * wx + wy * wy) + wz * wz;
}

// dist2(X, Y) and its feature, in the header's order: NaN rule, crossing, X's vertices against Y, Y's against X, the nine edge pairs.  xb / yb: the two stage-E
// boxes; xproper: tt_proper(X), computed once per query.  The minimum starts at +inf and is replaced by a strictly smaller term only: a NaN term never wins and
// the lowest index that attains the minimum is kept
__device__ __forceinline__ float tt_dist2(QF3 x1, QF3 x2, QF3 x3, bool xproper, const Box& xb, QF3 y1, QF3 y2, QF3 y3, const Box& yb, u32& feat) {
    feat = 0u;
    if (!tt_numbers(y1, y2, y3)) return __uint_as_float(0x7FC00000u);     // (the query's own coordinates were checked when it was loaded)
    if (xproper && box_overlap(xb, yb) && tt_proper(y1, y2, y3) && tt_crosses(x1, x2, x3, y1, y2, y3)) { feat = 15u; return 0.0f; }
    float m = __uint_as_float(0x7F800000u);
#pragma unroll 1
    for (u32 k = 0; k < 6u; ++k) {                                // features 0..2: X's vertex k against Y; 3..5: Y's vertex k - 3 against X
        const bool rev = k >= 3u;
        const u32 kk = rev ? k - 3u : k;
        const QF3 p = rev ? tt_pick(kk, y1, y2, y3) : tt_pick(kk, x1, x2, x3);
        const QF3 a = rev ? x1 : y1, b = rev ? x2 : y2, c = rev ? x3 : y3;
        QF3 q; float u, v;
        const float d = tri_closest(a, b, c, p, q, u, v);
        if (d < m) { m = d; feat = k; }
        if (m == 0.0f) return m;
    }
#pragma unroll 1
    for (u32 e = 0; e < 9u; ++e) {                                // feature 6 + 3 * i + j: edge i of X against edge j of Y, edges (v1,v2), (v2,v3), (v3,v1)
        const u32 i = e / 3u, j = e - 3u * i;
        const float d = seg_seg_dist2(tt_pick(i, x1, x2, x3), tt_pick(i, x2, x3, x1), tt_pick(j, y1, y2, y3), tt_pick(j, y2, y3, y1));
        if (d < m) { m = d; feat = 6u + e; }
        if (m == 0.0f) return m;
    }
    return m;
}

__device__ __forceinline__ void tri_hit_store(bvh_tri_hit* hits, u32 i, const TBest& b) {
    reinterpret_cast<uint4*>(hits + i)[0] = make_uint4(__float_as_uint(b.d2), b.prim, b.feat, 0u);
}

// one query triangle: its vertices, whether it is live (no NaN coordinate, radius >= 0; a NaN radius fails the comparison) and r2 = radius * radius either way
__device__ __forceinline__ bool tris_query_load(int qfmt, const TriSrc& qsrc, u32 i, float radius, QF3& x1, QF3& x2, QF3& x3, float& r2) {
    tri_fetch_rt(qfmt, qsrc, i, x1, x2, x3);
    r2 = radius * radius;
    return tt_numbers(x1, x2, x3) && radius >= 0.0f;
}

} // namespace bvh
