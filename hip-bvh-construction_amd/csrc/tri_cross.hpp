// tri_cross.hpp — the crossing predicate of bvh_intersect_tris (the header's contract), shared by intersect_tris.hip (tree-side triangles in
// object space), scene_tris.hip (tree-side triangles mapped to world space) and closest_tris.hip (bvh_closest_tris's distance-0 case): IEEE f64 on the f32 coordinates widened exactly, no contraction
// (-ffp-contract=off), no reassociation; strict comparisons only; both triangles must be proper (tt_proper).  The coordinates stay in f32 registers and are
// widened where a difference is formed: two triangles held in f64 would be 36 more VGPRs for values that cost one v_cvt_f64_f32 each to remake.
#pragma once
#include "query.hpp"

namespace bvh {

// orient(a, b, c, d): the determinant of the rows a - d, b - d, c - d, expanded along the first row, the three terms summed left to right
__device__ __forceinline__ double tt_orient(QF3 a, QF3 b, QF3 c, QF3 d) {
    const double dx = (double)d.x, dy = (double)d.y, dz = (double)d.z;
    const double adx = (double)a.x - dx, ady = (double)a.y - dy, adz = (double)a.z - dz;
    const double bdx = (double)b.x - dx, bdy = (double)b.y - dy, bdz = (double)b.z - dz;
    const double cdx = (double)c.x - dx, cdy = (double)c.y - dy, cdz = (double)c.z - dz;
    return (adx * (bdy * cdz - bdz * cdy) + ady * (bdz * cdx - bdx * cdz)) + adz * (bdx * cdy - bdy * cdx);
}

// edge_crosses(p, q; a, b, c) given the plane sides sp = orient(a, b, c, p) and sq = orient(a, b, c, q): the end points strictly on opposite sides and the
// edge's line strictly inside all three edges of (a, b, c).  A zero or a NaN anywhere: false
__device__ __forceinline__ bool tt_edge(QF3 p, QF3 q, double sp, double sq, QF3 a, QF3 b, QF3 c) {
    if (!((sp > 0.0 && sq < 0.0) || (sp < 0.0 && sq > 0.0))) return false;
    const double o1 = tt_orient(p, q, a, b), o2 = tt_orient(p, q, b, c), o3 = tt_orient(p, q, c, a);
    return (o1 > 0.0 && o2 > 0.0 && o3 > 0.0) || (o1 < 0.0 && o2 < 0.0 && o3 < 0.0);
}

// proper(T): no coordinate is a NaN and the normal (v2 - v1) x (v3 - v1) has a component that is strictly positive or strictly negative.  The determinants alone
// do not keep such triangles out: an edge of a zero-area triangle is still a segment, and an edge between two clean vertices of a triangle whose third vertex
// holds a NaN is one too, and either can pass through the other triangle's interior (tests/test_intersect_tris.py has the cases)
__device__ __forceinline__ bool tt_proper(QF3 a, QF3 b, QF3 c) {
    const bool numbers = a.x == a.x && a.y == a.y && a.z == a.z && b.x == b.x && b.y == b.y && b.z == b.z && c.x == c.x && c.y == c.y && c.z == c.z;
    const double ux = (double)b.x - (double)a.x, uy = (double)b.y - (double)a.y, uz = (double)b.z - (double)a.z;
    const double wx = (double)c.x - (double)a.x, wy = (double)c.y - (double)a.y, wz = (double)c.z - (double)a.z;
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    return numbers && (nx > 0.0 || nx < 0.0 || ny > 0.0 || ny < 0.0 || nz > 0.0 || nz < 0.0);
}

// the determinants of crosses(X, Y) for two proper triangles: an edge of X crosses Y or an edge of Y crosses X; each plane side once per vertex
__device__ __forceinline__ bool tt_crosses(QF3 x1, QF3 x2, QF3 x3, QF3 y1, QF3 y2, QF3 y3) {
    {
        const double s1 = tt_orient(y1, y2, y3, x1), s2 = tt_orient(y1, y2, y3, x2), s3 = tt_orient(y1, y2, y3, x3);
        if (tt_edge(x1, x2, s1, s2, y1, y2, y3) || tt_edge(x2, x3, s2, s3, y1, y2, y3) || tt_edge(x3, x1, s3, s1, y1, y2, y3)) return true;
    }
    const double t1 = tt_orient(x1, x2, x3, y1), t2 = tt_orient(x1, x2, x3, y2), t3 = tt_orient(x1, x2, x3, y3);
    return tt_edge(y1, y2, t1, t2, x1, x2, x3) || tt_edge(y2, y3, t2, t3, x1, x2, x3) || tt_edge(y3, y1, t3, t1, x1, x2, x3);
}

__device__ __forceinline__ Box tt_box(QF3 a, QF3 b, QF3 c) { return stage_e_box(a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z); }

} // namespace bvh
