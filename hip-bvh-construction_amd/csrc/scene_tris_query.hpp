// scene_tris_query.hpp — what the scene queries that ask with a TRIANGLE and walk an instance in object space share (scene_closest_tris.hip:
// bvh_scene_closest_tris; scene_radius_tris.hip: bvh_scene_radius_tris): the query side of a launch, the query's box on either level, the conservative box test
// and the entry of a query triangle into an instance.
//   a node box of instance k against the mapped triangle x'_i = W_k x_i: the componentwise min/max box of the x'_i, grown on every axis by
//   QUERY_GROW * (its largest |coordinate|) + e,  e = the largest of the point queries' slack (scene_slack, scene_query.hpp) over the three vertices;
//   the node box grown by QUERY_GROW * (its largest |coordinate|);   culled iff s2 * lb' * (1 - 2^-20) > bound.
// The top level is the same test with s2 = 1 on the world boxes, the query's stage-E box grown once.  Every one is a numerical contract stated once: the nearest
// record and the radius set agree because they run the same lines.  All in f32 without contraction, in the order written (every file that includes this is
// built with -ffp-contract=off and without the SLP vectoriser, Makefile).
#pragma once
#include "query.hpp"
#include "tri_cross.hpp"
#include "closest_tris.hpp"
#include "scene_map.hpp"
#include "kernels.hpp"

namespace bvh {

// the query side of a launch: the caller's mesh and its format (QUERY mode), or the instance whose triangles ask (INSTANCE mode); the call's one radius
struct SCQuery { TriSrc src; int fmt; u32 inst; float radius; };
// the query's box on the level the walk is on, already grown: the world stage-E box with s2 = 1, or instance k's object-space box with its scale bound
struct SCBox { Box q; float s2; };
// what the stack walk keeps of the BLAS it is in: the arrays and sizes every step reads, and the BLAS's index for the leaf
struct SCWalk { const void* nodes; const void* leaves; u32 n, layout, bl; };

__device__ __forceinline__ bool scene_box_box_pass(const Box& b, const SCBox& c, float best, float& lb_out) {
    const float g = box_grow(b);
    const float dx = fmaxf(fmaxf((b.lx - g) - c.q.hx, c.q.lx - (b.hx + g)), 0.0f);
    const float dy = fmaxf(fmaxf((b.ly - g) - c.q.hy, c.q.ly - (b.hy + g)), 0.0f);
    const float dz = fmaxf(fmaxf((b.lz - g) - c.q.hz, c.q.lz - (b.hz + g)), 0.0f);
    const float lb = (dx * dx + dy * dy) + dz * dz;
    lb_out = lb;
    return !((c.s2 * lb) * (1.0f - PQUERY_REL) > best);          // (a NaN product never culls)
}

// the query's world box for the top level: its stage-E box grown once
__device__ __forceinline__ SCBox sc_world_box(QF3 x1, QF3 x2, QF3 x3) { return { box_grown(tt_box(x1, x2, x3)), 1.0f }; }

// the world query triangle in instance k's object space: its grown box, the instance's scale bound and BLAS; false: inactive instance
__device__ __forceinline__ bool enter_instance_tris(const SceneQuery& a, u32 k, QF3 x1, QF3 x2, QF3 x3, SCBox& c, SceneBlas& B, u32& bl_out) {
    const float4* q = reinterpret_cast<const float4*>(a.inst + k);
    const float4 q3 = q[3];
    const u32 bl = __float_as_uint(q3.x);
    if (bl == INV) return false;
    float m[12];
    mat_rows({ q[0], q[1], q[2] }, m);
    B = a.blas[bl]; bl_out = bl;
    const QF3 p1 = xf_point(m, x1.x, x1.y, x1.z), p2 = xf_point(m, x2.x, x2.y, x2.z), p3 = xf_point(m, x3.x, x3.y, x3.z);
    const float e = fmaxf(fmaxf(scene_slack(m, x1), scene_slack(m, x2)), scene_slack(m, x3));
    const Box o{ fminf(fminf(p1.x, p2.x), p3.x), fminf(fminf(p1.y, p2.y), p3.y), fminf(fminf(p1.z, p2.z), p3.z),
                 fmaxf(fmaxf(p1.x, p2.x), p3.x), fmaxf(fmaxf(p1.y, p2.y), p3.y), fmaxf(fmaxf(p1.z, p2.z), p3.z) };
    const float g = box_grow(o) + e;
    c.q = { o.lx - g, o.ly - g, o.lz - g, o.hx + g, o.hy + g, o.hz + g };
    c.s2 = q3.y;
    return true;
}

// query triangle i, whether it is live (asked, no NaN coordinate, radius >= 0; a NaN radius fails the comparison) and r2 = radius * radius either way.  A row
// that is not asked (INSTANCE mode: an inactive or out-of-range query instance, a row at or beyond its BLAS's n) misses
template <int MODE>
__device__ __forceinline__ bool sc_query_load(const SceneQuery& a, const SCQuery& t, u32 i, QF3& x1, QF3& x2, QF3& x3, float& r2) {
    r2 = t.radius * t.radius;
    if (MODE == BVH_SCENE_TRIS_QUERY) tri_fetch_rt(t.fmt, t.src, i, x1, x2, x3);
    else {
        SOMat M; SceneBlas B;
        if (t.inst >= a.n_inst || !sov_enter_instance(a, t.inst, M, B) || i >= B.n) return false;
        st_world_tri(B, M, i, x1, x2, x3);
    }
    return tt_numbers(x1, x2, x3) && t.radius >= 0.0f;
}

// may the walk enter instance k?  (INSTANCE mode: the query's own instance is skipped by index; a second instance of the same BLAS is another instance)
template <int MODE> __device__ __forceinline__ bool sc_may_enter(const SceneQuery& a, const SCQuery& t, u32 k) {
    return k < a.n_inst && (MODE != BVH_SCENE_TRIS_INSTANCE || k != t.inst);
}

} // namespace bvh
