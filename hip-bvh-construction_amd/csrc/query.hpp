// query.hpp — device helpers shared by the query kernels (query.hip: bvh_intersect; scene.hip: bvh_scene_intersect; point_query.hip: bvh_closest_point; closest_tris.hip: bvh_closest_tris): the
// hit test, the closest-point formula, the conservative box tests, record / triangle / ray / point loads.  Compiled with -ffp-contract=off (Makefile): tri_hit is the reference's intersectTriangle operation for operation.
#pragma once
#include "bvh_mi355x.h"
#include "common.hpp"

namespace bvh {

constexpr int QUERY_BLOCK = 64;                // one wave per workgroup
constexpr int QUERY_STACK = 64;                // short-stack entries per lane, entry k of lane l at s_stack[k * QUERY_BLOCK + l] (16 KiB of LDS per wave)
constexpr u32 QUERY_DEEP_BLOCKS = 1024;        // k_intersect_deep's grid (grid-stride over the rays: an idle launch is 1024 workgroups that read one word)
constexpr u32 QUERY_MARK = 0xFFFFFFFEu;        // prim_idx of a ray left to k_intersect_deep (never a primitive: n < 2^30)
constexpr float QUERY_GROW = 0x1p-16f;         // absolute box growth on every axis, times the box's largest |coordinate| (a box flat at 0 still grows)
constexpr float QUERY_REL = 0x1p-20f;          // relative widening of the slab interval's ends (~16 ulp; the slab arithmetic errs by < 5 ulp)

struct QF3 { float x, y, z; };
__device__ __forceinline__ QF3 qsub(QF3 a, QF3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ QF3 qadd(QF3 a, QF3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
__device__ __forceinline__ float qdot(QF3 a, QF3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ QF3 qcross(QF3 a, QF3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }

struct QRay { QF3 o, d, inv; float tmin, tmax; bool nx, ny, nz; };   // n*: direction component has its sign bit set (planes swap)

// intersectTriangle (src/Common.h:516-531) operation for operation (file built with -ffp-contract=off): true with {it, iu, iv} iff iu, iv, iw > 0.  The four
// divisions are skipped when a sign already rules the hit out (iu > 0 needs u != 0 with the sign of den; NaN operands fall through to the divisions).
__device__ __forceinline__ bool tri_hit(QF3 v0, QF3 v1, QF3 v2, const QRay& r, float& it, float& iu, float& iv) {
    const QF3 p0 = qsub(v0, r.o), p1 = qsub(v1, r.o), p2 = qsub(v2, r.o), e0 = qsub(v2, v0), e1 = qsub(v0, v1), e2 = qsub(v1, v2);
    const QF3 nrm = qcross(e1, e0);
    const float u = qdot(qcross(qadd(p0, p2), e0), r.d), v = qdot(qcross(qadd(p1, p0), e1), r.d), w = qdot(qcross(qadd(p2, p1), e2), r.d);
    const float tt = qdot(p0, nrm) * 2.0f, den = qdot(nrm, r.d) * 2.0f;
    const u32 sd = __float_as_uint(den) >> 31;
    if (u == 0.0f || v == 0.0f || w == 0.0f || (__float_as_uint(u) >> 31) != sd || (__float_as_uint(v) >> 31) != sd || (__float_as_uint(w) >> 31) != sd) return false;
    iu = u / den; iv = v / den; it = tt / den;
    const float iw = w / den;
    return iu > 0.0f && iv > 0.0f && iw > 0.0f;
}

// the vertices of primitive `prim` (< n) in format FMT (bvh_tri_format)
struct TriSrc { const void* tris; const float* verts; const u32* idx; u32 nv; };
template <int FMT>
__device__ __forceinline__ void tri_fetch(const TriSrc& s, u32 prim, QF3& a, QF3& b, QF3& c) {
    if (FMT == BVH_TRI_PADDED64) {
        const float4* t = reinterpret_cast<const float4*>(s.tris) + 4 * (size_t)prim;
        const float4 q0 = t[0], q1 = t[1];
        const float q2 = reinterpret_cast<const float*>(t + 2)[0];
        a = { q0.x, q0.y, q0.z }; b = { q0.w, q1.x, q1.y }; c = { q1.z, q1.w, q2 };
    } else if (FMT == BVH_TRI_PACKED36) {
        const float* t = reinterpret_cast<const float*>(s.tris) + 9 * (size_t)prim;
        a = { t[0], t[1], t[2] }; b = { t[3], t[4], t[5] }; c = { t[6], t[7], t[8] };
    } else {
        const u32* ix = s.idx + 3 * (size_t)prim;
        u32 i0 = ix[0], i1 = ix[1], i2 = ix[2];
        i0 = i0 < s.nv ? i0 : 0u; i1 = i1 < s.nv ? i1 : 0u; i2 = i2 < s.nv ? i2 : 0u;       // (as stage E: an index out of range reads vertex 0)
        const float* p = s.verts + 3 * (size_t)i0; a = { p[0], p[1], p[2] };
        p = s.verts + 3 * (size_t)i1; b = { p[0], p[1], p[2] };
        p = s.verts + 3 * (size_t)i2; c = { p[0], p[1], p[2] };
    }
}

// how far every plane of box b moves out in a conservative test: QUERY_GROW times the box's largest |coordinate| (the one statement of it: DESIGN.md §8b, §8e, §8n)
__device__ __forceinline__ float box_grow(const Box& b) {
    return QUERY_GROW * fmaxf(fmaxf(fmaxf(fabsf(b.lx), fabsf(b.hx)), fmaxf(fabsf(b.ly), fabsf(b.hy))), fmaxf(fabsf(b.lz), fabsf(b.hz)));
}

// conservative slab test of box b against [tmin, best]: true iff the box may hold an accepted hit; tn_out = the interval's (unwidened) entry for ordering
__device__ __forceinline__ bool box_pass(const Box& b, const QRay& r, float best, float& tn_out) {
    const float g = box_grow(b);
    const float lx = b.lx - g, ly = b.ly - g, lz = b.lz - g, hx = b.hx + g, hy = b.hy + g, hz = b.hz + g;
    const float tnx = ((r.nx ? hx : lx) - r.o.x) * r.inv.x, tfx = ((r.nx ? lx : hx) - r.o.x) * r.inv.x;
    const float tny = ((r.ny ? hy : ly) - r.o.y) * r.inv.y, tfy = ((r.ny ? ly : hy) - r.o.y) * r.inv.y;
    const float tnz = ((r.nz ? hz : lz) - r.o.z) * r.inv.z, tfz = ((r.nz ? lz : hz) - r.o.z) * r.inv.z;
    const float tn = fmaxf(fmaxf(fmaxf(tnx, tny), tnz), r.tmin), tf = fminf(fminf(fminf(tfx, tfy), tfz), best);
    tn_out = tn;
    return fmaf(-QUERY_REL, fabsf(tn), tn) <= fmaf(QUERY_REL, fabsf(tf), tf);
}

// one record of the combined index space {internal [0, ni), leaf j at ni + j}: w0 = left link / leaf prim, w1 = right link (internal only)
template <int LAYOUT>
__device__ __forceinline__ void rec_fetch(const bvh2_node* __restrict__ nodes, const bvh_primref* __restrict__ leaves, u32 c, u32 ni, u32& w0, u32& w1, Box& b) {
    if (LAYOUT == 0 || c < ni) {
        const float4* q = reinterpret_cast<const float4*>(nodes + c);
        const float4 q0 = q[0], q1 = q[1];
        w0 = __float_as_uint(q0.x); w1 = __float_as_uint(q0.y);
        b = { q0.z, q0.w, q1.x, q1.y, q1.z, q1.w };
    } else {
        const bvh_primref* p = leaves + (c - ni);                  // (28-byte records: 4-byte loads)
        w0 = p->prim_idx; w1 = INV;
        b = box_load_u(&p->aabb);
    }
}

// ---- point queries (point_query.hip: bvh_closest_point) ----------------------------------------------------------------------------------------------------
constexpr float PQUERY_REL = 0x1p-20f;        // relative slack of the box lower bound (the f32 squared distance errs by < 6 ulp, 2^-20 is 16)

// Ericson's ClosestPtPointTriangle (Real-Time Collision Detection, 5.1.5) with a = v1, b = v2, c = v3, operation for operation (file built with -ffp-contract=off),
// regions in Ericson's order A, B, AB, C, AC, BC, interior.  Writes the closest point q and the weights (u, v) of b and c; returns dist2 = |p - q|^2.
__device__ __forceinline__ float tri_closest(QF3 a, QF3 b, QF3 c, QF3 p, QF3& q, float& u, float& v) {
    const QF3 ab = qsub(b, a), ac = qsub(c, a), ap = qsub(p, a);
    const float d1 = qdot(ab, ap), d2 = qdot(ac, ap);
    if (d1 <= 0.0f && d2 <= 0.0f) { q = a; u = 0.0f; v = 0.0f; }
    else {
        const QF3 bp = qsub(p, b);
        const float d3 = qdot(ab, bp), d4 = qdot(ac, bp);
        const float vc = d1 * d4 - d3 * d2;
        if (d3 >= 0.0f && d4 <= d3) { q = b; u = 1.0f; v = 0.0f; }
        else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
            const float t = d1 / (d1 - d3);
            q = { a.x + t * ab.x, a.y + t * ab.y, a.z + t * ab.z }; u = t; v = 0.0f;
        } else {
            const QF3 cp = qsub(p, c);
            const float d5 = qdot(ab, cp), d6 = qdot(ac, cp);
            const float vb = d5 * d2 - d1 * d6;
            if (d6 >= 0.0f && d5 <= d6) { q = c; u = 0.0f; v = 1.0f; }
            else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
                const float w = d2 / (d2 - d6);
                q = { a.x + w * ac.x, a.y + w * ac.y, a.z + w * ac.z }; u = 0.0f; v = w;
            } else {
                const float va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6;
                if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {
                    const float w = e43 / (e43 + e56);
                    q = { b.x + w * (c.x - b.x), b.y + w * (c.y - b.y), b.z + w * (c.z - b.z) }; u = 1.0f - w; v = w;
                } else {
                    const float denom = 1.0f / ((va + vb) + vc), tv = vb * denom, tw = vc * denom;
                    q = { (a.x + ab.x * tv) + ac.x * tw, (a.y + ab.y * tv) + ac.y * tw, (a.z + ab.z * tv) + ac.z * tw }; u = tv; v = tw;
                }
            }
        }
    }
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// conservative distance test of box b against best (a squared distance): true iff the box may hold an accepted candidate; lb_out = the
// grown box's f32 squared distance, for ordering.  The box grows as in box_pass; fmaxf drops the NaN of a NaN or infinite plane (the axis then costs 0).
__device__ __forceinline__ bool box_dist_pass(const Box& b, QF3 p, float best, float& lb_out) {
    const float g = box_grow(b);
    const float dx = fmaxf(fmaxf((b.lx - g) - p.x, p.x - (b.hx + g)), 0.0f);
    const float dy = fmaxf(fmaxf((b.ly - g) - p.y, p.y - (b.hy + g)), 0.0f);
    const float dz = fmaxf(fmaxf((b.lz - g) - p.z, p.z - (b.hz + g)), 0.0f);
    const float lb = (dx * dx + dy * dy) + dz * dz;
    lb_out = lb;
    return lb * (1.0f - PQUERY_REL) <= best;
}

// a query box grown once for box_box_dist_pass: every plane moves out by QUERY_GROW * (the box's largest |coordinate|), as box_dist_pass grows a node box
__device__ __forceinline__ Box box_grown(const Box& b) {
    const float g = box_grow(b);
    return { b.lx - g, b.ly - g, b.lz - g, b.hx + g, b.hy + g, b.hz + g };
}

// box_dist_pass for a query that is itself a box (closest_tris.hip: bvh_closest_tris): qg = the query's box, already grown (box_grown); b grows
// here.  The per-axis gap is the larger of the two one-sided gaps, or 0 where the intervals overlap; lb_out = the f32 sum of the squared gaps, for ordering.
// fmaxf drops the NaN of a NaN or infinite plane (the axis then costs 0).  True iff the box may hold an accepted candidate
__device__ __forceinline__ bool box_box_dist_pass(const Box& b, const Box& qg, float best, float& lb_out) {
    const float g = box_grow(b);
    const float dx = fmaxf(fmaxf((b.lx - g) - qg.hx, qg.lx - (b.hx + g)), 0.0f);
    const float dy = fmaxf(fmaxf((b.ly - g) - qg.hy, qg.ly - (b.hy + g)), 0.0f);
    const float dz = fmaxf(fmaxf((b.lz - g) - qg.hz, qg.lz - (b.hz + g)), 0.0f);
    const float lb = (dx * dx + dy * dy) + dz * dz;
    lb_out = lb;
    return lb * (1.0f - PQUERY_REL) <= best;
}

// ---- box queries (overlap.hip: bvh_overlap) -----------------------------------------------------------------------------------------------------------------
// closed, non-empty boxes: comparisons only, no arithmetic, so nothing is conservative here.  Touching boxes overlap, -0 == +0, a NaN anywhere fails, and an
// inverted box (a min above its max: the empty set, such as the reset box) overlaps nothing.  Monotone under containment: a box that contains a passing box
// passes, which is all the traversal needs.
__device__ __forceinline__ bool box_valid(const Box& b) { return b.lx <= b.hx && b.ly <= b.hy && b.lz <= b.hz; }
__device__ __forceinline__ bool box_overlap(const Box& q, const Box& b) {
    return q.lx <= b.hx && b.lx <= q.hx && q.ly <= b.hy && b.ly <= q.hy && q.lz <= b.hz && b.lz <= q.hz && box_valid(q) && box_valid(b);
}

// one bvh_point_query: true iff it is live (no NaN coordinate, radius >= 0); r2 = radius * radius either way (the miss record's dist2)
__device__ __forceinline__ bool point_load(const bvh_point_query* pts, u32 i, QF3& p, float& r2) {
    const float4 a = reinterpret_cast<const float4*>(pts)[i];
    p = { a.x, a.y, a.z }; r2 = a.w * a.w;
    return !(isnan(a.x) || isnan(a.y) || isnan(a.z)) && a.w >= 0.0f;   // (a NaN radius fails the comparison)
}

__device__ __forceinline__ bool ray_load(const bvh_ray* rays, u32 i, QRay& r) {
    const float4* q = reinterpret_cast<const float4*>(rays + i);
    const float4 a = q[0], c = q[1];
    r.o = { a.x, a.y, a.z }; r.d = { a.w, c.x, c.y }; r.tmin = c.z; r.tmax = c.w;
    r.inv = { 1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z };
    r.nx = __float_as_uint(r.d.x) >> 31; r.ny = __float_as_uint(r.d.y) >> 31; r.nz = __float_as_uint(r.d.z) >> 31;
    const bool nan = isnan(a.x) || isnan(a.y) || isnan(a.z) || isnan(a.w) || isnan(c.x) || isnan(c.y);
    return !nan && r.tmin < r.tmax;                               // (NaN tmin / tmax fail the comparison)
}

// ---- instanced scenes (scene.hip: bvh_scene_intersect; scene_point.hip: bvh_scene_closest_point) -----------------------------------------------------------
constexpr u32 SCENE_BLAS_ENTRY = 0x80000000u;   // stack entry of a BLAS node (top-level entries are plain indices: n < 2^30)
// a 3x4 row-major matrix applied to a point, in the order the header states
__device__ __forceinline__ QF3 xf_point(const float* m, float x, float y, float z) {
    return { ((m[0] * x + m[1] * y) + m[2] * z) + m[3], ((m[4] * x + m[5] * y) + m[6] * z) + m[7], ((m[8] * x + m[9] * y) + m[10] * z) + m[11] };
}
// rec_fetch with the layout chosen at run time (uniform per tree)
__device__ __forceinline__ void rec_fetch_rt(int layout, const void* nodes, const void* leaves, u32 c, u32 ni, u32& w0, u32& w1, Box& b) {
    if (layout == 0) rec_fetch<0>(reinterpret_cast<const bvh2_node*>(nodes), nullptr, c, ni, w0, w1, b);
    else rec_fetch<1>(reinterpret_cast<const bvh2_node*>(nodes), reinterpret_cast<const bvh_primref*>(leaves), c, ni, w0, w1, b);
}
// tri_fetch with the format chosen at run time (uniform per mesh: over a launch for a query mesh, per BLAS in a scene)
__device__ __forceinline__ void tri_fetch_rt(int fmt, const TriSrc& s, u32 prim, QF3& a, QF3& b, QF3& c) {
    if (fmt == BVH_TRI_PADDED64) tri_fetch<BVH_TRI_PADDED64>(s, prim, a, b, c);
    else if (fmt == BVH_TRI_PACKED36) tri_fetch<BVH_TRI_PACKED36>(s, prim, a, b, c);
    else tri_fetch<BVH_TRI_INDEXED>(s, prim, a, b, c);
}

} // namespace bvh
