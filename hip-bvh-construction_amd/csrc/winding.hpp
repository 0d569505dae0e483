// winding.hpp — device helpers shared by the winding-number kernels (winding.hip: bvh_winding_prepare / bvh_winding_number; scene_winding.hip: their scene
// forms): the seven sums of a subtree and their hand-over inside a climb, the leaf values, the Van Oosterom–Strackee solid angle, the dipole term, the point
// load and the answer store.  Compiled with -ffp-contract=off and WITHOUT -fno-honor-nans (Makefile): every expression is the header's, operation for
// operation, and the opening test and the area test must be false on NaN.
#pragma once
#include "query.hpp"

namespace bvh {

constexpr int WIND_BLOCK = 256;
constexpr float WIND_4PI = 12.566370614359172f;               // 4 pi rounded to f32
constexpr float WIND_THIRD = 1.0f / 3.0f;
constexpr u32 WIND_NAN = 0x7FC00000u;                         // the NaN every NaN answer is stored as

// the seven sums of a subtree: area vector, area, first moment (area-weighted centroid sum)
struct WSum { float ax, ay, az, area, mx, my, mz; };
__device__ __forceinline__ WSum wsum_add(const WSum& l, const WSum& r) {
    return { l.ax + r.ax, l.ay + r.ay, l.az + r.az, l.area + r.area, l.mx + r.mx, l.my + r.my, l.mz + r.mz };
}
// a leaf's values from its triangle (a, b, c = v1, v2, v3); a primitive index out of range — never in a tree — contributes nothing
template <int FMT>
__device__ __forceinline__ WSum wsum_leaf(const TriSrc& src, u32 prim, u32 n) {
    if (prim >= n) return { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    QF3 a, b, c; tri_fetch<FMT>(src, prim, a, b, c);
    const QF3 x = qcross(qsub(b, a), qsub(c, a));
    const float ax = 0.5f * x.x, ay = 0.5f * x.y, az = 0.5f * x.z;
    const float area = sqrtf((ax * ax + ay * ay) + az * az);
    const float cx = ((a.x + b.x) + c.x) * WIND_THIRD, cy = ((a.y + b.y) + c.y) * WIND_THIRD, cz = ((a.z + b.z) + c.z) * WIND_THIRD;
    return { ax, ay, az, area, area * cx, area * cy, area * cz };
}
// a moment record handed between workgroups inside the climb: two 16-byte write-through stores / L1-bypassing loads (common.hpp node_store_agent, rec_load_agent)
__device__ __forceinline__ void wsum_store_agent(bvh_winding_moment* m, const WSum& s) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f q0 = { s.ax, s.ay, s.az, s.area };
    const v4f q1 = { s.mx, s.my, s.mz, 0.0f };
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\tglobal_store_dwordx4 %0, %2, off offset:16 sc1\n\ts_nop 1" :: "v"(m), "v"(q0), "v"(q1) : "memory");
}
__device__ __forceinline__ WSum wsum_load_agent(const bvh_winding_moment* m) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f q0, q1;
    asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %2, off offset:16 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(q0), "=&v"(q1) : "v"(m) : "memory");
    return { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z };
}

// the primitive of leaf c (combined index space: leaf j at ni + j)
template <int LAYOUT>
__device__ __forceinline__ u32 leaf_prim(const bvh2_node* __restrict__ nodes, const bvh_primref* __restrict__ leaves, u32 c, u32 ni) {
    return LAYOUT == 0 ? nodes[c].left : leaves[c - ni].prim_idx;
}

// k_winding_finish's step on one record: the raw sums {A, area, M} -> {A, area, p, r} with p = M / area (the centre of box b when area is 0 or non-finite) and
// r = the distance from p to the farthest corner of b
__device__ __forceinline__ float wind_radius(const Box& b, float px, float py, float pz) {
    const float x = fmaxf(fabsf(b.lx - px), fabsf(b.hx - px)), y = fmaxf(fabsf(b.ly - py), fabsf(b.hy - py)), z = fmaxf(fabsf(b.lz - pz), fabsf(b.hz - pz));
    return sqrtf((x * x + y * y) + z * z);
}
__device__ __forceinline__ void wind_finish(bvh_winding_moment* mom, const Box& b) {
    float4* m = reinterpret_cast<float4*>(mom);
    const float4 s0 = m[0], s1 = m[1];
    const float area = s0.w;
    float px, py, pz;
    if (area != 0.0f && isfinite(area)) { px = s1.x / area; py = s1.y / area; pz = s1.z / area; }
    else { px = (b.lx + b.hx) * 0.5f; py = (b.ly + b.hy) * 0.5f; pz = (b.lz + b.hz) * 0.5f; }
    m[1] = make_float4(px, py, pz, wind_radius(b, px, py, pz));
}

// the Van Oosterom–Strackee solid angle of triangle (a, b, c) seen from q, over 4 pi
__device__ __forceinline__ float wind_solid_angle(QF3 a, QF3 b, QF3 c, QF3 q) {
    a = qsub(a, q); b = qsub(b, q); c = qsub(c, q);
    const float num = qdot(a, qcross(b, c));
    const float la = sqrtf(qdot(a, a)), lb = sqrtf(qdot(b, b)), lc = sqrtf(qdot(c, c));
    const float den = (((la * lb) * lc + qdot(a, b) * lc) + qdot(b, c) * la) + qdot(c, a) * lb;
    return (2.0f * atan2f(num, den)) / WIND_4PI;
}
// a node with area vector A, centre p and radius r seen from q: true with its dipole term iff it is approximated (false on NaN: +inf beta opens everything)
__device__ __forceinline__ bool wind_dipole(QF3 A, QF3 p, float r, QF3 q, float beta, float& term) {
    const QF3 d = { p.x - q.x, p.y - q.y, p.z - q.z };
    const float d2 = (d.x * d.x + d.y * d.y) + d.z * d.z, t = beta * r;
    if (!(d2 > t * t)) return false;
    term = qdot(A, d) / ((WIND_4PI * d2) * sqrtf(d2));
    return true;
}
// internal node c of the record array mom, as it stands
__device__ __forceinline__ bool wind_far(const bvh_winding_moment* __restrict__ mom, u32 c, QF3 q, float beta, float& term) {
    const float4* m = reinterpret_cast<const float4*>(mom + c);
    const float4 m0 = m[0], m1 = m[1];
    return wind_dipole(QF3{ m0.x, m0.y, m0.z }, QF3{ m1.x, m1.y, m1.z }, m1.w, q, beta, term);
}
__device__ __forceinline__ bool wind_point_load(const bvh_point_query* pts, u32 i, QF3& q) {
    const float4 a = reinterpret_cast<const float4*>(pts)[i];
    q = { a.x, a.y, a.z };
    return !(isnan(a.x) || isnan(a.y) || isnan(a.z));             // (the radius is not read)
}
__device__ __forceinline__ void wind_store(float* w, u32 i, double acc) {
    const float v = (float)acc;
    reinterpret_cast<u32*>(w)[i] = isnan(v) ? WIND_NAN : __float_as_uint(v);
}

} // namespace bvh
