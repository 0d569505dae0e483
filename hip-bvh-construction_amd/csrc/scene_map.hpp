// scene_map.hpp — what the set-valued scene queries that test MAPPED boxes share (scene_overlap.hip: bvh_scene_overlap; scene_tris.hip:
// bvh_scene_intersect_tris; scene_collide.hip: bvh_scene_collide): the forward matrix of the entered instance (SOMat, scene_query.hpp), the header's mapped box, the
// record sink and, for the two crossing-pair files, the world triangle of an instance's primitive.
//   mapped(M, {lo, hi}), row r:  a_c = m_rc * lo.c, b_c = m_rc * hi.c,  min.r = ((fminf(a_0, b_0) + fminf(a_1, b_1)) + fminf(a_2, b_2)) + m_r3,  max.r with fmaxf
// in f32 without contraction (every file that includes this is built with -ffp-contract=off and without the SLP vectoriser, Makefile).
#pragma once
#include "scene_query.hpp"
#include "tri_cross.hpp"

namespace bvh {

static_assert(sizeof(bvh_instance_prim) == sizeof(uint2), "a record leaves in one 8-byte store");

// where a walk's records go (overlap.hip's Sink for bvh_instance_prim records {prim, instance})
template <bool FILL, bool SORTED> struct SceneOverlapSink {
    uint2* out; u32 room, k = 0;
    __device__ __forceinline__ void put(u32 prim, u32 inst) {
        if (FILL) {
            if (k < room) {
                u32 j = k;
                if (SORTED) {
                    const u64 key = ((u64)inst << 32) | prim;
                    while (j > 0) {                               // (records above (inst, prim) move up by one; the slice below j + 1 stays sorted)
                        const uint2 p = out[j - 1];
                        if ((((u64)p.y << 32) | p.x) < key) break;
                        out[j] = p; --j;
                    }
                }
                out[j] = make_uint2(prim, inst);
            }
        }
        if (k < QUERY_MARK - 1u) ++k;                             // (many instances of one BLAS can answer: the counter saturates below the mark)
    }
};

// one row of the mapped box, in the header's order
__device__ __forceinline__ void sov_row(const float4 m, const Box& b, float& lo, float& hi) {
    const float a0 = m.x * b.lx, b0 = m.x * b.hx, a1 = m.y * b.ly, b1 = m.y * b.hy, a2 = m.z * b.lz, b2 = m.z * b.hz;
    lo = ((fminf(a0, b0) + fminf(a1, b1)) + fminf(a2, b2)) + m.w;
    hi = ((fmaxf(a0, b0) + fmaxf(a1, b1)) + fmaxf(a2, b2)) + m.w;
}

// the contract's test of object box b of the entered instance against world query box q: b valid, and q overlaps mapped(M, b)
__device__ __forceinline__ bool sov_box_pass(const Box& q, const SOMat& M, const Box& b) {
    Box w;
    sov_row(M.r0, b, w.lx, w.hx); sov_row(M.r1, b, w.ly, w.hy); sov_row(M.r2, b, w.lz, w.hz);
    return box_valid(b) && box_overlap(q, w);
}

// instance k's forward matrix and BLAS; false: inactive instance (the active flag is k_instance_boxes's, the matrix the caller's record)
__device__ __forceinline__ bool sov_enter_instance(const SceneQuery& a, u32 k, SOMat& M, SceneBlas& B) {
    const u32 bl = __float_as_uint(reinterpret_cast<const float4*>(a.inst + k)[3].x);
    if (bl == INV) return false;
    M = inst_load_m(a, k);
    B = a.blas[bl];
    return true;
}

// V.r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3: the header's world vertex (xf_point's order on the rows held in registers)
__device__ __forceinline__ QF3 st_world(const SOMat& M, QF3 v) {
    return { ((M.r0.x * v.x + M.r0.y * v.y) + M.r0.z * v.z) + M.r0.w, ((M.r1.x * v.x + M.r1.y * v.y) + M.r1.z * v.z) + M.r1.w,
             ((M.r2.x * v.x + M.r2.y * v.y) + M.r2.z * v.z) + M.r2.w };
}

// the world triangle of primitive prim (< B.n) of the instance whose matrix is M
__device__ __forceinline__ void st_world_tri(const SceneBlas& B, const SOMat& M, u32 prim, QF3& y1, QF3& y2, QF3& y3) {
    QF3 v1, v2, v3;
    blas_tri_fetch(B, prim, v1, v2, v3);
    y1 = st_world(M, v1); y2 = st_world(M, v2); y3 = st_world(M, v3);
}

} // namespace bvh
