// scene_map.hpp — what the set-valued scene queries that test MAPPED boxes share (scene_overlap.hip: bvh_scene_overlap; scene_tris.hip:
// bvh_scene_intersect_tris): the forward matrix of the entered instance, the header's mapped box and the record sink.
//   mapped(M, {lo, hi}), row r:  a_c = m_rc * lo.c, b_c = m_rc * hi.c,  min.r = ((fminf(a_0, b_0) + fminf(a_1, b_1)) + fminf(a_2, b_2)) + m_r3,  max.r with fmaxf
// in f32 without contraction (every file that includes this is built with -ffp-contract=off and without the SLP vectoriser, Makefile).
#pragma once
#include "query.hpp"
#include "kernels.hpp"

namespace bvh {

static_assert(sizeof(bvh_instance_prim) == sizeof(uint2), "a record leaves in one 8-byte store");

// the forward matrix of the instance the walk is in (rows of object_to_world)
struct SOMat { float4 r0, r1, r2; };

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
    const float4* mq = reinterpret_cast<const float4*>(reinterpret_cast<const bvh_instance*>(a.inst_in) + k);
    M.r0 = mq[0]; M.r1 = mq[1]; M.r2 = mq[2];
    B = a.blas[bl];
    return true;
}

} // namespace bvh
