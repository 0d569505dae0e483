// refit.hip — bvh_refit on gfx950: recompute every box of an existing BVH2 from new triangle positions, topology kept (no counterpart in the
// reference).  Stage E (stage_em.hip, unchanged) has already written the new primitive boxes; two kernels follow:
//   k_refit_plan  : one thread per internal node writes parent[left] and parent[right] (parent[root] = INVALID), over one index space for both layouts —
//                   internal nodes [0, n-1), leaf j at n-1+j (the LBVH layout's own numbering; a PLOC-layout child >= n-1 already means leaf child-(n-1)).
//                   api.hip keeps the plan of a context's own tree until a build rewrites the tree, so an animation loop pays for it once.
//   k_refit_climb : one thread per sorted position j: the leaf's primitive box into its leaf record, then the two-pass build's bottom-up walk
//                   (common.hpp refit_climb: second-arriver exchange on the self-cleaning flags words, internal box = union of the children's boxes).
// Compiled WITHOUT -fno-honor-nans / -mno-amdgpu-ieee (Makefile): nothing here may be folded on the assumption that no NaN exists.
#include "common.hpp"
#include "kernels.hpp"

namespace bvh {

constexpr int REFIT_BLOCK = 256;

__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_plan(const bvh2_node* __restrict__ nodes, u32* __restrict__ parent, u32 n, u32 root) {
    const u32 i = bid_x() * REFIT_BLOCK + tid_x();
    const u32 ni = n - 1, total = 2 * n - 1;
    if (i == 0u && root < total) parent[root] = INV;
    if (i >= ni) return;
    const uint2 lr = *reinterpret_cast<const uint2*>(nodes + i);
    if (lr.x < total) parent[lr.x] = i;        // (links out of range — never in a tree — are not followed: no write outside the array)
    if (lr.y < total) parent[lr.y] = i;
}

// LAYOUT 0: leaf j is nodes[n-1+j] = {prim, INVALID, box}; LAYOUT 1: leaf j is leaves[j] = {prim, box} (28-byte PrimRef)
template <int LAYOUT>
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_climb(const bvh_aabb* __restrict__ prim_boxes, bvh2_node* nodes, bvh_primref* leaves,
                                                             const u32* __restrict__ parent, u32* flags, u32 n) {
    const u32 j = bid_x() * REFIT_BLOCK + tid_x();
    if (j >= n) return;
    const u32 ni = n - 1, cur = ni + j;
    auto prim_box = [&](u32 prim) { return box_gather(prim_boxes + (prim < n ? prim : 0u)); };   // (an index out of range — never in a tree — reads box 0)
    if (LAYOUT == 0) {
        const uint2 lr = *reinterpret_cast<const uint2*>(nodes + cur);
        const Box box = prim_box(lr.x);
        node_store_agent(nodes + cur, lr.x, lr.y, box);                  // read by the sibling's walker in this launch: write-through
        refit_climb(cur, box, nodes, parent, flags, ni);
    } else {
        const u32 prim = leaves[j].prim_idx;
        const Box box = prim_box(prim);
        float* f = &leaves[j].aabb.min.x;                                 // (offset 4 of a 28-byte record: 4-byte stores; read by later launches only)
        f[0] = box.lx; f[1] = box.ly; f[2] = box.lz; f[3] = box.hx; f[4] = box.hy; f[5] = box.hz;
        // a leaf sibling's box is taken where stage E wrote it (previous launch: plain loads), not from the leaf record another workgroup is writing now
        refit_climb(cur, box, nodes, parent, flags, ni, [&](u32 s) { return s < ni ? node_box_agent(nodes + s) : prim_box(leaves[s - ni].prim_idx); });
    }
}

void launch_refit_plan(hipStream_t s, const void* d_nodes, uint32_t n, uint32_t root, uint32_t* d_parent) {
    const u32 blocks = (n - 1 + REFIT_BLOCK - 1) / REFIT_BLOCK;
    KernelScope ks(s, "k_refit_plan");
    hipLaunchKernelGGL(k_refit_plan, dim3(blocks), dim3(REFIT_BLOCK), 0, s, (const bvh2_node*)d_nodes, d_parent, n, root);
}

void launch_refit_climb(hipStream_t s, const void* d_prim_boxes, void* d_nodes, void* d_leaves, int layout, uint32_t n, const uint32_t* d_parent, uint32_t* d_flags) {
    const u32 blocks = (n + REFIT_BLOCK - 1) / REFIT_BLOCK;
    KernelScope ks(s, "k_refit_climb");
    if (layout == 0) hipLaunchKernelGGL(k_refit_climb<0>, dim3(blocks), dim3(REFIT_BLOCK), 0, s, (const bvh_aabb*)d_prim_boxes, (bvh2_node*)d_nodes, (bvh_primref*)d_leaves, d_parent, d_flags, n);
    else             hipLaunchKernelGGL(k_refit_climb<1>, dim3(blocks), dim3(REFIT_BLOCK), 0, s, (const bvh_aabb*)d_prim_boxes, (bvh2_node*)d_nodes, (bvh_primref*)d_leaves, d_parent, d_flags, n);
}

void warm_refit() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_refit_climb<0>)); }

} // namespace bvh
