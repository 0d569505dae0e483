// refit_subset.hip — bvh_refit_subset on gfx950: new boxes for the listed primitives' leaves and for the nodes on the paths from those leaves to the root, nothing
// else read-modified (no counterpart in the reference).  Work is bounded by n_dirty x depth, shared ancestors are visited once.  Scratch (api.hip, outside the
// arena): leaf_of_prim u32[cap], owner u32[cap] (per leaf), pending u32[cap] (per internal node); owner and pending are all-zero between calls.
//   k_refit_leafmap      : one thread per leaf j: leaf_of_prim[prim of leaf j] = j (the array is all-INVALID before: a primitive no leaf holds stays INVALID).
//                          Kept for the ctx's own tree under the rule of the parent plan.
//   k_refit_subset_boxes : one thread per list entry t: skip p >= n; claim the leaf (compare-and-swap owner[j] 0 -> t + 1: duplicates retire here); the winner
//                          writes stage E's box of triangle p (common.hpp stage_e_box*: stage E's own expression) to d_prim_aabbs[p] and to the leaf record.
//   k_refit_subset_mark  : owners climb parent[] adding 1 to pending[a]; a walker stops at the first ancestor that was already marked (somebody marked from there
//                          up).  Afterwards pending[a] in {1, 2} = number of dirty child subtrees of every node on a dirty path, 0 elsewhere.
//   k_refit_subset_climb : owners clear their owner word and climb: drain the stores, subtract 1 from pending[a]; previous value 2: the other side finishes the
//                          node; 1: box = union(own box, sibling's box as stored — read, never recomputed), write-through store, go on.  The walker that
//                          finishes the root writes the scene extent.  Every word is zero again when the launch ends.
// Separate launches: what an earlier one wrote is read with plain loads; internal boxes written in the climb itself travel as agent-scope stores / loads and
// are published by the agent-scope atomic on pending[] after the writer drained its stores (the discipline of common.hpp refit_climb).
// Arrays that are not a tree: every index is checked before it is used (no access outside the arrays), a mark walker stops where it meets a mark (its own
// included: a cycle ends it), a climb walker continues only past a 1 -> 0 transition, of which there are at most as many as marks.
// Compiled WITHOUT -fno-honor-nans / -mno-amdgpu-ieee (Makefile): stage E's clamp of NaN and infinity must not be folded away.
#include "common.hpp"
#include "kernels.hpp"
#include "bvh_mi355x.h"

namespace bvh {

constexpr int RS_BLOCK = 256;

// LAYOUT 0: leaf j is nodes[n-1+j] = {prim, INVALID, box}; LAYOUT 1: leaf j is leaves[j] = {prim, box} (28-byte PrimRef)
template <int LAYOUT>
__global__ __launch_bounds__(RS_BLOCK) void k_refit_leafmap(const bvh2_node* __restrict__ nodes, const bvh_primref* __restrict__ leaves, u32* __restrict__ leaf_of_prim, u32 n) {
    const u32 j = bid_x() * RS_BLOCK + tid_x();
    if (j >= n) return;
    const u32 prim = LAYOUT == 0 ? reinterpret_cast<const u32*>(nodes + (n - 1 + j))[0] : leaves[j].prim_idx;
    if (prim < n) leaf_of_prim[prim] = j;              // (an index out of range — never in a tree — is not followed)
}

struct SubsetTris { const void* tris; const void* verts; const u32* idx; u32 n_verts; };

template <int LAYOUT, int FMT>
__global__ __launch_bounds__(RS_BLOCK) void k_refit_subset_boxes(SubsetTris in, const u32* __restrict__ prims, u32 n_dirty, const u32* __restrict__ leaf_of_prim,
                                                                 u32* owner, bvh_aabb* prim_boxes, bvh2_node* nodes, bvh_primref* leaves, u32 n) {
    const u32 t = bid_x() * RS_BLOCK + tid_x();
    if (t >= n_dirty) return;
    const u32 p = prims[t];
    if (p >= n) return;
    const u32 j = leaf_of_prim[p];
    if (j < n) {
        u32 expect = 0u;
        if (!__hip_atomic_compare_exchange_strong(owner + j, &expect, t + 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }                                                  // (no leaf holds p: every duplicate writes the same box to d_prim_aabbs[p], nothing else)
    Box box;
    if (FMT == BVH_TRI_PADDED64)      box = stage_e_box_padded(static_cast<const float4*>(in.tris), p);
    else if (FMT == BVH_TRI_PACKED36) box = stage_e_box9(static_cast<const float*>(in.tris) + (size_t)p * 9);
    else                              box = stage_e_box_indexed(static_cast<const float*>(in.verts), in.idx, in.n_verts, p);
    box_store(prim_boxes + p, box);
    if (j >= n) return;
    if (LAYOUT == 0) {                                 // bytes 8..31 of the leaf's node record (the links stay)
        bvh2_node* leaf = nodes + (n - 1 + j);
        reinterpret_cast<float2*>(leaf)[1] = make_float2(box.lx, box.ly);
        reinterpret_cast<float4*>(leaf)[1] = make_float4(box.lz, box.hx, box.hy, box.hz);
    } else {
        float* f = &leaves[j].aabb.min.x;              // (offset 4 of a 28-byte record: 4-byte stores)
        f[0] = box.lx; f[1] = box.ly; f[2] = box.lz; f[3] = box.hx; f[4] = box.hy; f[5] = box.hz;
    }
}

// the leaf entry t of the list owns, or INVALID
__device__ __forceinline__ u32 owned_leaf(const u32* __restrict__ prims, u32 t, const u32* __restrict__ leaf_of_prim, const u32* owner, u32 n) {
    const u32 p = prims[t];
    if (p >= n) return INV;
    const u32 j = leaf_of_prim[p];
    if (j >= n || owner[j] != t + 1u) return INV;
    return j;
}

__global__ __launch_bounds__(RS_BLOCK) void k_refit_subset_mark(const u32* __restrict__ prims, u32 n_dirty, const u32* __restrict__ leaf_of_prim,
                                                                const u32* __restrict__ owner, const u32* __restrict__ parent, u32* pending, u32 n) {
    const u32 t = bid_x() * RS_BLOCK + tid_x();
    if (t >= n_dirty) return;
    const u32 j = owned_leaf(prims, t, leaf_of_prim, owner, n);
    if (j == INV) return;
    const u32 ni = n - 1;
    u32 a = parent[ni + j];
    while (a < ni) {
        if (__hip_atomic_fetch_add(pending + a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
        a = parent[a];
    }
}

template <int LAYOUT>
__global__ __launch_bounds__(RS_BLOCK) void k_refit_subset_climb(const u32* __restrict__ prims, u32 n_dirty, const u32* __restrict__ leaf_of_prim, u32* owner,
                                                                 const u32* __restrict__ parent, u32* pending, const bvh_aabb* __restrict__ prim_boxes,
                                                                 bvh2_node* nodes, const bvh_primref* __restrict__ leaves, float* __restrict__ scene, u32 n, u32 root) {
    const u32 t = bid_x() * RS_BLOCK + tid_x();
    if (t >= n_dirty) return;
    const u32 j = owned_leaf(prims, t, leaf_of_prim, owner, n);
    if (j == INV) return;
    owner[j] = 0u;                                     // (a duplicate's thread reads t + 1 or 0 here, neither is its own position)
    const u32 ni = n - 1, total = 2 * n - 1;
    Box box = box_gather(prim_boxes + prims[t]);       // the box pass's (previous launch: plain loads)
    u32 cur = ni + j, a = parent[cur];
    while (a < ni) {
        drain_stores();
        const u32 prev = __hip_atomic_fetch_sub(pending + a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev != 1u) {
            if (prev == 0u) __hip_atomic_fetch_add(pending + a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (never in a tree: an unmarked node; undo)
            return;
        }
        compiler_fence();
        const uint2 lr = *reinterpret_cast<const uint2*>(nodes + a);
        const u32 sib = lr.x == cur ? lr.y : lr.x;
        Box sb = box_empty();                          // (a link out of range — never in a tree — is not followed)
        if (LAYOUT == 0) { if (sib < total) sb = node_box_agent(nodes + sib); }
        else if (sib < ni) sb = node_box_agent(nodes + sib);
        else if (sib < total) sb = box_load_u(&leaves[sib - ni].aabb);          // a leaf record is written by the box pass or not at all: plain loads
        box = box_union(box, sb);
        node_box_store_agent(nodes + a, box);
        cur = a; a = parent[a];
    }
    if (cur == root) { scene[0] = box.lx; scene[1] = box.ly; scene[2] = box.lz; scene[3] = box.hx; scene[4] = box.hy; scene[5] = box.hz; }
}

void launch_refit_leafmap(hipStream_t s, const void* d_nodes, const void* d_leaves, int layout, uint32_t n, uint32_t* d_leaf_of_prim) {
    const u32 blocks = (n + RS_BLOCK - 1) / RS_BLOCK;
    KernelScope ks(s, "k_refit_leafmap");
    (void)hipMemsetAsync(d_leaf_of_prim, 0xFF, (size_t)n * sizeof(u32), s);
    if (layout == 0) hipLaunchKernelGGL(k_refit_leafmap<0>, dim3(blocks), dim3(RS_BLOCK), 0, s, (const bvh2_node*)d_nodes, (const bvh_primref*)d_leaves, d_leaf_of_prim, n);
    else             hipLaunchKernelGGL(k_refit_leafmap<1>, dim3(blocks), dim3(RS_BLOCK), 0, s, (const bvh2_node*)d_nodes, (const bvh_primref*)d_leaves, d_leaf_of_prim, n);
}

template <int LAYOUT>
static void launch_boxes_fmt(hipStream_t s, u32 blocks, int fmt, const SubsetTris& in, const u32* prims, u32 n_dirty, const u32* map, u32* owner, bvh_aabb* pb,
                             bvh2_node* nodes, bvh_primref* leaves, u32 n) {
    if (fmt == BVH_TRI_PADDED64)      hipLaunchKernelGGL((k_refit_subset_boxes<LAYOUT, BVH_TRI_PADDED64>), dim3(blocks), dim3(RS_BLOCK), 0, s, in, prims, n_dirty, map, owner, pb, nodes, leaves, n);
    else if (fmt == BVH_TRI_PACKED36) hipLaunchKernelGGL((k_refit_subset_boxes<LAYOUT, BVH_TRI_PACKED36>), dim3(blocks), dim3(RS_BLOCK), 0, s, in, prims, n_dirty, map, owner, pb, nodes, leaves, n);
    else                              hipLaunchKernelGGL((k_refit_subset_boxes<LAYOUT, BVH_TRI_INDEXED>), dim3(blocks), dim3(RS_BLOCK), 0, s, in, prims, n_dirty, map, owner, pb, nodes, leaves, n);
}

void launch_refit_subset_boxes(hipStream_t s, int tri_format, const void* d_tris, const void* d_vertices, const void* d_indices, uint32_t n_vertices,
                               const uint32_t* d_prims, uint32_t n_dirty, const uint32_t* d_leaf_of_prim, uint32_t* d_owner, void* d_prim_boxes, void* d_nodes,
                               void* d_leaves, int layout, uint32_t n) {
    const u32 blocks = (n_dirty + RS_BLOCK - 1) / RS_BLOCK;
    const SubsetTris in{ d_tris, d_vertices, (const u32*)d_indices, n_vertices };
    KernelScope ks(s, "k_refit_subset_boxes");
    if (layout == 0) launch_boxes_fmt<0>(s, blocks, tri_format, in, d_prims, n_dirty, d_leaf_of_prim, d_owner, (bvh_aabb*)d_prim_boxes, (bvh2_node*)d_nodes, (bvh_primref*)d_leaves, n);
    else             launch_boxes_fmt<1>(s, blocks, tri_format, in, d_prims, n_dirty, d_leaf_of_prim, d_owner, (bvh_aabb*)d_prim_boxes, (bvh2_node*)d_nodes, (bvh_primref*)d_leaves, n);
}

void launch_refit_subset_climb(hipStream_t s, const uint32_t* d_prims, uint32_t n_dirty, const uint32_t* d_leaf_of_prim, uint32_t* d_owner, uint32_t* d_pending,
                               const uint32_t* d_parent, const void* d_prim_boxes, void* d_nodes, const void* d_leaves, int layout, uint32_t n, uint32_t root,
                               void* d_scene) {
    const u32 blocks = (n_dirty + RS_BLOCK - 1) / RS_BLOCK;
    { KernelScope ks(s, "k_refit_subset_mark");
      hipLaunchKernelGGL(k_refit_subset_mark, dim3(blocks), dim3(RS_BLOCK), 0, s, d_prims, n_dirty, d_leaf_of_prim, (const u32*)d_owner, d_parent, d_pending, n); }
    KernelScope ks(s, "k_refit_subset_climb");
    if (layout == 0) hipLaunchKernelGGL(k_refit_subset_climb<0>, dim3(blocks), dim3(RS_BLOCK), 0, s, d_prims, n_dirty, d_leaf_of_prim, d_owner, d_parent, d_pending,
                                        (const bvh_aabb*)d_prim_boxes, (bvh2_node*)d_nodes, (const bvh_primref*)d_leaves, (float*)d_scene, n, root);
    else             hipLaunchKernelGGL(k_refit_subset_climb<1>, dim3(blocks), dim3(RS_BLOCK), 0, s, d_prims, n_dirty, d_leaf_of_prim, d_owner, d_parent, d_pending,
                                        (const bvh_aabb*)d_prim_boxes, (bvh2_node*)d_nodes, (const bvh_primref*)d_leaves, (float*)d_scene, n, root);
}

void warm_refit_subset() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_refit_subset_mark)); }

} // namespace bvh
