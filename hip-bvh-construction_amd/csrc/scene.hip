// scene.hip — bvh_scene on gfx950: instanced scenes, two levels (no counterpart in the reference).  A top-level tree (TLAS) over the instances' world boxes,
// whose leaves are instances, and per instance a bottom-level tree (BLAS) traversed with the ray mapped into the instance's object space.  One ray per lane; the
// BLAS's layout and triangle format are read from its 64-byte descriptor when the ray enters the instance and dispatched at run time (uniform per instance).
// The hit test, box test and loads are query.hpp's, shared with k_intersect; the entry into an instance and the BLAS's triangle are scene_query.hpp's.  DESIGN.md §8d.
// Compiled WITHOUT the SLP vectoriser (Makefile): with it, the record update of an equal-t replacement (a tie decided by the prim index) kept the losing
// candidate's v while taking the winner's t / u / prim — the vectoriser packs the divisions of the hit test into <iu, it> / <iv, iw> pairs that reach the record
// through separate phi chains.  Found by tests/test_gpu_scene.py (one identity instance against bvh_intersect, Sponza-like mesh: 682 of 4096 rays).
#include "scene_query.hpp"

namespace bvh {

//   k_instance_boxes       : one thread per instance: world-to-object matrix (f64 adjugate / determinant, rounded once), active flag, world box, scale bound s2.
//   k_scene_intersect      : one per-lane LDS short stack shared by both levels (bit 31 of an entry marks a BLAS node); entering an instance keeps best t,
//                            popping a top-level entry restores the world ray.  Overflow marks the ray, as k_intersect does.
//   k_scene_intersect_deep : the marked rays, stackless: the top-level plan, and for every instance whose world box passes, that BLAS's plan.
constexpr int SCENE_INST_BLOCK = 256;

// object_to_world M (row-major 3x4, f32) -> world_to_object, in the order the header states; false: the instance is inactive
__device__ __forceinline__ bool instance_inverse(const float* m, float* w) {
    bool ok = true;
    for (int j = 0; j < 12; ++j) ok = ok && isfinite(m[j]);
    const double a00 = m[0], a01 = m[1], a02 = m[2], t0 = m[3], a10 = m[4], a11 = m[5], a12 = m[6], t1 = m[7], a20 = m[8], a21 = m[9], a22 = m[10], t2 = m[11];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    ok = ok && det != 0.0 && isfinite(det);
    const double i00 = c00 / det, i01 = (a02 * a21 - a01 * a22) / det, i02 = (a01 * a12 - a02 * a11) / det;
    const double i10 = c01 / det, i11 = (a00 * a22 - a02 * a20) / det, i12 = (a02 * a10 - a00 * a12) / det;
    const double i20 = c02 / det, i21 = (a01 * a20 - a00 * a21) / det, i22 = (a00 * a11 - a01 * a10) / det;
    const double u0 = -((i00 * t0 + i01 * t1) + i02 * t2), u1 = -((i10 * t0 + i11 * t1) + i12 * t2), u2 = -((i20 * t0 + i21 * t1) + i22 * t2);
    w[0] = (float)i00; w[1] = (float)i01; w[2] = (float)i02; w[3] = (float)u0;
    w[4] = (float)i10; w[5] = (float)i11; w[6] = (float)i12; w[7] = (float)u1;
    w[8] = (float)i20; w[9] = (float)i21; w[10] = (float)i22; w[11] = (float)u2;
    for (int j = 0; j < 12; ++j) ok = ok && isfinite(w[j]);
    return ok;
}
// the point queries' scale bound s2 = (1 - 2^-10) / lambda of the rounded W (f32 entries as f64), lambda = max absolute row sum of W W^T >= sigma_max(W)^2
__device__ __forceinline__ float instance_s2(const float* w) {
    double lambda = 0.0, row[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) row[j] = fabs(((double)w[4 * i] * (double)w[4 * j] + (double)w[4 * i + 1] * (double)w[4 * j + 1]) + (double)w[4 * i + 2] * (double)w[4 * j + 2]);
        lambda = fmax(lambda, (row[0] + row[1]) + row[2]);
    }
    return (float)((1.0 - 0x1p-10) / lambda);
}

__global__ __launch_bounds__(SCENE_INST_BLOCK) void k_instance_boxes(const bvh_instance* __restrict__ instances, u32 n_inst, const SceneBlas* __restrict__ blas,
                                                                     u32 n_blas, SceneInst* __restrict__ out, bvh_aabb* __restrict__ wbox) {
    const u32 k = bid_x() * SCENE_INST_BLOCK + tid_x();
    if (k >= n_inst) return;
    const float4* q = reinterpret_cast<const float4*>(instances + k);
    float m[12], w[12];
    mat_rows({ q[0], q[1], q[2] }, m);
    const u32 bl = __float_as_uint(q[3].x);
    const bool ok = instance_inverse(m, w) && bl < n_blas;
    Box wb = box_empty();
    if (ok) {
        const SceneBlas B = blas[bl];
        const Box rb = box_load(&(reinterpret_cast<const bvh2_node*>(B.nodes) + B.root)->aabb);
        for (int c = 0; c < 8; ++c) {
            const QF3 p = xf_point(m, (c & 1) ? rb.hx : rb.lx, (c & 2) ? rb.hy : rb.ly, (c & 4) ? rb.hz : rb.lz);
            if (c == 0) wb = { p.x, p.y, p.z, p.x, p.y, p.z };
            else wb = { fminf(wb.lx, p.x), fminf(wb.ly, p.y), fminf(wb.lz, p.z), fmaxf(wb.hx, p.x), fmaxf(wb.hy, p.y), fmaxf(wb.hz, p.z) };
        }
    }
    float4* o = reinterpret_cast<float4*>(out + k);
    o[0] = make_float4(w[0], w[1], w[2], w[3]); o[1] = make_float4(w[4], w[5], w[6], w[7]); o[2] = make_float4(w[8], w[9], w[10], w[11]);
    o[3] = make_float4(__uint_as_float(ok ? bl : INV), ok ? instance_s2(w) : 0.0f, 0.0f, 0.0f);
    box_store(wbox + k, wb);
}

// leaf_test with the BLAS's format chosen at run time and the scene's order (t, instance, prim); true when an any-hit query is done
template <int QUERY>
__device__ __forceinline__ bool scene_leaf_test(const SceneBlas& B, u32 prim, u32 inst, const QRay& r, float& bt, float& bu, float& bv, u32& bp, u32& bi) {
    if (prim >= B.n) return false;
    QF3 a, b, c;
    blas_tri_fetch(B, prim, a, b, c);
    float it = 0.0f, iu = 0.0f, iv = 0.0f;                     // (defined on every path: the record below is taken whole or not at all)
    const bool hit = tri_hit(a, b, c, r, it, iu, iv) && r.tmin < it && it < r.tmax;
    const bool take = hit && (QUERY == BVH_QUERY_ANY || it < bt || (it == bt && (inst < bi || (inst == bi && prim < bp))));
    if (take) { bt = it; bu = iu; bv = iv; bp = prim; bi = inst; }
    return take && QUERY == BVH_QUERY_ANY;
}

__device__ __forceinline__ void scene_hit_store(void* hits, u32 i, float t, float u, float v, u32 prim, u32 inst) {
    float4* h = reinterpret_cast<float4*>(hits) + 2 * (size_t)i;
    h[0] = make_float4(t, u, v, __uint_as_float(prim));
    h[1] = make_float4(__uint_as_float(inst), 0.0f, 0.0f, 0.0f);
}

template <int QUERY>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_intersect(SceneQuery a) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= a.n_rays) return;
    u32* const stack = s_stack + tid_x();
    QRay w;
    const bool live = ray_load(reinterpret_cast<const bvh_ray*>(a.rays), i, w);
    float bt = w.tmax, bu = 0.0f, bv = 0.0f;
    u32 bp = INV, bi = INV;
    bool deep = false;
    if (live) {
        QRay r = w;
        SceneBlas B{};
        const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
        u32 ni = tni, total = ttotal;                                 // of the level the ray is on
        bool in_blas = false, pop = false, entering = false;         // entering: instance `enter` is entered at the top of the next step
        u32 inst = INV, enter = INV;
        u32 nl = INV, nr = INV, top = 0, tsteps = 0, bsteps = 0;
        if (a.n_inst == 1) {                                          // no top-level tree: the instance's world box, then the instance
            float tn;
            if (box_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), w, bt, tn)) { enter = 0; entering = true; } else pop = true;
        } else {
            const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(a.tnodes) + a.troot); nl = lr.x; nr = lr.y;
        }
        for (;;) {
            if (entering) {
                entering = false;
                const u32 k = enter;
                if (k < a.n_inst && enter_instance_ray(a, k, w, r, B)) {
                    in_blas = true; inst = k; ni = B.n - 1; total = 2 * B.n - 1; bsteps = 0;
                    const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(B.nodes) + B.root); nl = lr.x; nr = lr.y;
                } else pop = true;
            }
            if (!pop) {
                if (in_blas ? ++bsteps > B.n : ++tsteps > ttotal) { deep = true; break; }   // (a tree never gets here)
                const int layout = in_blas ? (int)B.layout : (int)a.tlayout;
                const void* nodes = in_blas ? B.nodes : a.tnodes; const void* leaves = in_blas ? B.leaves : a.tleaves;
                u32 a0 = INV, a1 = INV, b0 = INV, b1 = INV;
                Box ba, bb;
                float ta = 0.0f, tb = 0.0f;
                bool ha = false, hb = false;
                if (nl < total) { rec_fetch_rt(layout, nodes, leaves, nl, ni, a0, a1, ba); ha = box_pass(ba, r, bt, ta); }
                if (nr < total) { rec_fetch_rt(layout, nodes, leaves, nr, ni, b0, b1, bb); hb = box_pass(bb, r, bt, tb); }
                if (in_blas) {                                        // triangles at once; at the top level a leaf is an instance, entered like a node
                    bool done = false;
                    if (ha && nl >= ni) { done = scene_leaf_test<QUERY>(B, a0, inst, r, bt, bu, bv, bp, bi); ha = false; }
                    if (hb && nr >= ni && !done) { done = scene_leaf_test<QUERY>(B, b0, inst, r, bt, bu, bv, bp, bi); hb = false; }
                    if (done) break;
                }
                u32 c = INV, c0 = INV, c1 = INV;
                if (ha && hb) {
                    const bool left_first = ta <= tb;
                    if (top == (u32)QUERY_STACK) { deep = true; break; }
                    stack[top * QUERY_BLOCK] = (left_first ? nr : nl) | (in_blas ? SCENE_BLAS_ENTRY : 0u); ++top;
                    c = left_first ? nl : nr; c0 = left_first ? a0 : b0; c1 = left_first ? a1 : b1;
                } else if (ha) { c = nl; c0 = a0; c1 = a1; }
                else if (hb) { c = nr; c0 = b0; c1 = b1; }
                if (c == INV) pop = true;
                else if (in_blas || c < tni) { nl = c0; nr = c1; }
                else { enter = c0; entering = true; }                 // a top-level leaf: its instance
            }
            if (pop) {
                pop = false;
                if (top == 0) break;
                const u32 e = stack[--top * QUERY_BLOCK];
                if (e & SCENE_BLAS_ENTRY) {
                    const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(B.nodes) + (e & ~SCENE_BLAS_ENTRY)); nl = lr.x; nr = lr.y;
                } else {
                    if (in_blas) { r = w; in_blas = false; ni = tni; total = ttotal; }   // back to the top level: the world ray
                    u32 w0, w1; Box b;
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, e, tni, w0, w1, b);
                    if (e < tni) { nl = w0; nr = w1; } else { enter = w0; entering = true; }
                }
            }
        }
    }
    if (deep) { scene_hit_store(a.hits, i, w.tmax, 0.0f, 0.0f, QUERY_MARK, INV); atomicAdd(a.overflow, 1u); }
    else scene_hit_store(a.hits, i, bt, bu, bv, bp, bi);
}

// stackless walk of instance k's BLAS (k_intersect_deep's walk through the BLAS's plan); true when an any-hit query is done
template <int QUERY>
__device__ bool scene_walk_blas(const SceneQuery& a, u32 k, const QRay& w, float& bt, float& bu, float& bv, u32& bp, u32& bi) {
    QRay r; SceneBlas B;
    if (k >= a.n_inst || !enter_instance_ray(a, k, w, r, B)) return false;
    const u32 ni = B.n - 1, total = 2 * B.n - 1;
    const u64 bound = 3ull * total + 3ull;
    u32 cur = B.root, last = INV;
    bool down = true;
    for (u64 steps = 0; cur < total && steps < bound; ++steps) {
        u32 w0, w1; Box b;
        if (down) {
            rec_fetch_rt((int)B.layout, B.nodes, B.leaves, cur, ni, w0, w1, b);
            if (cur >= ni) {
                if (scene_leaf_test<QUERY>(B, w0, k, r, bt, bu, bv, bp, bi)) return true;
                last = cur; cur = B.parent[cur]; down = false;
                continue;
            }
            float tn;
            if (!box_pass(b, r, bt, tn)) { last = cur; cur = B.parent[cur]; down = false; continue; }
            if (w0 < total) { cur = w0; continue; }
            last = w0; down = false;
            continue;
        }
        if (cur >= ni) break;
        const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(B.nodes) + cur);
        if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
        last = cur; cur = B.parent[cur];
    }
    return false;
}

template <int QUERY>
__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_intersect_deep(SceneQuery a) {
    if (*a.overflow == 0u) return;
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 bound = 3ull * ttotal + 3ull;
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < a.n_rays; i += nbid_x() * QUERY_BLOCK) {
        if (__float_as_uint(reinterpret_cast<const float4*>(a.hits)[2 * (size_t)i].w) != QUERY_MARK) continue;
        QRay w;
        ray_load(reinterpret_cast<const bvh_ray*>(a.rays), i, w);     // (a marked ray passed the checks)
        float bt = w.tmax, bu = 0.0f, bv = 0.0f;
        u32 bp = INV, bi = INV;
        if (a.n_inst == 1) {
            float tn;
            if (box_pass(box_load(reinterpret_cast<const bvh_aabb*>(a.wbox)), w, bt, tn)) scene_walk_blas<QUERY>(a, 0, w, bt, bu, bv, bp, bi);
        } else {
            u32 cur = a.troot, last = INV;
            bool down = true;
            for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
                u32 w0, w1; Box b;
                if (down) {
                    rec_fetch_rt((int)a.tlayout, a.tnodes, a.tleaves, cur, tni, w0, w1, b);
                    float tn;
                    if (!box_pass(b, w, bt, tn)) { last = cur; cur = a.tparent[cur]; down = false; continue; }
                    if (cur >= tni) {                                 // an instance whose world box passes
                        if (scene_walk_blas<QUERY>(a, w0, w, bt, bu, bv, bp, bi)) break;
                        last = cur; cur = a.tparent[cur]; down = false;
                        continue;
                    }
                    if (w0 < ttotal) { cur = w0; continue; }
                    last = w0; down = false;
                    continue;
                }
                if (cur >= tni) break;
                const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(a.tnodes) + cur);
                if (last == lr.x && lr.y < ttotal && lr.y != lr.x) { cur = lr.y; down = true; continue; }
                last = cur; cur = a.tparent[cur];
            }
        }
        scene_hit_store(a.hits, i, bt, bu, bv, bp, bi);
    }
}

void launch_instance_boxes(hipStream_t s, const void* d_instances, uint32_t n_inst, const SceneBlas* d_blas, uint32_t n_blas, SceneInst* d_inst, void* d_wbox) {
    KernelScope ks(s, "k_instance_boxes");
    hipLaunchKernelGGL(k_instance_boxes, dim3((n_inst + SCENE_INST_BLOCK - 1) / SCENE_INST_BLOCK), dim3(SCENE_INST_BLOCK), 0, s,
                       (const bvh_instance*)d_instances, n_inst, d_blas, n_blas, d_inst, (bvh_aabb*)d_wbox);
}

void launch_scene_intersect(hipStream_t s, int query, const SceneQuery& q) {
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    { KernelScope ks(s, "k_scene_intersect");
      if (query == BVH_QUERY_ANY) hipLaunchKernelGGL(k_scene_intersect<BVH_QUERY_ANY>, dim3(blocks), dim3(QUERY_BLOCK), 0, s, q);
      else hipLaunchKernelGGL(k_scene_intersect<BVH_QUERY_CLOSEST>, dim3(blocks), dim3(QUERY_BLOCK), 0, s, q); }
    { KernelScope ks(s, "k_scene_intersect_deep");
      if (query == BVH_QUERY_ANY) hipLaunchKernelGGL(k_scene_intersect_deep<BVH_QUERY_ANY>, dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q);
      else hipLaunchKernelGGL(k_scene_intersect_deep<BVH_QUERY_CLOSEST>, dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q); }
}

void warm_scene() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_intersect<BVH_QUERY_CLOSEST>)); }

} // namespace bvh
