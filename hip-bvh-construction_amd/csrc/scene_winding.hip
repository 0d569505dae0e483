// scene_winding.hip — bvh_scene_winding_prepare / bvh_scene_winding_number on gfx950: the generalized winding number of query points against an instanced scene
// (no counterpart in the reference).  The value is bvh_winding_number's sum stated on WORLD triangles — the BLAS's vertices mapped by the instance's forward
// matrix, as bvh_scene_closest_point states its candidates — because the solid angle of one triangle is not invariant under a general 3x4 map (only the total
// over a closed surface is): DESIGN.md §8w.  The hierarchy is two-level Barnes–Hut.  A BLAS keeps bvh_winding_prepare's object-space records, made once per
// BLAS; seen from instance k a node's area vector is mapped by the cofactor matrix C_k (cross(Au, Av) = C (u x v)), its centre by M_k and its radius by
// smax_k >= sigma_max(A_k).  An instance is one dipole {C A, smax^2 area, M p, r from its world box} made from its BLAS's root record, and the top-level tree
// carries the flat climb's sums over those.
//   k_scene_winding_climb  : BLAS form: one thread per (BLAS, sorted leaf) of ALL BLASes at once — the BLAS by binary search of the prefix table the host made
//                            from the descriptors, layout and format per BLAS at run time — then k_winding_climb's walk on that BLAS's plan and its slice of
//                            the exchange words.  Top-level form: one thread per top-level leaf, whose sums are its instance's {A_k, a_k, a_k c_k}.
//   k_scene_winding_finish : k_winding_finish's step, one thread per (BLAS, internal node) or per top-level internal node.
//   k_scene_winding_inst   : one thread per instance: {C, smax} in f64 from the f32 matrix, and the instance moment from the BLAS's finished root record.
//   k_scene_winding        : one query per lane, one per-lane LDS short stack shared by both levels (k_scene_closest_point's structure, SCENE_BLAS_ENTRY tags a
//                            BLAS node).  Left child first at both levels.  A query whose push would overflow, or whose walk exceeds the step bound of the
//                            level it is on, writes QUERY_MARK's bits into its answer and bumps the overflow word.
//   k_scene_winding_deep   : returns at once while the overflow word is 0; otherwise re-walks the marked queries stackless through the top-level plan and the
//                            BLAS plans, left child first, under a step bound (arrays that are not trees terminate).
// The 22 values of an entered instance (M, C, smax) stay in registers while the walk is inside it: 88 VGPRs against 73 when they are re-read per node from the
// two 64-byte records, no scratch either way, and the kernel's occupancy is set by the 16 KiB stack (3 waves per SIMD) in both — DESIGN.md §8w.
// Built without the SLP vectoriser and without -fno-honor-nans (Makefile), as winding.o: the opening test must be false on NaN.
#include "winding.hpp"
#include "scene_query.hpp"

namespace bvh {

// the BLAS whose leaves hold thread t: the b with first[b] <= t < first[b + 1] (every BLAS has at least 2 leaves, so the table is strictly increasing)
__device__ __forceinline__ u32 wind_find_blas(const u32* __restrict__ first, u32 n_blas, u32 t) {
    u32 lo = 0, hi = n_blas;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (first[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ u32 blas_leaf_prim(const SceneBlas& B, u32 c) {
    const u32 ni = B.n - 1;
    return B.layout == 0 ? leaf_prim<0>(reinterpret_cast<const bvh2_node*>(B.nodes), nullptr, c, ni)
                         : leaf_prim<1>(nullptr, reinterpret_cast<const bvh_primref*>(B.leaves), c, ni);
}
// wsum_leaf of leaf c of BLAS B
__device__ __forceinline__ WSum blas_leaf_sum(const SceneBlas& B, u32 c) {
    const u32 prim = blas_leaf_prim(B, c);
    const TriSrc src{ B.tris, reinterpret_cast<const float*>(B.tris), reinterpret_cast<const u32*>(B.idx), B.nv };
    if (B.fmt == BVH_TRI_PADDED64) return wsum_leaf<BVH_TRI_PADDED64>(src, prim, B.n);
    if (B.fmt == BVH_TRI_PACKED36) return wsum_leaf<BVH_TRI_PACKED36>(src, prim, B.n);
    return wsum_leaf<BVH_TRI_INDEXED>(src, prim, B.n);
}
// the instance a top-level leaf c holds
__device__ __forceinline__ u32 top_leaf_inst(const SceneQuery& a, u32 c) {
    const u32 tni = a.n_inst - 1;
    return a.tlayout == 0 ? reinterpret_cast<const bvh2_node*>(a.tnodes)[c].left : reinterpret_cast<const bvh_primref*>(a.tleaves)[c - tni].prim_idx;
}
// the sums of top-level leaf c: {A_k, a_k, a_k * c_k} of its instance's moment (all zero for an inactive instance; an index out of range contributes nothing)
__device__ __forceinline__ WSum top_leaf_sum(const SceneQuery& a, const bvh_winding_moment* __restrict__ imom, u32 c) {
    const u32 k = top_leaf_inst(a, c);
    if (k >= a.n_inst) return { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    const float4* m = reinterpret_cast<const float4*>(imom + k);
    const float4 m0 = m[0], m1 = m[1];
    return { m0.x, m0.y, m0.z, m0.w, m0.w * m1.x, m0.w * m1.y, m0.w * m1.z };
}

// k_winding_climb's walk from leaf `cur` with sums s: the second arriver at a node adds left + right and writes the raw sums; leaf(c) recomputes a leaf sibling
template <typename Leaf>
__device__ __forceinline__ void wind_climb(u32 cur, WSum s, const bvh2_node* __restrict__ nodes, const u32* __restrict__ parent, u32* flags,
                                           bvh_winding_moment* mom, u32 ni, u32 total, Leaf leaf) {
    u32 p = parent[cur];
    while (p < ni) {
        drain_stores();
        const u32 sib = __hip_atomic_exchange(flags + p, cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (sib == INV) break;
        st_agent(flags + p, INV);
        compiler_fence();
        WSum o = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
        if (sib < ni) o = wsum_load_agent(mom + sib);                                  // written in this launch by the sibling's second arriver
        else if (sib < total) o = leaf(sib);
        s = nodes[p].left == cur ? wsum_add(s, o) : wsum_add(o, s);                    // left + right, whoever arrives second
        wsum_store_agent(mom + p, s);
        cur = p; p = parent[p];
    }
}

template <bool TOP>
__global__ __launch_bounds__(WIND_BLOCK) void k_scene_winding_climb(SceneQuery a, SceneWind sw, u32* tflags) {
    const u32 t = bid_x() * WIND_BLOCK + tid_x();
    if (TOP) {
        if (t >= a.n_inst) return;
        const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
        wind_climb(tni + t, top_leaf_sum(a, sw.imom, tni + t), reinterpret_cast<const bvh2_node*>(a.tnodes), a.tparent, tflags, sw.tmom, tni, ttotal,
                   [&](u32 c) { return top_leaf_sum(a, sw.imom, c); });
    } else {
        if (t >= sw.total_leaves) return;
        const u32 b = wind_find_blas(sw.first, sw.n_blas, t), f = sw.first[b];
        const SceneBlas B = a.blas[b];
        const u32 ni = B.n - 1, cur = ni + (t - f);
        if (cur >= 2 * B.n - 1) return;                           // (never: first[b + 1] - first[b] == B.n)
        wind_climb(cur, blas_leaf_sum(B, cur), reinterpret_cast<const bvh2_node*>(B.nodes), B.parent, sw.flags + f, sw.bmom + (f - b), ni, 2 * B.n - 1,
                   [&](u32 c) { return blas_leaf_sum(B, c); });
    }
}

template <bool TOP>
__global__ __launch_bounds__(WIND_BLOCK) void k_scene_winding_finish(SceneQuery a, SceneWind sw) {
    const u32 t = bid_x() * WIND_BLOCK + tid_x();
    const bvh2_node* nodes; bvh_winding_moment* mom; u32 i;
    if (TOP) {
        if (t + 1 >= a.n_inst) return;
        nodes = reinterpret_cast<const bvh2_node*>(a.tnodes); mom = sw.tmom; i = t;
    } else {
        if (t >= sw.total_leaves) return;
        const u32 b = wind_find_blas(sw.first, sw.n_blas, t), f = sw.first[b];
        i = t - f;
        if (i + 1 >= sw.first[b + 1] - f) return;                 // (one thread per leaf was launched: the last of each BLAS has no internal node)
        nodes = reinterpret_cast<const bvh2_node*>(a.blas[b].nodes); mom = sw.bmom + (f - b);
    }
    const float4* q = reinterpret_cast<const float4*>(nodes + i);
    const float4 q0 = q[0], q1 = q[1];
    wind_finish(mom + i, Box{ q0.z, q0.w, q1.x, q1.y, q1.z, q1.w });
}

// one thread per instance: the map {C, smax} and the instance moment (all zero for an inactive instance)
__global__ __launch_bounds__(WIND_BLOCK) void k_scene_winding_inst(SceneQuery a, SceneWind sw) {
    const u32 k = bid_x() * WIND_BLOCK + tid_x();
    if (k >= a.n_inst) return;
    float4* mo = reinterpret_cast<float4*>(sw.maps + k);
    float4* io = reinterpret_cast<float4*>(sw.imom + k);
    const u32 bl = a.inst[k].blas;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (bl == INV) { mo[0] = zero; mo[1] = zero; mo[2] = zero; mo[3] = zero; io[0] = zero; io[1] = zero; return; }
    float m[12];
    mat_rows(inst_load_m(a, k), m);
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    const float c[9] = { (float)(a11 * a22 - a12 * a21), (float)(a12 * a20 - a10 * a22), (float)(a10 * a21 - a11 * a20),
                         (float)(a02 * a21 - a01 * a22), (float)(a00 * a22 - a02 * a20), (float)(a01 * a20 - a00 * a21),
                         (float)(a01 * a12 - a02 * a11), (float)(a02 * a10 - a00 * a12), (float)(a00 * a11 - a01 * a10) };
    double lambda = 0.0;
    for (int i = 0; i < 3; ++i) {
        double row[3];
        for (int j = 0; j < 3; ++j)
            row[j] = fabs(((double)m[4 * i] * (double)m[4 * j] + (double)m[4 * i + 1] * (double)m[4 * j + 1]) + (double)m[4 * i + 2] * (double)m[4 * j + 2]);
        lambda = fmax(lambda, (row[0] + row[1]) + row[2]);
    }
    const float smax = (float)sqrt(lambda);
    mo[0] = make_float4(c[0], c[1], c[2], c[3]); mo[1] = make_float4(c[4], c[5], c[6], c[7]); mo[2] = make_float4(c[8], smax, 0.0f, 0.0f); mo[3] = zero;
    // the BLAS's root record, finished by k_scene_winding_finish in an earlier launch
    const SceneBlas B = a.blas[bl];
    const float4* r = reinterpret_cast<const float4*>(sw.bmom + (sw.first[bl] - bl) + B.root);
    const float4 r0 = r[0], r1 = r[1];
    const QF3 p = xf_point(m, r1.x, r1.y, r1.z);
    const Box wb = box_load(reinterpret_cast<const bvh_aabb*>(a.wbox) + k);
    io[0] = make_float4((c[0] * r0.x + c[1] * r0.y) + c[2] * r0.z, (c[3] * r0.x + c[4] * r0.y) + c[5] * r0.z, (c[6] * r0.x + c[7] * r0.y) + c[8] * r0.z,
                        (smax * smax) * r0.w);
    io[1] = make_float4(p.x, p.y, p.z, wind_radius(wb, p.x, p.y, p.z));
}

// ---- the query ------------------------------------------------------------------------------------------------------------------------------------------------
// what a walk knows of the instance it is in: the BLAS, its moments, the instance index and the 22 values of its maps (M, C, smax), live while it is inside
struct WInst { SceneBlas B; const bvh_winding_moment* mom; u32 k; float m[12], c[9], smax; };

// instance k for a walk; false: out of range or inactive (it contributes nothing)
__device__ __forceinline__ bool wind_enter(const SceneQuery& a, const SceneWind& sw, u32 k, WInst& I) {
    if (k >= a.n_inst) return false;
    const u32 bl = a.inst[k].blas;
    if (bl == INV) return false;
    I.B = a.blas[bl];
    I.mom = sw.bmom + (sw.first[bl] - bl);
    I.k = k;
    mat_rows(inst_load_m(a, k), I.m);
    const float4* cq = reinterpret_cast<const float4*>(sw.maps + k);
    const float4 c0 = cq[0], c1 = cq[1];
    const float2 c2 = *reinterpret_cast<const float2*>(cq + 2);
    I.c[0] = c0.x; I.c[1] = c0.y; I.c[2] = c0.z; I.c[3] = c0.w; I.c[4] = c1.x; I.c[5] = c1.y; I.c[6] = c1.z; I.c[7] = c1.w; I.c[8] = c2.x; I.smax = c2.y;
    return true;
}
// the world triangle of BLAS leaf c seen from q
__device__ __forceinline__ float scene_wind_leaf(const WInst& I, u32 c, QF3 q) {
    const u32 prim = blas_leaf_prim(I.B, c);
    if (prim >= I.B.n) return 0.0f;                               // (never in a tree: skipped)
    QF3 v1, v2, v3; blas_tri_fetch(I.B, prim, v1, v2, v3);
    return wind_solid_angle(xf_point(I.m, v1.x, v1.y, v1.z), xf_point(I.m, v2.x, v2.y, v2.z), xf_point(I.m, v3.x, v3.y, v3.z), q);
}
// BLAS internal node c seen from the world: A_w = C A, p_w = M p, r_w = smax r
__device__ __forceinline__ bool scene_wind_far(const WInst& I, u32 c, QF3 q, float beta, float& term) {
    const float4* r = reinterpret_cast<const float4*>(I.mom + c);
    const float4 r0 = r[0], r1 = r[1];
    const float* C = I.c;
    const QF3 A = { (C[0] * r0.x + C[1] * r0.y) + C[2] * r0.z, (C[3] * r0.x + C[4] * r0.y) + C[5] * r0.z, (C[6] * r0.x + C[7] * r0.y) + C[8] * r0.z };
    return wind_dipole(A, xf_point(I.m, r1.x, r1.y, r1.z), I.smax * r1.w, q, beta, term);
}
// one child of an opened BLAS node: adds its term and returns false, or returns true when it has to be opened (links out of range are skipped)
__device__ __forceinline__ bool scene_wind_blas_child(const WInst& I, u32 c, QF3 q, float beta, double& acc) {
    const u32 ni = I.B.n - 1, total = 2 * I.B.n - 1;
    if (c >= total) return false;
    if (c >= ni) { acc += (double)scene_wind_leaf(I, c, q); return false; }
    float term;
    if (!scene_wind_far(I, c, q, beta, term)) return true;
    acc += (double)term;
    return false;
}
// one child of an opened top-level node: an internal node follows the flat rule on its record; a leaf is its instance's dipole, or has to be entered
__device__ __forceinline__ bool scene_wind_top_child(const SceneQuery& a, const SceneWind& sw, u32 c, QF3 q, float beta, double& acc) {
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    if (c >= ttotal) return false;
    float term;
    if (c < tni) { if (!wind_far(sw.tmom, c, q, beta, term)) return true; }
    else {
        const u32 k = top_leaf_inst(a, c);
        if (k >= a.n_inst || a.inst[k].blas == INV) return false;
        if (!wind_far(sw.imom, k, q, beta, term)) return true;
    }
    acc += (double)term;
    return false;
}

__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_winding(SceneQuery a, SceneWind sw, float beta) {
    __shared__ u32 s_stack[QUERY_STACK * QUERY_BLOCK];
    const u32 i = bid_x() * QUERY_BLOCK + tid_x();
    if (i >= a.n_rays) return;
    u32* const stack = s_stack + tid_x();
    u32* const out = reinterpret_cast<u32*>(a.hits);
    QF3 q;
    if (!wind_point_load(reinterpret_cast<const bvh_point_query*>(a.rays), i, q)) { out[i] = WIND_NAN; return; }
    double acc = 0.0;
    bool deep = false;
    const u32 tni = a.n_inst - 1;
    const bvh2_node* const tnodes = reinterpret_cast<const bvh2_node*>(a.tnodes);
    WInst I{};
    bool in_blas = false, pop = false, entering = false;             // entering: instance `enter` is entered at the top of the next step
    u32 enter = INV, nl = INV, nr = INV, top = 0, tsteps = 0, bsteps = 0;
    if (a.n_inst == 1) { enter = 0; entering = true; }               // no top-level tree: the instance is always entered
    else { const uint2 lr = *reinterpret_cast<const uint2*>(tnodes + a.troot); nl = lr.x; nr = lr.y; }
    for (;;) {
        if (entering) {
            entering = false;
            if (wind_enter(a, sw, enter, I)) {
                in_blas = true; bsteps = 0;
                const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(I.B.nodes) + I.B.root); nl = lr.x; nr = lr.y;
            } else pop = true;
        }
        if (!pop) {
            if (in_blas ? ++bsteps > I.B.n : ++tsteps > a.n_inst) { deep = true; break; }   // more expansions than internal nodes (a tree never gets here)
            bool oa, ob;
            if (in_blas) { oa = scene_wind_blas_child(I, nl, q, beta, acc); ob = scene_wind_blas_child(I, nr, q, beta, acc); }
            else { oa = scene_wind_top_child(a, sw, nl, q, beta, acc); ob = scene_wind_top_child(a, sw, nr, q, beta, acc); }
            u32 next = INV;
            if (oa && ob) {
                if (top == (u32)QUERY_STACK) { deep = true; break; }
                stack[top * QUERY_BLOCK] = nr | (in_blas ? SCENE_BLAS_ENTRY : 0u); ++top;
                next = nl;
            } else if (oa) next = nl;
            else if (ob) next = nr;
            if (next == INV) pop = true;
            else if (in_blas) { const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(I.B.nodes) + next); nl = lr.x; nr = lr.y; }
            else if (next < tni) { const uint2 lr = *reinterpret_cast<const uint2*>(tnodes + next); nl = lr.x; nr = lr.y; }
            else { enter = top_leaf_inst(a, next); entering = true; }   // a top-level leaf that is not approximated: its instance
        }
        if (pop) {
            pop = false;
            if (top == 0) break;
            const u32 e = stack[--top * QUERY_BLOCK];
            if (e & SCENE_BLAS_ENTRY) {
                const uint2 lr = *reinterpret_cast<const uint2*>(reinterpret_cast<const bvh2_node*>(I.B.nodes) + (e & ~SCENE_BLAS_ENTRY)); nl = lr.x; nr = lr.y;
            } else {
                in_blas = false;                                      // back to the top level
                if (e < tni) { const uint2 lr = *reinterpret_cast<const uint2*>(tnodes + e); nl = lr.x; nr = lr.y; }
                else { enter = top_leaf_inst(a, e); entering = true; }
            }
        }
    }
    if (deep) { out[i] = QUERY_MARK; atomicAdd(a.overflow, 1u); }
    else wind_store(reinterpret_cast<float*>(a.hits), i, acc);
}

// stackless walk of instance k's BLAS (k_winding_deep's walk through the BLAS's plan, the root always opened)
__device__ void scene_wind_walk_blas(const SceneQuery& a, const SceneWind& sw, u32 k, QF3 q, float beta, double& acc) {
    WInst I;
    if (!wind_enter(a, sw, k, I)) return;
    const bvh2_node* const nodes = reinterpret_cast<const bvh2_node*>(I.B.nodes);
    const u32 ni = I.B.n - 1, total = 2 * I.B.n - 1;
    const u64 bound = 3ull * total + 3ull;                        // a tree: every node entered once from above and left at most twice
    u32 cur = I.B.root, last = INV;
    bool down = true;
    for (u64 steps = 0; cur < total && steps < bound; ++steps) {
        if (down) {
            if (cur >= ni) {
                acc += (double)scene_wind_leaf(I, cur, q);
                last = cur; cur = I.B.parent[cur]; down = false;
                continue;
            }
            float term;
            if (cur != I.B.root && scene_wind_far(I, cur, q, beta, term)) { acc += (double)term; last = cur; cur = I.B.parent[cur]; down = false; continue; }
            const u32 l = nodes[cur].left;
            if (l < total) { cur = l; continue; }
            last = l; down = false;                               // (a left link out of range: as if its subtree were done)
            continue;
        }
        if (cur >= ni) break;                                     // (parent links are internal nodes or INVALID)
        const uint2 lr = *reinterpret_cast<const uint2*>(nodes + cur);
        if (last == lr.x && lr.y < total && lr.y != lr.x) { cur = lr.y; down = true; continue; }
        last = cur; cur = I.B.parent[cur];
    }
}

__global__ __launch_bounds__(QUERY_BLOCK) void k_scene_winding_deep(SceneQuery a, SceneWind sw, float beta) {
    if (*a.overflow == 0u) return;
    const u32 tni = a.n_inst - 1, ttotal = 2 * a.n_inst - 1;
    const u64 bound = 3ull * ttotal + 3ull;
    const bvh2_node* const tnodes = reinterpret_cast<const bvh2_node*>(a.tnodes);
    for (u32 i = bid_x() * QUERY_BLOCK + tid_x(); i < a.n_rays; i += nbid_x() * QUERY_BLOCK) {
        if (reinterpret_cast<const u32*>(a.hits)[i] != QUERY_MARK) continue;
        QF3 q;
        wind_point_load(reinterpret_cast<const bvh_point_query*>(a.rays), i, q);   // (a marked query has no NaN coordinate)
        double acc = 0.0;
        if (a.n_inst == 1) scene_wind_walk_blas(a, sw, 0, q, beta, acc);
        else {
            u32 cur = a.troot, last = INV;
            bool down = true;
            for (u64 steps = 0; cur < ttotal && steps < bound; ++steps) {
                if (down) {
                    float term;
                    if (cur >= tni) {                             // an instance: its dipole, or its BLAS
                        const u32 k = top_leaf_inst(a, cur);
                        if (k < a.n_inst && a.inst[k].blas != INV) {
                            if (wind_far(sw.imom, k, q, beta, term)) acc += (double)term;
                            else scene_wind_walk_blas(a, sw, k, q, beta, acc);
                        }
                        last = cur; cur = a.tparent[cur]; down = false;
                        continue;
                    }
                    if (cur != a.troot && wind_far(sw.tmom, cur, q, beta, term)) { acc += (double)term; last = cur; cur = a.tparent[cur]; down = false; continue; }
                    const u32 l = tnodes[cur].left;
                    if (l < ttotal) { cur = l; continue; }
                    last = l; down = false;
                    continue;
                }
                if (cur >= tni) break;
                const uint2 lr = *reinterpret_cast<const uint2*>(tnodes + cur);
                if (last == lr.x && lr.y < ttotal && lr.y != lr.x) { cur = lr.y; down = true; continue; }
                last = cur; cur = a.tparent[cur];
            }
        }
        wind_store(reinterpret_cast<float*>(a.hits), i, acc);
    }
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------------------------------------
void launch_scene_winding_blas(hipStream_t s, const SceneQuery& q, const SceneWind& w) {
    const u32 blocks = (w.total_leaves + WIND_BLOCK - 1) / WIND_BLOCK;
    { KernelScope ks(s, "k_scene_winding_climb");
      hipLaunchKernelGGL(k_scene_winding_climb<false>, dim3(blocks), dim3(WIND_BLOCK), 0, s, q, w, (u32*)nullptr); }
    { KernelScope ks(s, "k_scene_winding_finish");
      hipLaunchKernelGGL(k_scene_winding_finish<false>, dim3(blocks), dim3(WIND_BLOCK), 0, s, q, w); }
}

void launch_scene_winding_top(hipStream_t s, const SceneQuery& q, const SceneWind& w, uint32_t* d_tflags) {
    const u32 blocks = (q.n_inst + WIND_BLOCK - 1) / WIND_BLOCK;
    { KernelScope ks(s, "k_scene_winding_inst");
      hipLaunchKernelGGL(k_scene_winding_inst, dim3(blocks), dim3(WIND_BLOCK), 0, s, q, w); }
    if (q.n_inst < 2) return;                                     // (one instance: no top-level tree)
    { KernelScope ks(s, "k_scene_winding_climb");
      hipLaunchKernelGGL(k_scene_winding_climb<true>, dim3(blocks), dim3(WIND_BLOCK), 0, s, q, w, d_tflags); }
    { KernelScope ks(s, "k_scene_winding_finish");
      hipLaunchKernelGGL(k_scene_winding_finish<true>, dim3(blocks), dim3(WIND_BLOCK), 0, s, q, w); }
}

void launch_scene_winding(hipStream_t s, const SceneQuery& q, const SceneWind& w, float beta) {
    const u32 blocks = (q.n_rays + QUERY_BLOCK - 1) / QUERY_BLOCK, deep_blocks = blocks < QUERY_DEEP_BLOCKS ? blocks : QUERY_DEEP_BLOCKS;
    { KernelScope ks(s, "k_scene_winding");
      hipLaunchKernelGGL(k_scene_winding, dim3(blocks), dim3(QUERY_BLOCK), 0, s, q, w, beta); }
    { KernelScope ks(s, "k_scene_winding_deep");
      hipLaunchKernelGGL(k_scene_winding_deep, dim3(deep_blocks), dim3(QUERY_BLOCK), 0, s, q, w, beta); }
}

void warm_scene_winding() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_scene_winding)); }

} // namespace bvh
