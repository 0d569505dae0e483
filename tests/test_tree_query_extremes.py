"""CPU: the inputs of tests/test_gpu_tree_query_extremes.py — the twelve meshes of tests/test_query_extremes.py (non-finite, huge, far-offset and denormal
vertices) against the five tree-level queries that came after that file: bvh_intersect_tris, bvh_closest_tris, bvh_radius_tris, bvh_winding_prepare /
bvh_winding_number and bvh_cull — and the checks that those inputs are worth running: the share of well-conditioned queries the GPU file compares bit for
bit, the coverage every family is there for (the replaced triangle as an answer, ties, all-inf distances, NaN answers of the winding number), and, on the
CPU oracle's trees, that no plane value of any node is a NaN for any cull volume (so bvh_cull is exact on all of them).  The brute forces and host
restatements are the existing ones, unchanged (test_intersect_tris, test_closest_tris, test_radius_tris, test_winding, test_cull); each is computed once per
mesh and shared with the GPU file.  Run with -s for the table of figures."""
import numpy as np
import pytest

from test_closest_tris import pair_matrix
from test_closest_tris import tris_brute_force as closest_brute_force
from test_cull import PADDING, Tree, box_planes, by_prim, group_walk, lane_walk, make_volumes, slices_of
from test_gpu_refit import no_negzero
from test_intersect_tris import as_triangles, shifted, stage_e_boxes, xyz
from test_intersect_tris import tris_brute_force as crossing_brute_force
from test_overlap import csr_of
from test_point_query import point_brute_force, tri_arrays
from test_query_extremes import FRAMES, MESH_NAMES, SPECIAL_MESHES, families, mesh, points_of, replaced
from test_radius_tris import radius_tris_brute_force
from test_winding import FOURPI32, _comps, _dot, leaf_terms, moments_host, tree_arrays, walk_host

F32, F64 = np.float32, np.float64
BULK, AIMED, SIDE = 256, 64, 64
N_VOLUMES, N_EXTREME = 80, 16                       # make_volumes' volumes per plane count, and the ones made for the mesh's extreme behind them
PLANE_COUNTS = (1, 6, 8)
RADII = ("inf", "band", "zero", "negzero", "r2_inf", "r2_zero", "negative", "nan")
SELF_RADII = ("zero", "band")
NAN_MESHES = ["nan_coordinate", "nan_vertex", "neg_nan_coordinate", "ff_filled_triangle"]
TRI_EXACT = [m for m in MESH_NAMES if m != "denormals"]       # denormals: every dist2 underflows; held to the unconditional guarantees only

_QUERIES, _TRI_REF, _SELF_REF, _WIND_REF, _VOLUMES, _PAIRS = {}, {}, {}, {}, {}, {}


def source(pkg, name):
    """the finite mesh the queries of ``name`` are generated from: the unmodified base mesh for the specials, the mesh itself for the frames"""
    return mesh(pkg, "base" if name in SPECIAL_MESHES else name)


def scene(tris):
    """(lo, extent, diagonal) in f64 — without the 1e-3 floor of the other files' generators, which is far above a denormal frame"""
    v = xyz(tris).reshape(-1, 3).astype(F64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    return lo, hi - lo, float(np.linalg.norm(hi - lo))


# ---- triangle queries -------------------------------------------------------------------------------------------------------------------------------------------

def bulk_tris(pkg, tris, seed):
    """BULK triangles of test_gpu_closest_tris.make_queries' kinds: 80 of the mesh's shifted copy, 64 small random ones inside and outside the box, 32 that share
    a vertex (first half) or an edge with a tree triangle, 16 exact copies, 64 copies moved along their normal"""
    rng = np.random.default_rng(seed)
    t = xyz(tris); n = len(t)
    lo, ext, diag = scene(tris)
    parts = [xyz(shifted(pkg, tris))[rng.integers(0, n, 80)]]
    c = lo - 0.5 * ext + rng.random((64, 1, 3)) * 2.0 * ext
    parts.append(c + rng.normal(0, 1, (64, 3, 3)) * ext * rng.choice([1e-3, 2e-2, 0.1], size=(64, 1, 1)))
    s = t[rng.integers(0, n, 32)].astype(F64)
    s[:, 2] = s[:, 0] + rng.normal(0, 0.05, (32, 3)) * ext
    s[:16, 1] = s[:16, 0] + rng.normal(0, 0.05, (16, 3)) * ext
    parts.append(np.stack([np.roll(x, r, axis=0) for x, r in zip(s, rng.integers(0, 3, 32))]))
    parts.append(t[rng.integers(0, n, 16)])
    k = t[rng.integers(0, n, 64)].astype(F64)
    nrm = np.cross(k[:, 1] - k[:, 0], k[:, 2] - k[:, 0]); ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), (0.0, 0.0, 1.0))
    parts.append(k + (nrm * diag * rng.choice([1e-4, 1e-3, 2e-2], size=(64, 1)) * rng.choice([-1.0, 1.0], size=(64, 1)))[:, None, :])
    q = np.concatenate([np.asarray(x, dtype=F64) for x in parts]).astype(F32)
    assert len(q) == BULK
    return no_negzero(as_triangles(pkg, q))


def aimed_tris(pkg, name, seed):
    """AIMED triangles at the replaced triangle T as the base mesh has it: the first half cut it (one vertex on one side of a point of T's interior, two on the
    other), the second half lie next to it (T shrunk towards its centroid by 0.9, 0.5 or 0.2 and moved along its normal by 1e-3 or 2e-2 of its size)"""
    rng = np.random.default_rng(seed)
    T = xyz(mesh(pkg, "base"))[replaced(pkg, name)].astype(F64)
    cen = T.mean(axis=0)
    nrm = np.cross(T[1] - T[0], T[2] - T[0]); nrm /= np.linalg.norm(nrm)
    size = float(np.mean([np.linalg.norm(T[i] - T[(i + 1) % 3]) for i in range(3)]))
    half = AIMED // 2
    w = rng.dirichlet((2.0, 2.0, 2.0), size=half)
    p = w @ T
    d = nrm[None] + rng.normal(0, 0.3, (half, 3))
    h = size * rng.uniform(0.2, 1.0, (half, 1))
    cut = np.stack([p + d * h, p - d * h + rng.normal(0, 0.2 * size, (half, 3)), p - d * h + rng.normal(0, 0.2 * size, (half, 3))], axis=1)
    f = rng.choice([0.9, 0.5, 0.2], size=(half, 1, 1)); off = size * rng.choice([1e-3, 2e-2], size=(half, 1, 1)) * rng.choice([-1.0, 1.0], size=(half, 1, 1))
    near = cen + f * (T[None] - cen) + off * nrm[None, None]
    return no_negzero(as_triangles(pkg, np.concatenate([cut, near]).astype(F32)))


SIDE_KINDS = {"vertex_inf": 12, "vertex_3e38": 12, "nan": 8, "denormal": 10, "zero_area": 12, "span_2p100": 10}


def side_tris(pkg, tris, seed):
    """SIDE query-side specials on the unmodified mesh, by family: tree triangles jittered by 2 % of the extent with one coordinate of one vertex +-inf, +-3e38
    or NaN; random triangles scaled by 1e-41 (denormal coordinates next to the origin); zero-area triangles (points on tree vertices, segments along tree
    edges with either end repeated); scene-spanning triangles scaled by 2^100"""
    rng = np.random.default_rng(seed)
    t = xyz(tris).astype(F64); n = len(t)
    lo, ext, _ = scene(tris)

    def near(k):
        return (t[rng.integers(0, n, k)] + rng.normal(0, 0.02, (k, 3, 3)) * ext).astype(F32)

    def poked(k, values):
        q = near(k); i = np.arange(k)
        q[i, i % 3, (i // 3) % 3] = values(i)
        return q
    out = {"vertex_inf": poked(12, lambda i: np.where(i % 2 == 0, np.inf, -np.inf).astype(F32)),
           "vertex_3e38": poked(12, lambda i: np.where(i % 2 == 0, 3e38, -3e38).astype(F32)),
           "nan": poked(8, lambda i: F32(np.nan)),
           "denormal": ((lo + rng.random((10, 1, 3)) * ext + rng.normal(0, 0.1, (10, 3, 3)) * ext).astype(F32) * F32(1e-41)).astype(F32)}
    z = t[rng.integers(0, n, 12)]
    z[:4, 1] = z[:4, 0]; z[:4, 2] = z[:4, 0]                          # points on tree vertices
    z[4:8, 2] = z[4:8, 1]                                              # segments along tree edges
    z[8:, 2] = z[8:, 0]                                                # the same with the first vertex repeated
    out["zero_area"] = z.astype(F32)
    out["span_2p100"] = ((lo - 0.25 * ext + rng.random((10, 3, 3)) * 1.5 * ext) * 2.0 ** 100).astype(F32)
    assert {k: len(v) for k, v in out.items()} == SIDE_KINDS and sum(SIDE_KINDS.values()) == SIDE
    return {k: no_negzero(as_triangles(pkg, v)) for k, v in out.items()}


def plane_tris(pkg, tris, seed):
    """huge_offset: every x of the mesh is 3e38 after rounding.  SIDE triangles on or 0 to 8 ulps off that plane, on either side: the first half copies of tree
    triangles moved off the plane as a whole, the second half small random triangles over the mesh's y-z extent whose vertices take different offsets"""
    rng = np.random.default_rng(seed)
    t = xyz(tris); n = len(t)
    x = t[0, 0, 0]
    assert (t[:, :, 0] == x).all()
    ulp = F64(np.spacing(x))
    lo, ext, _ = scene(tris)
    half = SIDE // 2
    i = np.arange(half); j = i % 9; side = np.where((i // 9) % 2 == 0, 1.0, -1.0)
    a = t[rng.integers(0, n, half)].astype(F64)
    a[:, :, 0] = (F64(x) + side * j * ulp)[:, None]
    c = lo + rng.random((half, 1, 3)) * ext
    b = c + rng.normal(0, 0.05, (half, 3, 3)) * ext
    b[:, :, 0] = F64(x) + rng.choice([-1.0, 1.0], size=(half, 3)) * rng.integers(0, 9, size=(half, 3)) * ulp
    q = np.concatenate([a, b]).astype(F32)
    assert (q[:, :, 0].astype(F64) == np.concatenate([a, b])[:, :, 0]).all()      # the offsets are representable
    return as_triangles(pkg, q)


def tri_queries_of(pkg, name):
    """(query triangles, {family: slice}) of a mesh"""
    if name not in _QUERIES:
        seed = 5000 + MESH_NAMES.index(name)
        if name == "base":
            parts = side_tris(pkg, mesh(pkg, name), seed)
        elif name in SPECIAL_MESHES:
            parts = {"bulk": bulk_tris(pkg, mesh(pkg, "base"), seed), "aimed": aimed_tris(pkg, name, seed)}
        elif name == "huge_offset":
            parts = {"plane": plane_tris(pkg, mesh(pkg, name), seed)}
        else:
            parts = {"frame": bulk_tris(pkg, mesh(pkg, name), seed)}
        _QUERIES[name] = families(parts)
    return _QUERIES[name]


def radii_of(pkg, name):
    """the call radii by label: +inf, a band of 2e-3 of the scene diagonal, 0, -0, 1e30 (r2 = +inf), 1e-41 (r2 = 0), a negative one and a NaN"""
    d = scene(source(pkg, name))[2]
    return {"inf": np.inf, "band": float(F32(2e-3 * d)), "zero": 0.0, "negzero": -0.0, "r2_inf": 1e30, "r2_zero": 1e-41, "negative": -1.0, "nan": np.nan}


def tri_reference(pkg, name):
    """(queries, families, {radius label: (radius, closest brute force, radius brute force)}, (crossing sets, their (offsets, prims)), tie: the smallest dist2 of
    the query is attained by more than one primitive), computed once"""
    if name not in _TRI_REF:
        q, fam = tri_queries_of(pkg, name)
        tris = mesh(pkg, name)
        with np.errstate(all="ignore"):
            pairs = pair_matrix(q, tris)
            per = {label: (r, closest_brute_force(pkg, q, tris, r, pairs), radius_tris_brute_force(pkg, q, tris, r, pairs)) for label, r in radii_of(pkg, name).items()}
            sets = crossing_brute_force(q, tris)
            d2 = pairs[0]
            tie = (d2 == np.where(np.isnan(d2), np.inf, d2).min(axis=1, keepdims=True)).sum(axis=1) > 1      # the smallest dist2 is attained by two primitives
        _TRI_REF[name] = (q, fam, per, (sets, csr_of(sets)), tie)
        _PAIRS[(name, False)] = pairs
    return _TRI_REF[name]


def pairs_of(pkg, name, self_pairs=False):
    """test_closest_tris.pair_matrix of the mesh's queries (self_pairs: of the mesh itself) against the mesh, as the references above computed it"""
    self_reference(pkg, name) if self_pairs else tri_reference(pkg, name)
    return _PAIRS[(name, self_pairs)]


def self_reference(pkg, name):
    """a frame against itself, j > i: ((crossing sets, their (offsets, prims)), {radius label: (radius, radius brute force with SKIP_SHARED)})"""
    if name not in _SELF_REF:
        tris = mesh(pkg, name)
        r = radii_of(pkg, name)
        with np.errstate(all="ignore"):
            pairs = pair_matrix(tris, tris)
            rad = {label: (r[label], radius_tris_brute_force(pkg, tris, tris, r[label], pairs, self_pairs=True, skip_shared=True)) for label in SELF_RADII}
            sets = crossing_brute_force(tris, tris, self_pairs=True)
        _SELF_REF[name] = ((sets, csr_of(sets)), rad)
        _PAIRS[(name, True)] = pairs
    return _SELF_REF[name]


def in_slices(bf, prim):
    """how many slices of a radius brute force hold ``prim``"""
    return int((bf["hits"]["prim"] == prim).sum())


# ---- winding numbers ----------------------------------------------------------------------------------------------------------------------------------------------

def wind_points(pkg, name):
    """points_of(name) as the winding number reads them (the radius is ignored)"""
    return points_of(pkg, name)[0]


def terms32_sum64(pts, v1, v2, v3, chunk_elems=1 << 21):
    """the header's plain sum: the f32 leaf terms of test_winding.leaf_terms accumulated in f64"""
    pts = np.asarray(pts, dtype=F32)
    out = np.zeros(len(pts), dtype=F64)
    step = max(1, chunk_elems // max(len(v1), 1))
    with np.errstate(all="ignore"):
        for s in range(0, len(pts), step):
            out[s:s + step] = leaf_terms(pts[s:s + step, None, :], v1[None], v2[None], v3[None], F32).astype(F64).sum(axis=1)
    return out


def walk_host_sum64(nodes, leaves, layout, root, tris, moments, pts, beta):
    """test_winding.walk_host with dtype f32 — the same decisions and the same f32 terms, level by level — but the terms accumulated in f64 as the header says
    (walk_host(..., np.float32) also SUMS in f32, which can overflow or cancel where the f64 sum does not).  A point with a NaN coordinate answers NaN."""
    n, ni, prims = tree_arrays(nodes, leaves, layout)
    total = 2 * n - 1
    v1, v2, v3 = tri_arrays(tris)
    pts = np.ascontiguousarray(pts, dtype=F32)
    live = ~np.isnan(pts).any(axis=1)
    beta = F32(beta)
    if np.isinf(beta):
        use = np.sort(prims[prims < len(tris)])
        acc = terms32_sum64(pts, v1[use], v2[use], v3[use])
    else:
        acc = np.zeros(len(pts), dtype=F64)
        left, right = nodes["left"][:ni].astype(np.int64), nodes["right"][:ni].astype(np.int64)
        A, P, R = moments["a"].astype(F32), moments["p"].astype(F32), moments["r"].astype(F32)
        pi = np.nonzero(live)[0]; nd = np.full(len(pi), int(root), dtype=np.int64)
        with np.errstate(all="ignore"):
            while len(pi):
                nxt_p, nxt_n = [], []
                for side in (left, right):
                    ch = side[nd]
                    lf = (ch >= ni) & (ch < total)
                    pr = prims[ch[lf] - ni]
                    inr = pr < len(tris)
                    if inr.any():
                        sel = pi[lf][inr]; pr = pr[inr]
                        np.add.at(acc, sel, leaf_terms(pts[sel], v1[pr], v2[pr], v3[pr], F32).astype(F64))
                    it = ch < ni
                    c, qi = ch[it], pi[it]
                    d = P[c] - pts[qi]
                    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                    t = beta * R[c]
                    far = d2 > t * t
                    if far.any():
                        cf, qf = c[far], qi[far]
                        dd = _comps(P[cf] - pts[qf], F32)
                        dd2 = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]
                        term = _dot(_comps(A[cf], F32), dd) / ((FOURPI32 * dd2) * np.sqrt(dd2))
                        np.add.at(acc, qf, term.astype(F32).astype(F64))
                    nxt_p.append(qi[~far]); nxt_n.append(c[~far])
                pi, nd = np.concatenate(nxt_p), np.concatenate(nxt_n)
    acc[~live] = np.nan
    return acc


def wind_reference(pkg, name):
    """(points xyz f32, live, well: farther than 1e-4 of the scene diagonal from the surface, plain sum with f32 terms accumulated in f64, f64 brute force)"""
    if name not in _WIND_REF:
        tris = mesh(pkg, name)
        pts = wind_points(pkg, name)
        xyz_ = np.ascontiguousarray(pts["point"], dtype=F32)
        far = pts.copy(); far["radius"] = np.inf
        v1, v2, v3 = tri_arrays(tris)
        with np.errstate(all="ignore"):
            dist = np.sqrt(point_brute_force(pkg, far, tris)["closest"]["dist2"].astype(F64))
            well = dist > 1e-4 * scene(source(pkg, name))[2]
            plain = terms32_sum64(xyz_, v1, v2, v3)
            bf = leaf_terms(xyz_[:, None, :], v1[None], v2[None], v3[None], F64).sum(axis=1)
        live = ~np.isnan(xyz_).any(axis=1)
        plain[~live] = np.nan; bf[~live] = np.nan
        _WIND_REF[name] = (xyz_, live, well & live, plain, bf)
    return _WIND_REF[name]


# ---- cull volumes -------------------------------------------------------------------------------------------------------------------------------------------------

def finite_leaf_boxes(pkg, name):
    """the stage-E boxes the volumes are made around: the base mesh's for the specials, the mesh's own otherwise (all finite)"""
    b = stage_e_boxes(xyz(source(pkg, name)))
    assert np.isfinite(b["min"]).all() and np.isfinite(b["max"]).all()
    return b


def pow2_below(x):
    return 2.0 ** int(np.floor(np.log2(x)))


def extreme_volumes(pkg, name, per):
    """N_EXTREME volumes of ``per`` planes (a volume with fewer real planes is padded with (0, 0, 0, 1); per 1 keeps the first plane) made for the extremes:
    0-4 axis-aligned (the padded scene box, and half-spaces through the centre along +x, -x, +y, -z: every other coefficient a zero that meets the infinite
    and the huge box planes); 5-7 the same with -0 coefficients, 6 the all -0 padding plane; 8-10 the planes x >= 3e38, x <= -3e38 and x <= 3e38 (the boundary
    of huge_offset and of huge_triangle's box); 11-12 the scene box scaled up and down, 13 an oblique half-space scaled down (up: by 2^100 over the frame's
    own magnitude, so that the products stay finite on the finite boxes; down: by 2^-100); 14-15 oblique half-spaces through the centre with coefficients of
    both signs on two and three axes.  (The two volumes the issue asks for that keep a NaN under the zero-coefficient rule need a box with an infinite
    plane on both sides of one axis, lo = hi = +-inf: no mesh has one — test_no_box_lies_at_infinity — so they are left out.)"""
    lb = finite_leaf_boxes(pkg, name)
    lo = lb["min"].astype(F64).min(axis=0); hi = lb["max"].astype(F64).max(axis=0)
    ext = np.maximum(hi - lo, 1e-3 * np.maximum(np.abs(lo).max(), np.abs(hi).max())); ctr = 0.5 * (lo + hi)
    big = max(np.abs(lo - ext).max(), np.abs(hi + ext).max(), 1.0)
    up = 2.0 ** 100 / pow2_below(big) if big < 2.0 ** 90 else 1.0
    down = 2.0 ** -100
    box = box_planes(lo - ext, hi + ext)
    obl = np.array([1.0, 1.0, 1.0]); ob2 = np.array([1.0, -1.0, 0.0]); ob3 = np.array([-1.0, 1.0, -1.0])
    planes = [
        box, [(1.0, 0.0, 0.0, -ctr[0])], [(-1.0, 0.0, 0.0, ctr[0])], [(0.0, 1.0, 0.0, -ctr[1])], [(0.0, 0.0, -1.0, ctr[2])],
        [(1.0, -0.0, -0.0, -ctr[0])], [(-0.0, -0.0, -0.0, 1.0)], [(-0.0, 1.0, -0.0, -ctr[1])],
        [(1.0, 0.0, 0.0, -3e38)], [(-1.0, 0.0, 0.0, -3e38)], [(-1.0, 0.0, 0.0, 3e38)],
        [tuple(up * np.array(p)) for p in box], [tuple(down * np.array(p)) for p in box], [tuple(down * np.array((*obl, -float(obl @ ctr))))],
        [(*ob2, -float(ob2 @ ctr))], [(*ob3, -float(ob3 @ ctr))],
    ]
    assert len(planes) == N_EXTREME
    pad = [PADDING] * 8
    with np.errstate(over="ignore"):
        return np.array([(list(p) + pad)[:per] for p in planes], dtype=F64).astype(F32)


def volumes_of(pkg, name, per):
    """f32 (N_VOLUMES + N_EXTREME, per, 4): test_cull.make_volumes over the finite leaf boxes, then extreme_volumes"""
    if (name, per) not in _VOLUMES:
        lb = finite_leaf_boxes(pkg, name)
        with np.errstate(over="ignore", invalid="ignore"):
            v = make_volumes(pkg, lb, np.concatenate([lb["min"], lb["max"]]), 7000 + 10 * MESH_NAMES.index(name) + per, per, count=N_VOLUMES)
        _VOLUMES[(name, per)] = np.concatenate([v, extreme_volumes(pkg, name, per)])
    return _VOLUMES[(name, per)]


def nan_free(pkg, tree, volumes):
    """bool per volume: no plane value s — at the p-vertex or at the n-vertex — of any valid node of the tree is a NaN: bvh_cull's answer is then exact on that
    tree.  (From pkg.cull_plane_values, which test_cull.node_tests calls: node_tests itself returns the comparisons s >= 0, in which a NaN can no longer be told
    from a negative value.)"""
    out = np.zeros(len(volumes), dtype=bool)
    for i, vol in enumerate(volumes):
        s_p, s_n = pkg.cull_plane_values(vol[:, None, :], tree.lo[None], tree.hi[None])
        valid = (tree.lo <= tree.hi).all(axis=1)
        out[i] = not (np.isnan(s_p[:, valid]).any() or np.isnan(s_n[:, valid]).any())
    return out


def old_plane_values(planes, lo, hi):
    """pkg.cull_plane_values as it was before the zero-coefficient rule: every product taken, so 0 * inf is a NaN.  Only for the figures of
    test_the_zero_coefficient_rule_on_inf_vertex"""
    pl = np.asarray(planes, dtype=F32); lo = np.asarray(lo, dtype=F32); hi = np.asarray(hi, dtype=F32)
    with np.errstate(all="ignore"):
        sel = [pl[..., k] >= F32(0.0) for k in range(3)]

        def s_of(v):
            t = pl[..., 0] * v[0] + pl[..., 1] * v[1]
            t = t + pl[..., 2] * v[2]
            return (t + pl[..., 3]).astype(F32)
        return s_of([np.where(sel[k], hi[..., k], lo[..., k]) for k in range(3)]), s_of([np.where(sel[k], lo[..., k], hi[..., k]) for k in range(3)])


def share(mask, sl=slice(None)):
    return float(np.asarray(mask)[sl].mean())


# ---- triangle queries: shares, coverage ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MESH_NAMES)
def test_triangle_families_are_well_conditioned(pkg, name):
    q, fam, per, (sets, (coff, cprims)), tie = tri_reference(pkg, name)
    for f, sl in fam.items():
        for label in ("inf", "band", "zero"):
            _, cbf, rbf = per[label]
            print(f"tris   {name:20s} {f:12s} radius {label:5s} well: closest {share(cbf['well'], sl):.3f} radius {share(rbf['well'], sl):.3f}  hit {share(cbf['hit'], sl):.3f}  "
                  f"records {int(rbf['counts'][sl].sum())}  tie {share(tie, sl):.3f}  crossing pairs {int(coff[sl.stop] - coff[sl.start])}")
            if name in TRI_EXACT:
                assert share(cbf["well"], sl) >= 0.99 and share(rbf["well"], sl) >= 0.99, (name, f, label)
    if name == "denormals":                                          # every product of denormal edges underflows: dist2 == 0 for every pair, far below the boxes' distance
        assert per["inf"][1]["well"].mean() <= 0.8 and (per["zero"][2]["counts"] == len(mesh(pkg, name))).all()
    # radii that are the same r2 give the same answer; a negative or NaN radius answers nothing
    for a, b in (("zero", "negzero"), ("zero", "r2_zero"), ("inf", "r2_inf")):
        assert per[a][2]["hits"].tobytes() == per[b][2]["hits"].tobytes() and per[a][2]["offsets"].tobytes() == per[b][2]["offsets"].tobytes(), (a, b)
        assert per[a][1]["closest"]["prim"].tobytes() == per[b][1]["closest"]["prim"].tobytes()
    for label in ("negative", "nan"):
        assert not per[label][1]["hit"].any() and len(per[label][2]["hits"]) == 0
    # the two entry points agree: a sorted radius slice starts with the closest answer
    for label in RADII:
        _, cbf, rbf = per[label]
        has = rbf["counts"] > 0
        assert (has == cbf["hit"]).all() and rbf["hits"][rbf["offsets"][:-1][has]].tobytes() == cbf["closest"][has].tobytes(), (name, label)


@pytest.mark.parametrize("name", SPECIAL_MESHES)
def test_aimed_triangles_meet_the_replaced_triangle(pkg, name):
    """on the unmodified mesh the replaced triangle is an answer of an aimed triangle in each of the three queries; with a NaN coordinate it is in no answer of any
    query at any radius; with an infinite vertex it is still a candidate — the nearest triangle of some queries, a crossing one of some, in every slice of an
    infinite radius — and must be found through its infinite box; the huge triangle is in every slice of an infinite radius (at dist2 = +inf: its products
    overflow) and in no other answer"""
    rep = replaced(pkg, name)
    q, fam, per, (sets, (coff, cprims)), _ = tri_reference(pkg, name)
    aimed = q[fam["aimed"]]
    base = mesh(pkg, "base")
    with np.errstate(all="ignore"):
        pairs = pair_matrix(aimed, base)
        band = radii_of(pkg, name)["band"]
        n_closest = int((closest_brute_force(pkg, aimed, base, np.inf, pairs)["closest"]["prim"] == rep).sum())
        n_radius = in_slices(radius_tris_brute_force(pkg, aimed, base, band, pairs), rep)
        n_cross = sum(int(rep in s) for s in crossing_brute_force(aimed, base))
    print(f"{name}: on the base mesh the replaced triangle {rep} is the nearest of {n_closest} aimed triangles, within the band of {n_radius}, crossed by {n_cross}")
    assert n_closest >= 1 and n_radius >= 1 and n_cross >= 1
    got = {label: (int((per[label][1]["closest"]["prim"] == rep).sum()), in_slices(per[label][2], rep)) for label in RADII}
    crossed = int((cprims == rep).sum())
    print(f"{name}: on the special mesh (nearest of, in slices of) per radius {got}, crossed by {crossed}")
    if name in NAN_MESHES:
        assert all(v == (0, 0) for v in got.values()) and crossed == 0
    elif name == "huge_triangle":
        assert got["inf"] == (0, len(q)) and got["r2_inf"] == (0, len(q)) and all(got[label] == (0, 0) for label in RADII if label not in ("inf", "r2_inf")) and crossed == 0
        hits = per["inf"][2]["hits"]
        assert (hits["dist2"][hits["prim"] == rep] == np.inf).all()
    else:
        assert got["inf"][1] == len(q) and got["inf"][0] >= 1 and got["band"][1] >= 1 and crossed >= 1


def test_query_side_specials_keep_what_they_must(pkg):
    q, fam, per, (sets, (coff, cprims)), tie = tri_reference(pkg, "base")
    n = len(mesh(pkg, "base"))
    v = xyz(q)
    assert np.isinf(v[fam["vertex_inf"]]).any(axis=(1, 2)).all() and (np.abs(v[fam["vertex_3e38"]]) == F32(3e38)).any(axis=(1, 2)).all()
    assert np.isnan(v[fam["nan"]]).any(axis=(1, 2)).all() and (np.abs(v[fam["denormal"]]) < np.finfo(F32).tiny).all() and (np.abs(v[fam["span_2p100"]]) > 2.0 ** 90).any(axis=(1, 2)).all()
    counts = {f: {label: int(per[label][2]["counts"][sl].sum()) for label in ("inf", "band", "zero")} for f, sl in fam.items()}
    crossings = {f: int(coff[sl.stop] - coff[sl.start]) for f, sl in fam.items()}
    print("records per query-side special:", counts, " crossing pairs:", crossings)
    sl = fam["nan"]                                                   # a NaN query answers nothing, whatever the radius
    assert all(per[label][2]["counts"][sl].sum() == 0 and not per[label][1]["hit"][sl].any() for label in RADII) and crossings["nan"] == 0
    for f in ("vertex_inf", "vertex_3e38", "denormal", "zero_area", "span_2p100"):      # an infinite r2 accepts every candidate whose dist2 is not a NaN
        assert counts[f]["inf"] >= 1, f
    assert counts["denormal"]["inf"] == SIDE_KINDS["denormal"] * n and counts["zero_area"]["inf"] == SIDE_KINDS["zero_area"] * n
    assert counts["zero_area"]["zero"] >= 8 and crossings["zero_area"] == 0          # points on vertices and segments along edges are at dist2 == 0; no area, no crossing
    assert crossings["vertex_3e38"] >= 1                                            # huge but finite triangles still cut the mesh: found through huge boxes


def test_the_far_frames_tie(pkg):
    """at 2^20 the ulp is 1/8 on a unit mesh and on the plane x = 3e38 every off-plane distance overflows: the smallest dist2 is shared by several primitives, which the
    near-origin meshes of the other files never see; the (dist2, prim) rule decides"""
    for name, floor in (("offset_2p20", 0.25), ("huge_offset", 0.25)):
        q, fam, per, _, tie = tri_reference(pkg, name)
        rbf = per["inf"][2]
        rows = np.repeat(np.arange(len(q)), rbf["counts"])
        d = rbf["hits"]["dist2"]
        equal_neighbours = (d[1:] == d[:-1]) & (rows[1:] == rows[:-1])
        print(f"{name}: the closest answer ties on {tie.mean():.3f} of the queries; {equal_neighbours.mean():.3f} of the sorted records of an infinite radius equal their predecessor's dist2; "
              f"{int(np.isinf(d).sum())} of {len(d)} records at dist2 = +inf")
        assert tie.mean() >= floor and equal_neighbours.any(), name
    assert np.isinf(tri_reference(pkg, "huge_offset")[2]["inf"][2]["hits"]["dist2"]).any()


@pytest.mark.parametrize("name", FRAMES)
def test_self_modes_on_the_frames(pkg, name):
    (sets, (off, prims)), rad = self_reference(pkg, name)
    n = len(mesh(pkg, name))
    print(f"self   {name:20s} crossing pairs {int(off[-1])}  " + "  ".join(f"radius {label}: {len(bf['hits'])} records, well {bf['well'].mean():.3f}" for label, (_, bf) in rad.items()))
    assert off[-1] >= 1 and (prims > np.repeat(np.arange(n), np.diff(off.astype(np.int64)))).all()
    for label, (_, bf) in rad.items():
        assert len(bf["hits"]) >= 1
        if name != "denormals":
            assert bf["well"].mean() >= 0.99 and bf["ill_pairs"] == 0, (name, label)


# ---- winding numbers ----------------------------------------------------------------------------------------------------------------------------------------------

def test_sum64_twin_is_walk_host_with_an_f64_accumulator(pkg, orc):
    """walk_host_sum64 opens the nodes walk_host opens and adds the f32 terms walk_host(f32) adds: on the base mesh, where every term is tame, it lies within the
    f32 accumulator's own rounding of walk_host(f32) and nearer to walk_host(f64) than that is; beta = +inf is the plain sum"""
    tris = mesh(pkg, "base")
    xyz_, live, well, plain, bf = wind_reference(pkg, "offset_2p20")
    pts = (xyz_[live] - F32(2.0 ** 20)).astype(F32)                 # the frame's points moved back onto the base-sized mesh at the origin
    t = orc.build_tree(3, tris)
    mom = moments_host(pkg, t["nodes"], t["leaves"], t["layout"], t["root"], tris)
    for beta in (2.0, np.inf):
        w32 = walk_host(t["nodes"], t["leaves"], t["layout"], t["root"], tris, mom, pts, beta, np.float32).astype(F64)
        w64 = walk_host(t["nodes"], t["leaves"], t["layout"], t["root"], tris, mom, pts, beta, np.float64)
        mine = walk_host_sum64(t["nodes"], t["leaves"], t["layout"], t["root"], tris, mom, pts, beta)
        assert np.isfinite(mine).all() and np.abs(mine - w32).max() <= 4000 * 2.0 ** -24 * np.abs(w32).max() + 1e-6
        print(f"beta {beta}: |sum64 - f64| max {np.abs(mine - w64).max():.3e}, |f32 - f64| max {np.abs(w32 - w64).max():.3e}")
    v1, v2, v3 = tri_arrays(tris)
    assert walk_host_sum64(t["nodes"], t["leaves"], t["layout"], t["root"], tris, mom, pts, np.inf).tobytes() == terms32_sum64(pts, v1, v2, v3).tobytes()


@pytest.mark.parametrize("name", MESH_NAMES)
def test_winding_nan_counts(pkg, name):
    """where the header's formula itself answers NaN: the plain sum of the f32 terms (accumulated in f64) against the f64 brute force"""
    xyz_, live, well, plain, bf = wind_reference(pkg, name)
    n32, n64 = int(np.isnan(plain[live]).sum()), int(np.isnan(bf[live]).sum())
    both = live & np.isfinite(plain) & np.isfinite(bf) & well
    gap = float(np.abs(plain - bf)[both].max()) if both.any() else float("nan")
    print(f"wind   {name:20s} points {len(xyz_)} live {int(live.sum())} well {int(well.sum())}  NaN: f32 terms {n32}, f64 {n64}  |f32 terms - f64| max on the finite well points {gap:.3e}")
    if name in NAN_MESHES:
        assert n32 == n64 == int(live.sum())                          # the term of a triangle with a NaN coordinate is a NaN for every point
    elif name in ("huge_triangle", "scale_2p60"):
        assert n32 == int(live.sum()) and n64 == 0                     # the f32 products overflow to inf - inf; the f64 sum is finite
    elif name in ("offset_2p20", "scale_2p40", "denormals"):
        assert n32 == 0 and n64 == 0
    elif name in ("inf_vertex", "neg_inf_vertex", "huge_offset"):
        assert 1 <= n32 <= int(live.sum())
    assert np.isnan(plain[~live]).all() and np.isnan(bf[~live]).all()                 # a point with a NaN coordinate answers NaN


# ---- cull ---------------------------------------------------------------------------------------------------------------------------------------------------------

def test_no_box_lies_at_infinity(pkg):
    """after the zero-coefficient rule a NaN plane value needs inf - inf between two nonzero terms of one vertex: a box with lo = +inf or hi = -inf on an axis (the
    p-vertex of coefficients of opposite sign on two such axes).  Stage E keeps lo <= FLT_MAX and hi >= -FLT_MAX, and none of the twelve meshes has a box that is
    infinite on both sides of an axis either: the two made-for-NaN volumes of the issue have nothing to meet and are left out of extreme_volumes"""
    for name in MESH_NAMES:
        b = stage_e_boxes(xyz(mesh(pkg, name)))
        assert (b["min"] < np.inf).all() and (b["max"] > -np.inf).all(), name
        assert not (np.isinf(b["min"]) & np.isinf(b["max"])).any(), name


def overflowing(volumes, leaf):
    """bool per volume: a product of a nonzero plane coefficient with a finite box coordinate overflows, or an offset d is infinite — the inf - inf the contract
    leaves as a NaN"""
    lo, hi = leaf["min"].astype(F64), leaf["max"].astype(F64)
    big = np.maximum(np.abs(lo[np.isfinite(lo)]).max(), np.abs(hi[np.isfinite(hi)]).max())
    fmax = F64(np.finfo(F32).max)
    v = volumes.astype(F64)
    return ((np.abs(v[:, :, :3]) * big > fmax).any(axis=(1, 2))) | np.isinf(v[:, :, 3]).any(axis=1)


@pytest.mark.parametrize("name", MESH_NAMES)
def test_cull_volumes_are_exact_on_the_oracle_trees(pkg, orc, name):
    """no plane value of any node of any builder's tree is a NaN, for every volume without a NaN of its own — so bvh_cull's answer is exact —, and both host
    walks equal the brute force on the leaf boxes.  The one exception is stated, not hidden: make_volumes' camera frusta around huge_offset, a mesh at x = 3e38,
    have products a * x that overflow against an offset d = -inf; there the NaN is inf - inf between nonzero terms (overflowing()), which the contract keeps, and
    the host walks still equal the brute force."""
    tris = mesh(pkg, name); n = len(tris)
    trees = []
    for algo in (0, 1, 2, 3):
        t = orc.build_tree(algo, tris)
        trees.append(Tree(t["nodes"], t["leaves"], t["root"], n, t["layout"]))
    leaf = trees[0].leaf_boxes
    assert leaf.tobytes() == stage_e_boxes(xyz(tris)).tobytes()
    for per in PLANE_COUNTS:
        vols = volumes_of(pkg, name, per)
        assert vols.shape == (N_VOLUMES + N_EXTREME, per, 4)
        own_nan = np.isnan(vols).any(axis=(1, 2))
        assert own_nan.sum() == 1
        allowed = own_nan | (overflowing(vols, leaf) if name == "huge_offset" else False)
        off, hits = pkg.cull_brute_force(vols, leaf)
        ref = slices_of(off, hits)
        counts = np.diff(off.astype(np.int64))
        ext = counts[N_VOLUMES:]
        print(f"cull   {name:20s} x {per} planes: {int(off[-1])} records, extreme volumes {ext.tolist()}, not NaN-free {int(allowed.sum())}")
        valid = int((leaf["min"] <= leaf["max"]).all(axis=1).sum())
        assert counts[0] == valid and ext[6] == valid and (ext[:8] > 0).all()           # everything passes the padded scene box and the all -0 padding plane
        pick = list(range(10)) + list(range(10, N_VOLUMES, 7)) + list(range(N_VOLUMES, N_VOLUMES + N_EXTREME))
        for algo, tree in enumerate(trees):
            ok = nan_free(pkg, tree, vols)
            assert not (~ok & ~allowed).any(), f"{name} algo {algo} x {per}: volumes {np.nonzero(~ok & ~allowed)[0].tolist()} have a NaN plane value"
            for i in (pick if algo in (0, 3) else pick[::3]):
                got, _ = lane_walk(pkg, tree, vols[i], False)
                assert got.tobytes() == ref[i].tobytes(), f"{name} algo {algo} volume {i} x {per}: lane walk"
                got, _ = group_walk(pkg, tree, vols[i])
                assert by_prim(got).tobytes() == ref[i].tobytes(), f"{name} algo {algo} volume {i} x {per}: group walk"


def test_the_zero_coefficient_rule_on_inf_vertex(pkg, orc):
    """why the rule exists.  With every product taken (0 * inf = NaN) each ancestor of inf_vertex's infinite leaf fails every plane with a zero coefficient on that
    axis, the padding plane (0, 0, 0, 1) included: on the LBVH tree both host walks lose about half of the mesh, on the HPLOC tree they happen to lose nothing.
    With the rule the walks equal the brute force on both, and the infinite leaf itself passes."""
    tris = mesh(pkg, "inf_vertex"); n = len(tris)

    class Old:
        CULL_HIT = pkg.CULL_HIT
        cull_plane_values = staticmethod(old_plane_values)
    lb = finite_leaf_boxes(pkg, "inf_vertex")
    ctr = 0.5 * (lb["min"].astype(F64).min(axis=0) + lb["max"].astype(F64).max(axis=0))
    vols = {"scene box, 8 planes": volumes_of(pkg, "inf_vertex", 8)[0], "oblique half-space, padded": np.array([(1.0, 1.0, 1.0, -ctr.sum()), PADDING], dtype=F32)}
    for algo in (0, 3):
        t = orc.build_tree(algo, tris)
        tree = Tree(t["nodes"], t["leaves"], t["root"], n, t["layout"])
        valid = (tree.leaf_boxes["min"] <= tree.leaf_boxes["max"]).all(axis=1)
        for what, v in vols.items():
            row = {}
            for rule, P in (("old", Old), ("new", pkg)):
                s_p, _ = P.cull_plane_values(v[:, None, :], tree.leaf_boxes["min"][None], tree.leaf_boxes["max"][None])
                with np.errstate(invalid="ignore"):
                    brute = int((valid & (s_p >= F32(0.0)).all(axis=0)).sum())
                row[rule] = (len(lane_walk(P, tree, v, False)[0]), len(group_walk(P, tree, v)[0]), brute)
            print(f"inf_vertex algo {algo}, {what}: (lane walk, group walk, brute force) old rule {row['old']}, new rule {row['new']}")
            assert row["new"][0] == row["new"][1] == row["new"][2] == row["old"][2] + 1          # the infinite leaf passes now
            if algo == 0:
                assert row["old"][0] == row["old"][1] < 0.6 * row["old"][2]
