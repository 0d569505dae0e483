"""bvh_winding_prepare / bvh_winding_number on the GPU: the per-node moments of every builder, both node layouts and all three triangle formats bit for bit
against the f32 restatement (tests/test_winding.py moments_host), the walk against its restatement (walk_host) and the f64 brute force, inside / outside
classification on a closed mesh, the stackless pass on a tree deeper than the short stack, buffer hygiene, errors and the Python binding."""
import ctypes as C

import numpy as np
import pytest

from test_point_query import E_INVALID, point_brute_force, tri_arrays
from test_winding import WIND_NAN_BITS, moments_host, stack_depth_all_open, walk_host, winding_brute_force
from test_gpu_query import caterpillar, lbvh_result, mesh
from test_gpu_refit import jitter, no_negzero

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

SIZES = [2, 3, 63, 64, 65, 1000, 20_000]
MESHES = [f"uniform_{n}" for n in SIZES] + ["bunny_320", "bunny_1280", "cornell32", "cornell382"]
N_POINTS = 1536
TOL_FLOOR = 2.0 ** -20
TOL_FACTOR = 8.0                                                  # the device atan2f is a few ulp, numpy's is correctly rounded
_MESHES, _REF = {}, {}


def wmesh(pkg, name):
    if name.startswith("bunny"):
        if name not in _MESHES:
            _MESHES[name] = no_negzero(pkg.meshgen.bunny_like(int(name.split("_")[1])))
        return _MESHES[name]
    return mesh(pkg, name)


def make_points(pkg, tris, m, seed):
    """points inside and outside the scene box; the first quarter near the surface (centroids jittered by 1e-2 of the extent); the last 8 have a NaN coordinate"""
    rng = np.random.default_rng(seed)
    v1, v2, v3 = tri_arrays(tris)
    v = np.concatenate([v1, v2, v3]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    p = lo - 0.5 * ext + rng.random((m, 3)) * 2.0 * ext
    k = m // 4
    t = rng.integers(0, len(tris), size=k)
    p[:k] = ((v1[t].astype(np.float64) + v2[t]) + v3[t]) / 3.0 + rng.normal(0, 1e-2, (k, 3)) * ext
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    pts["point"] = p.astype(np.float32)
    pts["radius"] = np.inf
    for j, c in enumerate(range(m - 8, m)):
        pts["point"][c, j % 3] = np.nan
    return pts


def conditioning(pkg, pts, tris):
    """(distance to the surface f64[m] (NaN for dead points), scene diagonal)"""
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(point_brute_force(pkg, pts, tris)["closest"]["dist2"].astype(np.float64))
    dist[np.isnan(pts["point"]).any(axis=1)] = np.nan
    v = np.concatenate(tri_arrays(tris)).astype(np.float64)
    return dist, float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


def reference(pkg, name):
    """(points, distance to the surface, scene diagonal, f64 brute-force winding numbers) per mesh, computed once"""
    if name not in _REF:
        tris = wmesh(pkg, name)
        pts = make_points(pkg, tris, N_POINTS, 31 + len(tris))
        dist, diag = conditioning(pkg, pts, tris)
        _REF[name] = (pts, dist, diag, winding_brute_force(tris, pts["point"]))
    return _REF[name]


def prepare(pkg, ctx, result, inp=None):
    buf = ctx.alloc((result.n_leaves - 1) * 32)
    rc = pkg.lib().bvh_winding_prepare(ctx.handle, C.byref(result), C.byref(inp) if inp is not None else None, buf.ptr)
    assert rc == 0, rc
    return buf


def winding(pkg, ctx, result, mom, pts, beta, inp=None):
    d_pts = ctx.upload(pts)
    w = ctx.alloc(len(pts) * 4)
    try:
        rc = pkg.lib().bvh_winding_number(ctx.handle, C.byref(result), C.byref(inp) if inp is not None else None, mom.ptr, d_pts.ptr, len(pts), beta, w.ptr)
        assert rc == 0, rc
        return w.download(np.float32, len(pts))
    finally:
        d_pts.free(); w.free()


def trees_of(pkg, ctx, b, keep):
    """[(label, result, nodes, leaves, layout)] of a builder: as built and, for a layout-1 tree, its layout-0 copy in a caller's buffer"""
    t = b.download()
    n = b.result.n_leaves
    out = [("as built", b.result, t["nodes"], t["leaves"], t["layout"])]
    if b.result.layout == 1:
        r = lbvh_result(pkg, ctx, b, keep)
        out.append(("lbvh layout", r, keep[-1].download(pkg.BVH2_NODE, 2 * n - 1), None, 0))
    return out


def check_walk(pkg, what, tris, nodes, leaves, layout, root, mom_host, pts, dist, diag, bf, got, beta):
    """checks 2 and 3: on the well-conditioned points |w_gpu - walk_host(f64)| <= 8 * max |walk_host(f32) - walk_host(f64)| (floor 2^-20); at beta = +inf the same
    bound against the f64 brute force; NaN points answer the canonical NaN"""
    xyz = pts["point"]
    dead = np.isnan(xyz).any(axis=1)
    with np.errstate(invalid="ignore"):
        well = dist > 1e-4 * diag
    assert well.mean() >= 0.95, f"{what}: only {well.mean():.4f} of the points are well-conditioned"
    assert (got.view(np.uint32)[dead] == WIND_NAN_BITS).all(), f"{what}: a NaN point does not answer NaN"
    assert not np.isnan(got[~dead]).any(), f"{what}: NaN on a live point"
    w64 = walk_host(nodes, leaves, layout, root, tris, mom_host, xyz, beta, np.float64)
    w32 = walk_host(nodes, leaves, layout, root, tris, mom_host, xyz, beta, np.float32)
    tol = max(TOL_FACTOR * float(np.abs(w32[well].astype(np.float64) - w64[well]).max()), TOL_FLOOR)
    err = float(np.abs(got[well].astype(np.float64) - w64[well]).max())
    print(f"{what} beta {beta}: |gpu - host f64| max {err:.3e}, tol {tol:.3e}, |host f64 - brute| max {float(np.abs(w64[well] - bf[well]).max()):.3e}")
    assert err <= tol, f"{what} beta {beta}: {err:.3e} > {tol:.3e}"
    if np.isinf(beta):
        err = float(np.abs(got[well].astype(np.float64) - bf[well]).max())
        assert err <= tol, f"{what} beta inf against the brute force: {err:.3e} > {tol:.3e}"


@pytest.mark.parametrize("name", MESHES)
def test_moments_bitwise_and_walk_against_the_restatement(pkg, ctx, name):
    tris = wmesh(pkg, name)
    pts, dist, diag, bf = reference(pkg, name)
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        keep = []
        try:
            for label, res, nodes, leaves, layout in trees_of(pkg, ctx, b, keep):
                what = f"{name} algo {algo} {label}"
                mom = prepare(pkg, ctx, res); keep.append(mom)
                host = moments_host(pkg, nodes, leaves, layout, res.root, tris)
                assert mom.download(pkg.WINDING_MOMENT, len(tris) - 1).tobytes() == host.tobytes(), f"{what}: moments differ"
                for beta in (2.0, np.inf):
                    got = winding(pkg, ctx, res, mom, pts, beta)
                    check_walk(pkg, what, tris, nodes, leaves, layout, res.root, host, pts, dist, diag, bf, got, beta)
        finally:
            for k in keep:
                k.free()


def test_formats_give_identical_moments_and_answers(pkg, ctx):
    tris = wmesh(pkg, "uniform_1000"); n = len(tris)
    pts, _, _, _ = reference(pkg, "uniform_1000")
    packed = np.ascontiguousarray(np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1).astype(np.float32).reshape(n, 9))
    uniq, inv = np.unique(packed.reshape(-1, 3), axis=0, return_inverse=True)
    idx = inv.reshape(-1).astype(np.uint32)
    d_p, d_v, d_i = ctx.upload(packed), ctx.upload(np.ascontiguousarray(uniq.astype(np.float32))), ctx.upload(idx)
    keep = [d_p, d_v, d_i]
    try:
        for algo in (1, 3):                                         # a layout-0 and a layout-1 tree
            b = pkg.BUILDERS[algo]().build(ctx, tris)
            t = b.download()
            host = moments_host(pkg, t["nodes"], t["leaves"], t["layout"], b.result.root, tris)
            inputs = {"padded": None, "packed": pkg.BuildInput(pkg.TRI_PACKED36, 30, d_p.ptr, None, None, 0, 0),
                      "indexed": pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, len(uniq), 0)}
            answers = {}
            for fmt, inp in inputs.items():
                mom = prepare(pkg, ctx, b.result, inp); keep.append(mom)
                assert mom.download(pkg.WINDING_MOMENT, n - 1).tobytes() == host.tobytes(), f"algo {algo} {fmt}: moments differ"
                answers[fmt] = winding(pkg, ctx, b.result, mom, pts, 2.0, inp).tobytes()
            assert answers["padded"] == answers["packed"] == answers["indexed"]
    finally:
        for k in keep:
            k.free()


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_moments_after_refit_and_optimize(pkg, algo):
    tris = wmesh(pkg, "uniform_1000"); moved = jitter(tris, 23, 2e-3)
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, tris)
        for step, cur in (("refit", moved), ("optimize", moved)):
            b.refit(moved) if step == "refit" else b.optimize(3)
            keep = []
            for label, res, nodes, leaves, layout in trees_of(pkg, c, b, keep):
                mom = prepare(pkg, c, res); keep.append(mom)
                host = moments_host(pkg, nodes, leaves, layout, res.root, cur)
                assert mom.download(pkg.WINDING_MOMENT, len(tris) - 1).tobytes() == host.tobytes(), f"algo {algo} after {step}, {label}: moments differ"
            for k in keep:
                k.free()
    finally:
        c.close()


def test_classification_on_a_closed_mesh(pkg, ctx):
    """check 4: on bunny_1280 at beta 2, w > 0.5 is the brute force's answer on every point farther than 1e-3 of the diagonal from the surface"""
    tris = wmesh(pkg, "bunny_1280")
    pts, dist, diag, bf = reference(pkg, "bunny_1280")
    with np.errstate(invalid="ignore"):
        clear = dist > 1e-3 * diag
    assert clear.mean() >= 0.9 and 0.02 < (bf[clear] > 0.5).mean() < 0.98
    assert (np.minimum(np.abs(bf[clear]), np.abs(bf[clear] - 1.0)) <= 1e-6).all()      # closed and outward: 0 or 1
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        mom = prepare(pkg, ctx, b.result)
        try:
            got = winding(pkg, ctx, b.result, mom, pts, 2.0)
            t = b.download()
            host = moments_host(pkg, t["nodes"], t["leaves"], t["layout"], b.result.root, tris)
            st = {}
            w64 = walk_host(t["nodes"], t["leaves"], t["layout"], b.result.root, tris, host, pts["point"], 2.0, np.float64, st)
            print(f"bunny_1280 algo {algo} beta 2: host walk max error {float(np.abs(w64[clear] - bf[clear]).max()):.4f}, "
                  f"min |w - 0.5| {float(np.abs(got[clear] - 0.5).min()):.4f}, mean terms {st['terms']:.1f}")
            assert ((got > 0.5) == (bf > 0.5))[clear].all(), f"algo {algo}: {np.count_nonzero(((got > 0.5) != (bf > 0.5)) & clear)} points misclassified"
        finally:
            mom.free()


def test_deep_tree_takes_the_stackless_pass(pkg):
    """check 5: a caterpillar deeper than the 64-entry stack.  At beta = +inf every query opens every node, so every live query overflows the short stack and is
    finished by k_winding_deep; at beta 2 the far side nodes are approximated and the short stack suffices"""
    H = 250
    tris, nodes, root, n = caterpillar(pkg, H, 7 + H)
    assert stack_depth_all_open(nodes, root, n - 1) > 64
    rng = np.random.default_rng(H)
    m = 300
    pts = np.zeros(m, dtype=pkg.POINT_QUERY)
    pts["point"] = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-3, -0.5, m)], axis=1)
    pts["point"][m // 2:, 2] = 1000.5 + rng.integers(0, 2 * H - 1, m - m // 2)        # between two of the far triangles
    pts["point"][-1, 0] = np.nan
    pts["radius"] = np.inf
    dist, diag = conditioning(pkg, pts, tris)
    bf = winding_brute_force(tris, pts["point"])
    c = pkg.Context(0)
    try:
        c.reserve(n)
        d_nodes, d_tris = c.upload(nodes), c.upload(tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        c.set_profiling(2)
        mom = prepare(pkg, c, r)
        host = moments_host(pkg, nodes, None, 0, root, tris)
        assert mom.download(pkg.WINDING_MOMENT, n - 1).tobytes() == host.tobytes()
        for beta in (2.0, np.inf):
            got = winding(pkg, c, r, mom, pts, beta)
            check_walk(pkg, f"caterpillar {H}", tris, nodes, None, 0, root, host, pts, dist, diag, bf, got, beta)
        kt = c.kernel_times()
        c.set_profiling(0)
        assert {"k_winding_climb", "k_winding_finish", "k_winding", "k_winding_deep", "k_refit_plan"} <= set(kt)
        for x in (mom, d_nodes, d_tris):
            x.free()
    finally:
        c.close()


def test_buffers_untouched_outside_the_answers(pkg, ctx):
    tris = wmesh(pkg, "uniform_1000"); n = len(tris)
    pts, _, _, _ = reference(pkg, "uniform_1000")
    m = len(pts)
    b = pkg.HPLOC().build(ctx, tris)
    L = pkg.lib()
    guard = 64
    sent_m = np.full(2 * guard + (n - 1) * 32, 0xA5, dtype=np.uint8)
    sent_w = np.full(2 * guard + m * 4, 0x5A, dtype=np.uint8)
    d_m, d_w, d_pts = ctx.upload(sent_m), ctx.upload(sent_w), ctx.upload(pts)
    try:
        assert L.bvh_winding_prepare(ctx.handle, C.byref(b.result), None, d_m.ptr + guard) == 0
        out_m = d_m.download(np.uint8, len(sent_m))
        assert (out_m[:guard] == 0xA5).all() and (out_m[-guard:] == 0xA5).all()
        t = b.download()
        assert out_m[guard:-guard].tobytes() == moments_host(pkg, t["nodes"], t["leaves"], t["layout"], b.result.root, tris).tobytes()
        # n_points == 0: returns 0 and writes nothing
        assert L.bvh_winding_number(ctx.handle, C.byref(b.result), None, d_m.ptr + guard, d_pts.ptr, 0, 2.0, d_w.ptr + guard) == 0
        assert d_w.download(np.uint8, len(sent_w)).tobytes() == sent_w.tobytes()
        runs = []
        for _ in range(2):
            d_w.upload(sent_w)
            assert L.bvh_winding_number(ctx.handle, C.byref(b.result), None, d_m.ptr + guard, d_pts.ptr, m, 2.0, d_w.ptr + guard) == 0
            out_w = d_w.download(np.uint8, len(sent_w))
            assert (out_w[:guard] == 0x5A).all() and (out_w[-guard:] == 0x5A).all()
            runs.append(out_w[guard:-guard].tobytes())
        assert runs[0] == runs[1]                                   # two calls on the same arrays: the same bytes
        w = np.frombuffer(runs[0], dtype=np.float32)
        dead = np.isnan(pts["point"]).any(axis=1)
        assert dead.sum() == 8 and (w.view(np.uint32)[dead] == WIND_NAN_BITS).all() and not np.isnan(w[~dead]).any()
        assert d_m.download(np.uint8, len(sent_m)).tobytes() == out_m.tobytes()          # the query leaves the moments alone
        assert d_pts.download(pkg.POINT_QUERY, m).tobytes() == pts.tobytes()
    finally:
        for x in (d_m, d_w, d_pts):
            x.free()


def test_errors_write_nothing(pkg):
    tris = wmesh(pkg, "uniform_1000"); n = len(tris)
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        assert b.result.layout == 1
        pts, _, _, _ = reference(pkg, "uniform_1000")
        pts = pts[:256]
        d_pts = c.upload(pts)
        sent_m = np.full((n - 1) * 32, 0xA5, dtype=np.uint8); sent_w = np.full(256 * 4, 0x5A, dtype=np.uint8)
        d_m, d_w = c.upload(sent_m), c.upload(sent_w)
        L = pkg.lib()

        def prep(res=b.result, inp=None, mom=d_m.ptr, ctx=c.handle):
            return L.bvh_winding_prepare(ctx, C.byref(res) if res is not None else None, C.byref(inp) if inp is not None else None, mom)

        def call(res=b.result, inp=None, mom=d_m.ptr, p=d_pts.ptr, m=256, beta=2.0, w=d_w.ptr, ctx=c.handle):
            return L.bvh_winding_number(ctx, C.byref(res) if res is not None else None, C.byref(inp) if inp is not None else None, mom, p, m, beta, w)

        def variant(**kw):
            r = pkg.Result.from_buffer_copy(b.result)
            for k, v in kw.items():
                setattr(r, k, v)
            return r
        nodes_bytes = (n - 1) * 32
        cases = {
            "prepare: null ctx": prep(ctx=None), "prepare: null tree": prep(res=None), "prepare: null moments": prep(mom=None),
            "prepare: n_leaves 1": prep(res=variant(n_leaves=1)), "prepare: layout 2": prep(res=variant(layout=2)),
            "prepare: null nodes": prep(res=variant(d_nodes=None)), "prepare: layout 1 without leaves": prep(res=variant(d_leaves=None)),
            "prepare: root not internal": prep(res=variant(root=n - 1)), "prepare: no triangles": prep(res=variant(d_tris=None)),
            "prepare: bad format": prep(inp=pkg.BuildInput(7, 30, b.result.d_tris, None, None, 0, 0)),
            "prepare: moments unaligned": prep(mom=d_m.ptr + 4),
            "prepare: moments over the nodes": prep(mom=b.result.d_nodes + nodes_bytes - 32),
            "prepare: moments over the leaves": prep(mom=(b.result.d_leaves + 15) & ~15),
            "prepare: moments over the triangles": prep(mom=b.result.d_tris + 64 * (n - 1)),
            "prepare: above capacity": prep(res=variant(n_leaves=n + 1_000_000, root=0)),
            "null ctx": call(ctx=None), "null tree": call(res=None), "null moments": call(mom=None), "null points": call(p=None), "null w": call(w=None),
            "beta -1": call(beta=-1.0), "beta -inf": call(beta=-np.inf), "beta nan": call(beta=np.nan),
            "n_leaves 1": call(res=variant(n_leaves=1)), "layout 2": call(res=variant(layout=2)), "root not internal": call(res=variant(root=n - 1)),
            "no triangles": call(res=variant(d_tris=None)),
            "moments over the points": call(mom=d_pts.ptr), "moments over w": call(mom=d_w.ptr),
            "moments over the nodes": call(mom=b.result.d_nodes), "moments over the triangles": call(mom=b.result.d_tris),
            "w over the points": call(w=d_pts.ptr + 16), "w over the moments": call(w=d_m.ptr + 32), "w over the nodes": call(w=b.result.d_nodes + 64),
            "w over the triangles": call(w=b.result.d_tris), "above capacity": call(res=variant(n_leaves=n + 1_000_000, root=0)),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        c2 = pkg.Context(0)                                         # a fresh ctx (capacity 0) refuses a caller tree until bvh_ctx_reserve
        try:
            assert L.bvh_winding_prepare(c2.handle, C.byref(b.result), None, d_m.ptr) == E_INVALID
        finally:
            c2.close()
        c.synchronize()
        assert d_m.download(np.uint8, len(sent_m)).tobytes() == sent_m.tobytes()
        assert d_w.download(np.uint8, len(sent_w)).tobytes() == sent_w.tobytes()
        for x in (d_pts, d_m, d_w):
            x.free()
    finally:
        c.close()


def test_python_binding(pkg):
    tris = wmesh(pkg, "bunny_1280"); moved = jitter(tris, 5, 2e-3)
    pts, _, _, _ = reference(pkg, "bunny_1280")
    xyz = np.ascontiguousarray(pts["point"])
    c = pkg.Context(0)
    try:
        b = pkg.HPLOC().build(c, tris)
        w = b.winding_number(xyz)                                   # prepares on first use
        assert w.dtype == np.float32 and w.shape == (len(xyz),)
        kept = b._winding[1]
        assert w.tobytes() == winding(pkg, c, b.result, kept, pts, 2.0).tobytes()           # the C call's bytes
        assert b.winding_number(pts, beta=3.0).tobytes() == winding(pkg, c, b.result, kept, pts, 3.0).tobytes()
        assert b._winding[1] is kept                                # ... from the kept moments
        d = c.upload(pts)
        assert b.winding_number(d).tobytes() == w.tobytes()
        d.free()
        sd, hits = b.signed_distance(xyz)
        cp = b.closest_point(xyz)
        assert hits.tobytes() == cp.tobytes()
        with np.errstate(invalid="ignore"):
            want = np.where(w > np.float32(0.5), -np.sqrt(cp["dist2"]), np.sqrt(cp["dist2"])).astype(np.float32)
        assert sd.tobytes() == want.tobytes() and (sd < 0).any() and (sd > 0).any()
        # after a refit the kept moments are dropped and made again: the same as a fresh prepare on the refit tree
        b.refit(moved)
        assert b._winding is None
        w2 = b.winding_number(xyz)
        fresh = prepare(pkg, c, b.result)
        assert w2.tobytes() == winding(pkg, c, b.result, fresh, pts, 2.0).tobytes()
        assert b._winding[1].download(pkg.WINDING_MOMENT, len(tris) - 1).tobytes() == fresh.download(pkg.WINDING_MOMENT, len(tris) - 1).tobytes()
        assert w2.tobytes() != w.tobytes()
        fresh.free()
        b.optimize(2)
        assert b._winding is None
        assert b.winding_number(np.zeros((0, 3), dtype=np.float32)).shape == (0,)
    finally:
        c.close()
