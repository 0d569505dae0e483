"""bvh_intersect on the GPU: closest-hit and any-hit answers of every builder, both node layouts and all three triangle formats against the numpy brute force
(tests/test_query.py), the stackless pass on trees deeper than the short stack, queries after a refit and a rebuild, large sizes, buffer hygiene and errors."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_query import E_INVALID, brute_force, recompute
from test_gpu_refit import jitter, no_negzero

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

SIZES = [2, 3, 63, 64, 65, 1000, 20_000]


def make_rays(pkg, tris, m, seed):
    """a mix: random origins inside and outside the scene box towards random points of it, axis-parallel rays (zero components), origins on triangles' box
    planes, tmin / tmax windows, tmin < 0, tmax == tmin, NaN components"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([tris["v1"], tris["v2"], tris["v3"]]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    o = lo - 0.5 * ext + rng.random((m, 3)) * 2.0 * ext
    target = lo + rng.random((m, 3)) * ext
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True) + 1e-30
    r = np.zeros(m, dtype=pkg.RAY)
    r["tmin"] = 0.0; r["tmax"] = np.float32(3.0e38)
    k = m // 8
    # axis-parallel: one or two zero components
    for j in range(k):
        zero = rng.choice(3, size=1 + j % 2, replace=False)
        d[j, zero] = 0.0
        if not d[j].any():
            d[j, (zero[0] + 1) % 3] = 1.0
    # origins on box planes: one coordinate copied from a triangle vertex's coordinate (a leaf box's plane)
    pick = rng.integers(0, len(v), size=k)
    ax = rng.integers(0, 3, size=k)
    o[k + np.arange(k), ax] = v[pick, ax]
    d[k + np.arange(k // 2), ax[: k // 2]] = 0.0                  # (half of them also run inside that plane)
    r["origin"] = o.astype(np.float32); r["direction"] = d.astype(np.float32)
    # windows
    w = slice(2 * k, 3 * k)
    span = float(np.linalg.norm(ext)) * 2.0
    r["tmin"][w] = rng.random(k) * span; r["tmax"][w] = r["tmin"][w] + rng.random(k) * span
    r["tmin"][3 * k: 3 * k + k // 2] = -rng.random(k // 2) * span                                 # tmin < 0
    r["tmax"][3 * k + k // 2: 4 * k] = r["tmin"][3 * k + k // 2: 4 * k]                           # tmax == tmin: empty
    nan = rng.integers(0, 8, size=8)
    for j, c in enumerate(range(m - 8, m)):                                                       # NaN components (origin, direction, tmin, tmax)
        if nan[j] < 3:
            r["origin"][c, nan[j]] = np.nan
        elif nan[j] < 6:
            r["direction"][c, nan[j] - 3] = np.nan
        elif nan[j] == 6:
            r["tmin"][c] = np.nan
        else:
            r["tmax"][c] = np.nan
    return r


def camera_rays(pkg, ctx, W=32):
    cam, _ = pkg.cornell_view()
    ctx.reserve(2)                                            # (the camera record is staged in the ctx's arena)
    buf = ctx.alloc(W * W * 32)
    assert pkg.lib().bvh_generate_rays(ctx.handle, np.ascontiguousarray(cam).ctypes.data, buf.ptr, W, W) == 0
    out = buf.download(pkg.RAY, W * W)
    buf.free()
    return out


_MESHES = {}


def mesh(pkg, name):
    if name not in _MESHES:
        if name.startswith("cornell"):
            t = pkg.meshgen.load_tri(os.path.join(GOLDEN, name + ".tri"))
        else:
            kind, n = name.split("_"); n = int(n)
            t = pkg.meshgen.sponza_like(n, 3) if kind == "sponza" else pkg.meshgen.uniform(n, 5 + n % 11)
        _MESHES[name] = no_negzero(t)
    return _MESHES[name]


MESHES = [f"uniform_{n}" for n in SIZES] + ["sponza_1000", "sponza_20000", "cornell32", "cornell82", "cornell382"]
_REF = {}


def reference(pkg, ctx, name):
    """(rays, brute force) per mesh, computed once"""
    if name not in _REF:
        tris = mesh(pkg, name)
        rays = np.concatenate([make_rays(pkg, tris, 1536, 7 + len(tris)), camera_rays(pkg, ctx)])
        _REF[name] = (rays, brute_force(rays, tris))
    return _REF[name]


def lbvh_result(pkg, ctx, b, keep):
    """a caller-filled layout-0 result: bvh_to_lbvh_layout of a PLOC-layout tree in a buffer of the caller's"""
    n = b.result.n_leaves
    buf = ctx.alloc((2 * n - 1) * 32); keep.append(buf)
    assert pkg.lib().bvh_to_lbvh_layout(ctx.handle, C.byref(b.result), buf.ptr) == 0
    r = pkg.Result.from_buffer_copy(b.result)
    r.d_nodes = buf.ptr; r.d_leaves = None; r.layout = 0
    return r


def query(pkg, ctx, result, rays, kind, inp=None):
    d_rays = ctx.upload(rays)
    hits = ctx.alloc(len(rays) * 16)
    try:
        rc = pkg.lib().bvh_intersect(ctx.handle, C.byref(result), C.byref(inp) if inp is not None else None, d_rays.ptr, len(rays), hits.ptr, kind)
        assert rc == 0, rc
        return hits.download(pkg.HIT, len(rays))
    finally:
        d_rays.free(); hits.free()


def check_exact(pkg, rays, tris, bf, closest, anyhit, what):
    well = bf["well"]
    assert well.mean() >= 0.99, f"{what}: only {well.mean():.4f} of the rays are well-conditioned"
    ref = bf["closest"]
    for f in ("t", "u", "v"):
        eq = closest[f].view(np.uint32) == ref[f].view(np.uint32)
        assert eq[well].all(), f"{what}: closest {f} differs on {np.count_nonzero(~eq & well)} well-conditioned rays"
    assert (closest["prim"] == ref["prim"])[well].all(), f"{what}: closest prim differs on {np.count_nonzero((closest['prim'] != ref['prim']) & well)} rays"
    hit_any = anyhit["prim"] != pkg.INVALID
    assert (hit_any == bf["hit"])[well].all(), f"{what}: any-hit hit/miss differs"
    # every ray: reported hits are accepted hits with bit-equal t / u / v; a closest hit is never lexicographically below the brute force's best
    assert recompute(rays, tris, closest).all(), f"{what}: a closest hit is not an accepted hit of its prim"
    assert recompute(rays, tris, anyhit).all(), f"{what}: an any hit is not an accepted hit of its prim"
    got = closest["prim"] != pkg.INVALID
    below = got & ((closest["t"] < ref["t"]) | ((closest["t"] == ref["t"]) & (closest["prim"] < ref["prim"])))
    assert not below.any() and not (got & ~bf["hit"]).any(), f"{what}: closest below the brute force"


@pytest.mark.parametrize("name", MESHES)
def test_exact_against_brute_force(pkg, ctx, name):
    tris = mesh(pkg, name)
    rays, bf = reference(pkg, ctx, name)
    per_algo = {}
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        keep = []
        results = [("as built", b.result)]
        if b.result.layout == 1:
            results.append(("lbvh layout", lbvh_result(pkg, ctx, b, keep)))
        for label, res in results:
            c = query(pkg, ctx, res, rays, pkg.QUERY_CLOSEST)
            a = query(pkg, ctx, res, rays, pkg.QUERY_ANY)
            check_exact(pkg, rays, tris, bf, c, a, f"{name} algo {algo} {label}")
            per_algo.setdefault(algo, c)
        assert b.intersect(rays, "closest").tobytes() == per_algo[algo].tobytes()      # the Python binding, host rays
        for k in keep:
            k.free()
    well = bf["well"]
    for algo in (1, 2, 3):
        assert per_algo[algo][well].tobytes() == per_algo[0][well].tobytes(), f"{name}: builders {algo} and 0 differ"


@pytest.mark.parametrize("name", ["uniform_1000", "sponza_20000", "cornell382"])
def test_formats_give_identical_hits(pkg, ctx, name):
    tris = mesh(pkg, name); n = len(tris)
    rays, bf = reference(pkg, ctx, name)
    b = pkg.HPLOC().build(ctx, tris)
    packed = np.ascontiguousarray(np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1).astype(np.float32).reshape(n, 9))
    verts = packed.reshape(-1, 3)
    uniq, inv = np.unique(verts, axis=0, return_inverse=True)
    idx = inv.reshape(-1).astype(np.uint32)
    d_p, d_v, d_i = ctx.upload(packed), ctx.upload(np.ascontiguousarray(uniq.astype(np.float32))), ctx.upload(idx)
    try:
        for kind in (pkg.QUERY_CLOSEST, pkg.QUERY_ANY):
            base = query(pkg, ctx, b.result, rays, kind)
            p = query(pkg, ctx, b.result, rays, kind, pkg.BuildInput(pkg.TRI_PACKED36, 30, d_p.ptr, None, None, 0, 0))
            i = query(pkg, ctx, b.result, rays, kind, pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, len(uniq), 0))
            assert base.tobytes() == p.tobytes() == i.tobytes()
            assert b.intersect(rays, kind, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED).tobytes() == base.tobytes()
        # a tree built FROM indexed input answers the same
        bi = pkg.PLOCNew().build_ex(ctx, n, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED)
        got = bi.intersect(rays, "closest", vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED)
        assert got[bf["well"]].tobytes() == bf["closest"][bf["well"]].tobytes()
    finally:
        for x in (d_p, d_v, d_i):
            x.free()


def caterpillar(pkg, H, seed):
    """a layout-0 tree of height > H over 2H + 2 parallel triangles: chain node c_i has children c_{i+1} (nearer: its subtree holds the two triangles at z = 0 and 0.5)
    and a side node s_i over two triangles far along +z; left / right shuffled, internal ids shuffled.  Returns (tris, nodes, root, n)."""
    rng = np.random.default_rng(seed)
    n = 2 * H + 2; ni = n - 1
    z = np.concatenate([[0.0, 0.5], 1000.0 + np.arange(2 * H)]).astype(np.float32)
    tris = np.zeros(n, dtype=pkg.meshgen.TRIANGLE)
    tris["v1"] = np.stack([np.full(n, -10.0), np.full(n, -10.0), z], axis=1); tris["v2"] = np.stack([np.full(n, 30.0), np.full(n, -10.0), z], axis=1)
    tris["v3"] = np.stack([np.full(n, -10.0), np.full(n, 30.0), z], axis=1)
    prim_of_leaf = rng.permutation(n)                         # leaf j holds prim prim_of_leaf[j]
    leaf_of_prim = np.argsort(prim_of_leaf)
    ids = rng.permutation(ni)                                 # chain c_i -> ids[i], side s_i -> ids[H + i], bottom -> ids[2H]
    kids = {}
    for i in range(H):
        nxt = ids[i + 1] if i + 1 < H else ids[2 * H]
        kids[ids[H + i]] = (ni + leaf_of_prim[2 + 2 * i], ni + leaf_of_prim[3 + 2 * i])
        kids[ids[i]] = (nxt, ids[H + i])
    kids[ids[2 * H]] = (ni + leaf_of_prim[0], ni + leaf_of_prim[1])
    nodes = np.zeros(2 * n - 1, dtype=pkg.BVH2_NODE)
    lo = np.minimum(np.minimum(tris["v1"], tris["v2"]), tris["v3"]); hi = np.maximum(np.maximum(tris["v1"], tris["v2"]), tris["v3"])
    nodes["left"][ni:] = prim_of_leaf; nodes["right"][ni:] = pkg.INVALID
    nodes["min"][ni:] = lo[prim_of_leaf]; nodes["max"][ni:] = hi[prim_of_leaf]
    order = [ids[2 * H]] + [ids[H + i] for i in range(H)][::-1]
    for i in reversed(range(H)):
        order.append(ids[i])
    for v in order:                                            # children before parents
        a, bb = kids[v]
        if rng.random() < 0.5:
            a, bb = bb, a
        nodes["left"][v], nodes["right"][v] = a, bb
        nodes["min"][v] = np.minimum(nodes["min"][a], nodes["min"][bb]); nodes["max"][v] = np.maximum(nodes["max"][a], nodes["max"][bb])
    return tris, nodes, int(ids[0]), n


def tree_height_and_stack(nodes, root, ni, o, d):
    """height, and the deepest short stack near-first traversal reaches for a ray that enters every box (both internal children always pushed / entered)"""
    height, stack_max = 0, 0
    work = [(root, 1, 0)]
    while work:
        v, depth, st = work.pop()
        height = max(height, depth); stack_max = max(stack_max, st)
        if v >= ni:
            continue
        l, r = int(nodes["left"][v]), int(nodes["right"][v])
        internal = [c for c in (l, r) if c < ni]
        for c in (l, r):
            if c >= ni:
                work.append((c, depth + 1, st))
        if len(internal) == 2:
            tn = [(nodes["min"][c][2] - o[2]) / d[2] for c in internal]
            near, far = (internal[0], internal[1]) if tn[0] <= tn[1] else (internal[1], internal[0])
            work.append((far, depth + 1, st)); work.append((near, depth + 1, st + 1))
        else:
            for c in internal:
                work.append((c, depth + 1, st))
    return height, stack_max


@pytest.mark.parametrize("H", [70, 250])
def test_deep_tree_takes_the_stackless_pass(pkg, H):
    tris, nodes, root, n = caterpillar(pkg, H, 3 + H)
    height, depth = tree_height_and_stack(nodes, root, n - 1, (0.0, 0.0, -1.0), (0.0, 0.0, 1.0))
    assert height > 200 or H < 200
    assert depth > 64, depth
    rng = np.random.default_rng(H)
    m = 300
    rays = np.zeros(m, dtype=pkg.RAY)
    rays["origin"] = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), np.full(m, -1.0)], axis=1)
    rays["direction"] = np.stack([rng.normal(0, 1e-3, m), rng.normal(0, 1e-3, m), np.ones(m)], axis=1)
    rays["direction"][: m // 4, :2] = 0.0                     # exactly axis-parallel
    rays["tmax"] = 1e30
    rays["tmin"][m // 2:] = rng.uniform(0, 1000 + 2 * H, m - m // 2)     # windows reach into the far side nodes
    bf = brute_force(rays, tris)
    assert bf["well"].all()
    c = pkg.Context(0)
    try:
        c.reserve(n)
        d_nodes, d_tris = c.upload(nodes), c.upload(tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        c.set_profiling(2)
        closest = query(pkg, c, r, rays, pkg.QUERY_CLOSEST)
        anyhit = query(pkg, c, r, rays, pkg.QUERY_ANY)
        kt = c.kernel_times()
        c.set_profiling(0)
        assert {"k_intersect", "k_intersect_deep", "k_refit_plan"} <= set(kt)
        assert closest.tobytes() == bf["closest"].tobytes()
        assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"]).all() and recompute(rays, tris, anyhit).all()
        d_nodes.free(); d_tris.free()
    finally:
        c.close()


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_query_after_refit_and_rebuild(pkg, algo):
    a = mesh(pkg, "uniform_20000"); moved = jitter(a, 17, 2e-3)
    other = mesh(pkg, "sponza_20000")
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        rays = make_rays(pkg, moved, 1024, 5)
        b.intersect(rays)                                     # (the plan of the ctx's own tree is made here and kept)
        b.refit(moved)
        bf = brute_force(rays, moved)
        check_exact(pkg, rays, moved, bf, b.intersect(rays, "closest"), b.intersect(rays, "any"), f"refit algo {algo}")
        b2 = pkg.BUILDERS[algo]().build(c, other)
        rays2 = make_rays(pkg, other, 1024, 6)
        bf2 = brute_force(rays2, other)
        check_exact(pkg, rays2, other, bf2, b2.intersect(rays2, "closest"), b2.intersect(rays2, "any"), f"rebuild algo {algo}")
    finally:
        c.close()


@pytest.mark.parametrize("name,n", [("sponza", 262_144), ("uniform", 2_000_000)])
def test_large_trees(pkg, ctx, name, n):
    tris = no_negzero(pkg.meshgen.sponza_like(n, 3) if name == "sponza" else pkg.meshgen.uniform(n, 9))
    m = 1_000_003
    rays = make_rays(pkg, tris, m, 21)
    res = {}
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        c, a = b.intersect(rays, "closest"), b.intersect(rays, "any")
        assert recompute(rays, tris, c).all() and recompute(rays, tris, a).all()
        agree = (c["prim"] != pkg.INVALID) == (a["prim"] != pkg.INVALID)
        assert agree.mean() >= 0.999, f"any / closest hit-miss agree on {agree.mean():.5f}"
        res[algo] = c
    for algo in (1, 2, 3):
        same = (res[algo].view(np.uint32).reshape(-1, 4) == res[0].view(np.uint32).reshape(-1, 4)).all(axis=1)
        assert same.mean() >= 0.999, f"builders {algo} / 0 agree on {same.mean():.5f}"
    sample = np.random.default_rng(1).choice(m, 64, replace=False)
    bf = brute_force(rays[sample], tris)
    well = bf["well"]
    assert well.mean() >= 0.95
    assert res[3][sample][well].tobytes() == bf["closest"][well].tobytes()


def test_buffers_untouched_outside_the_hits(pkg, ctx):
    tris = mesh(pkg, "uniform_1000")
    b = pkg.HPLOC().build(ctx, tris)
    rays = make_rays(pkg, tris, 1000, 3)
    d_rays = ctx.upload(rays)
    extra = 37
    sentinel = np.frombuffer(np.full((len(rays) + extra) * 16, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.HIT)
    hits = ctx.upload(sentinel)
    try:
        for kind in (0, 1):
            assert pkg.lib().bvh_intersect(ctx.handle, C.byref(b.result), None, d_rays.ptr, len(rays), hits.ptr, kind) == 0
            out = hits.download(pkg.HIT, len(rays) + extra)
            assert out[len(rays):].tobytes() == sentinel[len(rays):].tobytes()
            assert recompute(rays, tris, out[: len(rays)]).all()
            assert d_rays.download(pkg.RAY, len(rays)).tobytes() == rays.tobytes()
        hits.upload(sentinel)
        assert pkg.lib().bvh_intersect(ctx.handle, C.byref(b.result), None, d_rays.ptr, 0, hits.ptr, 0) == 0      # n_rays == 0: nothing touched
        assert hits.download(pkg.HIT, len(rays) + extra).tobytes() == sentinel.tobytes()
    finally:
        d_rays.free(); hits.free()


def test_errors_write_nothing(pkg):
    tris = mesh(pkg, "uniform_1000"); n = len(tris)
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        rays = make_rays(pkg, tris, 256, 4)
        d_rays = c.upload(rays)
        sentinel = np.frombuffer(np.full(256 * 16, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.HIT)
        hits = c.upload(sentinel)
        L = pkg.lib()

        def call(res=b.result, inp=None, r=d_rays.ptr, m=256, h=hits.ptr, q=0, ctx=c.handle):
            return L.bvh_intersect(ctx, C.byref(res) if res is not None else None, C.byref(inp) if inp is not None else None, r, m, h, q)

        def variant(**kw):
            r = pkg.Result.from_buffer_copy(b.result)
            for k, v in kw.items():
                setattr(r, k, v)
            return r
        cases = {
            "null ctx": call(ctx=None), "null tree": call(res=None), "null rays": call(r=None), "null hits": call(h=None),
            "n_leaves 1": call(res=variant(n_leaves=1)), "layout 2": call(res=variant(layout=2)), "null nodes": call(res=variant(d_nodes=None)),
            "layout 1 without leaves": call(res=variant(d_leaves=None)), "root not internal": call(res=variant(root=n - 1)),
            "no triangles": call(res=variant(d_tris=None)), "bad format": call(inp=pkg.BuildInput(7, 30, b.result.d_tris, None, None, 0, 0)),
            "packed unaligned": call(inp=pkg.BuildInput(pkg.TRI_PACKED36, 30, b.result.d_tris + 4, None, None, 0, 0)),
            "indexed without vertices": call(inp=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, None, b.result.d_tris, 3, 0)),
            "query 2": call(q=2), "query -1": call(q=-1),
            "overlap": call(h=d_rays.ptr + 16), "above capacity": call(res=variant(n_leaves=n + 1_000_000, root=0)),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        c.synchronize()
        assert hits.download(pkg.HIT, 256).tobytes() == sentinel.tobytes()
        # on a fresh ctx (capacity 0) a caller tree is refused until bvh_ctx_reserve
        c2 = pkg.Context(0)
        try:
            assert L.bvh_intersect(c2.handle, C.byref(b.result), None, d_rays.ptr, 256, hits.ptr, 0) == E_INVALID
        finally:
            c2.close()
        assert hits.download(pkg.HIT, 256).tobytes() == sentinel.tobytes()
        d_rays.free(); hits.free()
    finally:
        c.close()
