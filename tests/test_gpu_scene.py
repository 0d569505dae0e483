"""Instanced scenes on the GPU (bvh_scene_*): closest-hit and any-hit answers against the two-level numpy brute force (tests/test_scene.py) for 1 to 1000
instances over BLASes of every builder and triangle format built on other contexts, independence from the builders, one identity instance against
bvh_intersect, deep BLASes through the stackless pass, bvh_scene_update after moves and after a BLAS refit, rejections and buffer hygiene."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_query import caterpillar, make_rays
from test_gpu_refit import jitter, no_negzero
from test_query import E_INVALID
from test_scene import identity, instance_inverse, make_instances, mat34, rot, scene_brute_force, scene_recompute, xf_points

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32


class Blases:
    """bottom-level trees, each built on a context of its own (never the scene's), in a chosen triangle format"""

    def __init__(self, pkg):
        self.pkg, self.ctxs, self.bufs = pkg, [], []

    def add(self, algo, tris, fmt=0):
        pkg = self.pkg
        c = pkg.Context(0); self.ctxs.append(c)
        n = len(tris)
        flat = np.ascontiguousarray(np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1).reshape(n, 9), dtype=F32)
        if fmt == pkg.TRI_PADDED64:
            return pkg.BUILDERS[algo]().build(c, tris)
        if fmt == pkg.TRI_PACKED36:
            d = c.upload(flat); self.bufs.append(d)
            return pkg.BUILDERS[algo]().build_ex(c, n, tris=d, tri_format=fmt), pkg.BuildInput(fmt, 30, d.ptr, None, None, 0, 0)
        dv = c.upload(flat.reshape(3 * n, 3)); di = c.upload(np.arange(3 * n, dtype=np.uint32).reshape(n, 3)); self.bufs += [dv, di]
        return (pkg.BUILDERS[algo]().build_ex(c, n, vertices=dv, indices=di, n_vertices=3 * n, tri_format=fmt),
                pkg.BuildInput(fmt, 30, None, dv.ptr, di.ptr, 3 * n, 0))

    def close(self):
        for b in self.bufs:
            b.free()
        for c in self.ctxs:
            c.close()


def transform(rng, kind, t):
    if kind == "identity":
        return identity()
    A = np.eye(3)
    if kind in ("rotation", "scale", "mirror"):
        A = rot(rng.integers(3), rng.uniform(0, 2 * np.pi)) @ rot(rng.integers(3), rng.uniform(0, 2 * np.pi))
    if kind == "scale":
        A = A @ np.diag(rng.uniform(0.25, 4.0, 3))
    if kind == "mirror":
        A = A @ np.diag([-1.0, 1.0, 1.0])
    return mat34(A, t)


KINDS = ["identity", "translation", "rotation", "scale", "mirror"]


def scene_instances(pkg, rng, n_inst, n_blas, spacing, specials=True):
    side = int(np.ceil(n_inst ** (1 / 3)))
    mats, blas = [], []
    for k in range(n_inst):
        kind = KINDS[k % len(KINDS)]
        t = np.array([k % side, (k // side) % side, k // (side * side)], dtype=np.float64) * spacing + rng.uniform(-0.2, 0.2, 3) * spacing
        mats.append(transform(rng, kind, t)); blas.append(k % n_blas)
    inst = make_instances(pkg, mats, blas)
    if specials and n_inst >= 3:                               # never hit: singular, NaN, blas out of range (3 instances: the singular one only)
        inst["object_to_world"][-1] = mat34(np.zeros((3, 3)), (1, 1, 1))
    if specials and n_inst > 3:
        inst["object_to_world"][-2][5] = np.nan
        inst["blas"][-3] = n_blas + 5
    return inst


def world_tris(pkg, blas_tris, inst):
    _, active = instance_inverse(inst["object_to_world"])
    active &= inst["blas"] < len(blas_tris)
    parts = []
    for k in np.nonzero(active)[0]:
        t = blas_tris[inst["blas"][k]]
        w = np.zeros(len(t), dtype=pkg.meshgen.TRIANGLE)
        for f in ("v1", "v2", "v3"):
            w[f] = xf_points(inst["object_to_world"][k], t[f])
        parts.append(w)
    return np.concatenate(parts)


def root_boxes(pkg, blases):
    out = []
    for b in blases:
        b = b[0] if isinstance(b, tuple) else b
        nd = b.download()["nodes"][b.result.root]
        out.append(np.concatenate([nd["min"], nd["max"]]).astype(F32))
    return out


def check_exact(pkg, rays, blas_tris, inst, bf, closest, anyhit, what):
    well = bf["well"]
    assert well.mean() >= 0.99, f"{what}: only {well.mean():.4f} of the rays are well-conditioned"
    ref = bf["closest"]
    for f in ("t", "u", "v"):
        eq = closest[f].view(np.uint32) == ref[f].view(np.uint32)
        assert eq[well].all(), f"{what}: closest {f} differs on {np.count_nonzero(~eq & well)} well-conditioned rays"
    for f in ("prim", "instance"):
        assert (closest[f] == ref[f])[well].all(), f"{what}: closest {f} differs on {np.count_nonzero((closest[f] != ref[f]) & well)} rays"
    assert (closest["reserved"] == 0).all()
    assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"])[well].all(), f"{what}: any-hit hit / miss differs"
    assert scene_recompute(pkg, rays, blas_tris, inst, closest).all(), f"{what}: a closest hit is not an accepted hit"
    assert scene_recompute(pkg, rays, blas_tris, inst, anyhit).all(), f"{what}: an any hit is not an accepted hit"


MESH_SIZES = {1: [300, 200, 250, 150], 2: [300, 200, 250, 150], 3: [200, 150, 120, 100], 64: [120, 100, 80, 60], 1000: [24, 20, 16, 12]}
TLAS_ALGO = {1: 3, 2: 0, 3: 1, 64: 2, 1000: 3}


@pytest.mark.parametrize("n_inst", [1, 2, 3, 64, 1000])
def test_exact_against_brute_force(pkg, n_inst):
    rng = np.random.default_rng(n_inst)
    meshes = [no_negzero(pkg.meshgen.uniform(n, 31 + n)) for n in MESH_SIZES[n_inst]]
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo], fmt=algo % 3) for algo in range(4)]
        inst = scene_instances(pkg, rng, n_inst, 4, 1.5)
        scene = pkg.Scene(sc_ctx).build(TLAS_ALGO[n_inst], blases, inst)
        rays = make_rays(pkg, world_tris(pkg, meshes, inst), 512 if n_inst == 1000 else 1536, 100 + n_inst)
        bf = scene_brute_force(pkg, rays, meshes, inst, root_boxes(pkg, blases))
        assert bf["hit"].sum() > len(rays) // 10
        closest, anyhit = scene.intersect(rays, "closest"), scene.intersect(rays, "any")
        check_exact(pkg, rays, meshes, inst, bf, closest, anyhit, f"{n_inst} instances")
        if n_inst >= 3:
            hit_inst = set(closest["instance"][closest["prim"] != pkg.INVALID].tolist())
            assert not hit_inst & ({n_inst - 1, n_inst - 2, n_inst - 3} if n_inst > 3 else {n_inst - 1}), "an inactive instance was hit"
        t = scene.tlas()
        assert t.n_leaves == n_inst and (t.d_nodes is None) == (n_inst == 1)
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_independent_of_builders(pkg):
    rng = np.random.default_rng(9)
    mesh = no_negzero(pkg.meshgen.uniform(200, 77))
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(algo, mesh) for algo in range(4)]
        inst = scene_instances(pkg, rng, 64, 1, 1.2)
        rays = make_rays(pkg, world_tris(pkg, [mesh], inst), 1536, 5)
        outs = []
        for tl in range(4):                                   # top-level builders over the same BLAS
            outs.append(pkg.Scene(sc_ctx).build(tl, [blases[3]], inst).intersect(rays, "closest"))
        for b in range(3):                                    # BLAS builders of the same mesh
            outs.append(pkg.Scene(sc_ctx).build(3, [blases[b]], inst).intersect(rays, "closest"))
        assert (outs[0]["prim"] != pkg.INVALID).sum() > 100
        for o in outs[1:]:
            assert o.tobytes() == outs[0].tobytes()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("algo", [1, 3])
def test_one_identity_instance_equals_intersect(pkg, algo):
    mesh = no_negzero(pkg.meshgen.sponza_like(20_000, 3))
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        b = bl.add(algo, mesh)
        rays = make_rays(pkg, mesh, 4096, 8)
        ref = b.intersect(rays, "closest")
        got = pkg.Scene(sc_ctx).build(3, [b], make_instances(pkg, [identity()], [0])).intersect(rays, "closest")
        for f in ("t", "u", "v", "prim"):
            bad = np.nonzero(got[f].view(np.uint32) != ref[f].view(np.uint32))[0]
            assert bad.size == 0, f"{f} differs on {bad.size} rays, e.g. {bad[:4]}: scene {got[bad[:4]]} intersect {ref[bad[:4]]} rays {rays[bad[:4]]}"
        hit = ref["prim"] != pkg.INVALID
        assert hit.sum() > 500 and (got["instance"][hit] == 0).all() and (got["instance"][~hit] == pkg.INVALID).all()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("H", [70, 250])
def test_deep_blas_takes_the_stackless_pass(pkg, H):
    tris, nodes, root, n = caterpillar(pkg, H, 3 + H)
    c = pkg.Context(0)
    sc_ctx = pkg.Context(0)
    try:
        d_nodes, d_tris = c.upload(nodes), c.upload(tris)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
        offs = [(0, 0), (100, 0), (0, 100), (100, 100), (200, 50)]
        inst = make_instances(pkg, [mat34(np.eye(3), (x, y, 0.0)) for x, y in offs], [0] * len(offs))
        scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
        rng = np.random.default_rng(H)
        m = 500
        rays = np.zeros(m, dtype=pkg.RAY)
        base = np.array(offs, dtype=np.float64)[rng.integers(0, len(offs), m)]
        rays["origin"] = np.stack([base[:, 0] + rng.uniform(-1, 1, m), base[:, 1] + rng.uniform(-1, 1, m), np.full(m, -1.0)], axis=1)
        rays["direction"] = np.stack([rng.normal(0, 1e-3, m), rng.normal(0, 1e-3, m), np.ones(m)], axis=1)
        rays["direction"][: m // 4, :2] = 0.0
        rays["tmax"] = 1e30
        rays["tmin"][m // 2:] = rng.uniform(0, 1000 + 2 * H, m - m // 2)
        bf = scene_brute_force(pkg, rays, [tris], inst)
        assert bf["well"].all()
        closest, anyhit = scene.intersect(rays, "closest"), scene.intersect(rays, "any")
        # the stackless pass did the work: k_scene_intersect_deep is launched on every call and returns at once while no ray overflowed, so its time on
        # these rays is compared with its time on the same rays moved off every instance (nothing overflows: an idle launch)
        away = rays.copy(); away["origin"][:, 0] += 1.0e4

        def deep_ms(r):
            sc_ctx.set_profiling(2)
            for _ in range(5):
                scene.intersect(r, "closest")
            kt = sc_ctx.kernel_times()
            sc_ctx.set_profiling(0)
            return kt["k_scene_intersect_deep"][0]
        busy, idle = deep_ms(rays), deep_ms(away)
        assert busy > 4.0 * idle, f"k_scene_intersect_deep {busy:.4f} ms on the caterpillar rays vs {idle:.4f} ms idle: no ray took the stackless pass"
        assert closest.tobytes() == bf["closest"].tobytes()
        assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"]).all() and scene_recompute(pkg, rays, [tris], inst, anyhit).all()
        scene.close(); d_nodes.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()


def test_update_after_moves_and_blas_refit(pkg):
    rng = np.random.default_rng(21)
    meshes = [no_negzero(pkg.meshgen.uniform(n, 5 + n)) for n in (150, 120)]
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        inst = scene_instances(pkg, rng, 64, 2, 1.5)
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        moved = scene_instances(pkg, np.random.default_rng(22), 64, 2, 1.7)
        moved["blas"][:8] = 1 - np.minimum(moved["blas"][:8], 1)      # (the blas field changes too)
        scene.update(moved)
        rays = make_rays(pkg, world_tris(pkg, meshes, moved), 1536, 23)
        bf = scene_brute_force(pkg, rays, meshes, moved, root_boxes(pkg, blases))
        closest, anyhit = scene.intersect(rays, "closest"), scene.intersect(rays, "any")
        check_exact(pkg, rays, meshes, moved, bf, closest, anyhit, "after update")
        fresh = pkg.Scene(sc_ctx).build(3, blases, moved).intersect(rays, "closest")
        assert fresh.tobytes() == closest.tobytes()
        # refit a BLAS with jittered vertices, then update with the same instances
        m0 = jitter(meshes[0], 3, 2e-2)
        blases[0].refit(m0)
        bl.ctxs[0].synchronize()                              # (the refit ran on the BLAS's own stream: complete before the scene reads the root box)
        scene.update(moved)
        meshes2 = [m0, meshes[1]]
        bf2 = scene_brute_force(pkg, rays, meshes2, moved, root_boxes(pkg, blases))
        check_exact(pkg, rays, meshes2, moved, bf2, scene.intersect(rays, "closest"), scene.intersect(rays, "any"), "after BLAS refit")
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("tlas_algo", [0, 1, 2, 3])
def test_coincident_instances_tie_to_the_lower_index(pkg, tlas_algo):
    """two instances place the same triangles identically, so every hit ties on t; one BLAS also holds a far-off extra triangle that stretches its world box
    towards the rays, so its instance is entered first.  The lower instance index must win whichever that is."""
    mesh = no_negzero(pkg.meshgen.uniform(120, 12))
    v = np.concatenate([mesh["v1"], mesh["v2"], mesh["v3"]])
    lo, hi = v.min(axis=0), v.max(axis=0)
    extra = np.zeros(1, dtype=pkg.meshgen.TRIANGLE)                   # (appended: the prim indices of the shared triangles are the same in both BLASes)
    extra["v1"] = (hi[0] + 50, lo[1], lo[2] - 5); extra["v2"] = (hi[0] + 51, lo[1], lo[2] - 5); extra["v3"] = (hi[0] + 50, lo[1] + 1, lo[2] - 5)
    stretched = no_negzero(np.concatenate([mesh, extra]))
    rng = np.random.default_rng(tlas_algo)
    m = 1024
    rays = np.zeros(m, dtype=pkg.RAY)
    rays["origin"] = np.stack([rng.uniform(lo[0], hi[0], m), rng.uniform(lo[1], hi[1], m), np.full(m, lo[2] - 10.0)], axis=1)
    rays["direction"] = np.stack([rng.normal(0, 0.05, m), rng.normal(0, 0.05, m), np.ones(m)], axis=1)
    rays["tmax"] = 1e30
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        plain, far = bl.add(3, mesh), bl.add(1, stretched)
        for order in ((plain, far), (far, plain)):                      # the stretched instance is entered first: it is instance 1, then instance 0
            blas_tris = [mesh, stretched] if order[0] is plain else [stretched, mesh]
            inst = make_instances(pkg, [identity(), identity()], [0, 1])
            got = pkg.Scene(sc_ctx).build(tlas_algo, list(order), inst).intersect(rays, "closest")
            bf = scene_brute_force(pkg, rays, blas_tris, inst, root_boxes(pkg, list(order)))
            hit = got["prim"] != pkg.INVALID
            assert hit.sum() > m // 8, hit.sum()
            assert (got["instance"][hit] == 0).all(), f"stretched BLAS at index {1 if order[0] is plain else 0}: {np.count_nonzero(got['instance'][hit])} ties went to instance 1"
            assert bf["well"].mean() >= 0.99
            assert got[bf["well"]].tobytes() == bf["closest"][bf["well"]].tobytes()
    finally:
        bl.close(); sc_ctx.close()


def test_rejections_and_hygiene(pkg):
    mesh = no_negzero(pkg.meshgen.uniform(100, 3))
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    L = pkg.lib()
    try:
        own = pkg.HPLOC().build(sc_ctx, mesh)                 # a BLAS in the scene ctx's arena: rejected
        inst = make_instances(pkg, [identity(), mat34(np.eye(3), (2.0, 0, 0))], [0, 0])
        with pytest.raises(pkg.BvhError, match="-10001"):
            pkg.Scene(sc_ctx).build(3, [own], inst)
        b = bl.add(3, mesh)
        scene = pkg.Scene(sc_ctx)
        rays = make_rays(pkg, mesh, 256, 4)
        d_rays = sc_ctx.upload(rays)
        pad = 32
        hits = sc_ctx.alloc((len(rays) + 2 * pad) * 32)
        pattern = np.full((len(rays) + 2 * pad) * 32, 0xAB, dtype=np.uint8)
        hits.upload(pattern)
        h = hits.ptr + pad * 32
        assert L.bvh_scene_intersect(scene.handle, d_rays.ptr, len(rays), h, 0) == E_INVALID          # not built
        scene.build(2, [b], inst)
        assert L.bvh_scene_intersect(scene.handle, d_rays.ptr, len(rays), h, 2) == E_INVALID          # query kind
        assert L.bvh_scene_intersect(scene.handle, None, len(rays), h, 0) == E_INVALID
        assert L.bvh_scene_intersect(scene.handle, d_rays.ptr, len(rays), d_rays.ptr + 64, 0) == E_INVALID   # overlapping
        assert L.bvh_scene_intersect(scene.handle, d_rays.ptr, 0, h, 0) == 0
        sc_ctx.synchronize()
        assert np.array_equal(hits.download(np.uint8, pattern.size), pattern), "an error or n_rays == 0 wrote to the hits"
        assert L.bvh_scene_intersect(scene.handle, d_rays.ptr, len(rays), h, 0) == 0
        sc_ctx.synchronize()
        got = hits.download(np.uint8, pattern.size)
        assert np.array_equal(got[: pad * 32], pattern[: pad * 32]) and np.array_equal(got[-pad * 32:], pattern[-pad * 32:])
        # the top-level tree reads as any tree
        t = scene.tlas()
        assert t.n_leaves == 2 and t.layout == 1 and t.d_tris is None
        cost = C.c_double(); ck = C.c_uint64()
        assert L.bvh_sah_cost(sc_ctx.handle, C.byref(t), C.byref(cost)) == 0 and cost.value > 0
        assert L.bvh_checksum(sc_ctx.handle, C.byref(t), C.byref(ck)) == 0
        nodes = np.empty(1, dtype=pkg.BVH2_NODE); leaves = np.empty(2, dtype=pkg.PRIMREF)
        assert L.bvh_download(sc_ctx.handle, C.byref(t), nodes.ctypes.data, leaves.ctypes.data, None, None, None) == 0
        assert ck.value == pkg.checksum_host(nodes, leaves, t.root)
        assert sorted(leaves["prim"].tolist()) == [0, 1]
        scene.close(); d_rays.free(); hits.free()
    finally:
        bl.close(); sc_ctx.close()
