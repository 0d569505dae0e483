"""CPU: bvh_scene_intersect_all in the C ABI, the library and the Python binding; the numpy two-level brute force (every ray against every triangle of every
active instance in object space, ALL accepted hits per ray in ascending (t, instance, prim) order, compressed-row form), the checker the GPU tests
(tests/test_gpu_scene_multihit.py) use, and the inputs of those tests with the share of well-conditioned rays on them."""
import ctypes as C
import re

import numpy as np
import pytest

from test_gpu_query import caterpillar, make_rays
from test_gpu_refit import jitter, no_negzero
from test_gpu_scene import MESH_SIZES, scene_instances, world_tris
from test_multihit import HITS_SORTED, all_hits_brute_force, slice_rays
from test_query import E_INVALID, F32, QUERY_GROW, accepted, ray_ok, tri_formula, tri_vertices
from test_scene import header_text, identity, instance_inverse, make_instances, mat34, object_rays, scene_brute_force, tris_root_box, world_box


def scene_all_hits_brute_force(pkg, rays, blas_tris, instances, root_boxes=None, chunk_elems=1 << 22):
    """every ray against every triangle of every active instance, in object space (test_scene.scene_brute_force's arithmetic).  Returns dict: offsets
    (u32[m + 1]) and hits (INSTANCE_HIT records; ray i's slice hits[offsets[i]:offsets[i + 1]] holds ALL its accepted hits in ascending (t, instance, prim)
    order), n_acc (accepted hits per ray), well (bool: for EVERY accepted hit of the ray, the object-space point lies in its triangle's box grown by half the
    kernel's growth and the world point lies in its instance's world box grown likewise)."""
    n_blas = len(blas_tris)
    if root_boxes is None:
        root_boxes = [tris_root_box(t) for t in blas_tris]
    w, active = instance_inverse(instances["object_to_world"])
    active &= instances["blas"] < n_blas
    m = len(rays)
    ok = ray_ok(rays)
    bad = np.zeros(m, dtype=bool)
    found = []
    for k in np.nonzero(active)[0]:
        b = int(instances["blas"][k]); tris = blas_tris[b]
        wb = world_box(instances["object_to_world"][k], root_boxes[b]).astype(np.float64)
        g = 0.5 * QUERY_GROW * np.abs(wb).max()
        wlo, whi = wb[:3] - g, wb[3:] + g
        orays = object_rays(rays, w[k])
        v0, v1, v2 = tri_vertices(tris)
        lo = np.minimum(np.minimum(v0, v1), v2).astype(np.float64); hi = np.maximum(np.maximum(v0, v1), v2).astype(np.float64)
        gt = 0.5 * QUERY_GROW * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True)
        step = max(1, chunk_elems // max(len(tris), 1))
        for s in range(0, m, step):
            r = orays[s:s + step]; rw = rays[s:s + step]
            it, iu, iv, iw = tri_formula(r["origin"].astype(F32)[:, None, :], r["direction"].astype(F32)[:, None, :], v0[None], v1[None], v2[None])
            acc = accepted(it, iu, iv, iw, r["tmin"][:, None], r["tmax"][:, None]) & ok[s:s + step, None]
            ri, pi = np.nonzero(acc)
            if not ri.size:
                continue
            t = it[ri, pi]
            found.append((ri + s, np.full(len(ri), k, dtype=np.int64), pi, t, iu[ri, pi], iv[ri, pi]))
            po = r["origin"][ri].astype(np.float64) + t.astype(np.float64)[:, None] * r["direction"][ri].astype(np.float64)
            pw = rw["origin"][ri].astype(np.float64) + t.astype(np.float64)[:, None] * rw["direction"][ri].astype(np.float64)
            inside = ((po >= lo[pi] - gt[pi]) & (po <= hi[pi] + gt[pi])).all(axis=1) & ((pw >= wlo) & (pw <= whi)).all(axis=1)
            np.logical_or.at(bad, ri + s, ~inside)
    if found:
        ri, ki, pi, t, u, v = (np.concatenate([f[j] for f in found]) for j in range(6))
    else:
        ri = ki = pi = np.zeros(0, dtype=np.int64); t = u = v = np.zeros(0, dtype=F32)
    order = np.lexsort((pi, ki, t, ri))                               # by ray, then t, then instance, then prim
    rec = np.zeros(len(ri), dtype=pkg.INSTANCE_HIT)
    rec["t"] = t[order]; rec["u"] = u[order]; rec["v"] = v[order]; rec["prim"] = pi[order]; rec["instance"] = ki[order]
    n_acc = np.bincount(ri, minlength=m).astype(np.int64)
    offsets = np.zeros(m + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(n_acc)
    return {"offsets": offsets, "hits": rec, "n_acc": n_acc, "well": ~bad}


def scene_host_sort(offsets, hits):
    """every slice in ascending (t, instance, prim) order"""
    return hits[np.lexsort((hits["prim"], hits["instance"], hits["t"], slice_rays(offsets)))]


def _keys(offsets, hits, n_inst, n_max):
    return (slice_rays(offsets) * n_inst + hits["instance"].astype(np.int64)) * n_max + hits["prim"].astype(np.int64)


def check_scene_all_hits(pkg, rays, blas_tris, instances, ref, offsets, hits, sorted_, what=""):
    """the GPU tests' checker (test_multihit.check_all_hits for scenes).  Every ray: the offsets are a scan from 0 up to len(hits); each record names an active
    instance and a primitive of its BLAS and is an accepted hit of that pair with bit-equal t / u / v; the reserved words are 0; no (instance, prim) pair
    appears twice in a slice; each slice is a subset of the brute force's; a sorted answer is strictly ascending in (t, instance, prim).  Well-conditioned
    rays: the counts are equal (the offsets word for word up to the first ray that is not), a sorted fill is byte-equal to the brute force's slice and an
    unsorted one is after a host sort."""
    m, n_inst = len(rays), len(instances)
    off = offsets.astype(np.int64)
    assert len(off) == m + 1 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(hits), f"{what}: offsets are not a scan of the slices"
    assert hits.dtype == pkg.INSTANCE_HIT
    assert (hits["reserved"] == 0).all(), f"{what}: a reserved word is not 0"
    w, active = instance_inverse(instances["object_to_world"])
    active &= instances["blas"] < len(blas_tris)
    ray = slice_rays(offsets)
    inst, prim = hits["instance"].astype(np.int64), hits["prim"].astype(np.int64)
    assert (inst < n_inst).all(), f"{what}: an instance index out of range"
    assert active[inst].all(), f"{what}: {np.count_nonzero(~active[inst])} records name an inactive instance"
    sizes = np.array([len(t) for t in blas_tris], dtype=np.int64)
    assert (prim < sizes[instances["blas"][inst]]).all(), f"{what}: a primitive index out of range"
    good = np.zeros(len(hits), dtype=bool)
    for k in np.unique(inst):
        sel = np.nonzero(inst == k)[0]
        r = object_rays(rays[ray[sel]], w[k])
        v0, v1, v2 = tri_vertices(blas_tris[int(instances["blas"][k])][prim[sel]])
        it, iu, iv, iw = tri_formula(np.ascontiguousarray(r["origin"], dtype=F32), np.ascontiguousarray(r["direction"], dtype=F32), v0, v1, v2)
        acc = accepted(it, iu, iv, iw, r["tmin"], r["tmax"]) & ray_ok(rays[ray[sel]])
        h = hits[sel]
        good[sel] = acc & (it.view(np.uint32) == h["t"].view(np.uint32)) & (iu.view(np.uint32) == h["u"].view(np.uint32)) & \
            (iv.view(np.uint32) == h["v"].view(np.uint32))
    assert good.all(), f"{what}: {np.count_nonzero(~good)} records are not accepted hits of their (instance, prim) with bit-equal t / u / v"
    n_max = int(sizes.max())
    key = _keys(offsets, hits, n_inst, n_max)
    assert len(np.unique(key)) == len(key), f"{what}: an (instance, prim) pair appears twice in a slice"
    assert np.isin(key, _keys(ref["offsets"], ref["hits"], n_inst, n_max)).all(), f"{what}: a slice is not a subset of the true set"
    if sorted_ and len(hits) > 1:
        nxt = ray[1:] == ray[:-1]
        t, k, p = hits["t"], hits["instance"], hits["prim"]
        asc = (t[1:] > t[:-1]) | ((t[1:] == t[:-1]) & ((k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (p[1:] > p[:-1]))))
        assert asc[nxt].all(), f"{what}: {np.count_nonzero(~asc & nxt)} slices are not strictly ascending in (t, instance, prim)"
    well = ref["well"]
    counts, ref_counts = np.diff(off), np.diff(ref["offsets"].astype(np.int64))
    assert (counts == ref_counts)[well].all(), f"{what}: counts differ on {np.count_nonzero((counts != ref_counts) & well)} well-conditioned rays"
    first_bad = m if well.all() else int(np.argmin(well))
    assert offsets[: first_bad + 1].tobytes() == ref["offsets"][: first_bad + 1].tobytes(), f"{what}: offsets differ"
    got = hits if sorted_ else scene_host_sort(offsets, hits)
    mine, theirs = got[well[ray]], ref["hits"][well[slice_rays(ref["offsets"])]]
    assert mine.tobytes() == theirs.tobytes(), f"{what}: the {'sorted' if sorted_ else 'host-sorted'} slices of the well-conditioned rays differ from the brute force"


# ---- the GPU tests' inputs (tests/test_gpu_scene_multihit.py), made here so that their premises are checked without a device --------------------------------
EXACT_N_INST = [1, 2, 3, 64]


def exact_inputs(pkg, n_inst):
    """test_gpu_scene.test_exact_against_brute_force's recipe: four meshes, n_inst instances of every kind (with the inactive ones), 1536 mixed rays"""
    meshes = [no_negzero(pkg.meshgen.uniform(n, 31 + n)) for n in MESH_SIZES[n_inst]]
    inst = scene_instances(pkg, np.random.default_rng(n_inst), n_inst, 4, 1.5)
    return meshes, inst, make_rays(pkg, world_tris(pkg, meshes, inst), 1536, 100 + n_inst)


def inactive_of(n_inst):
    return set() if n_inst < 3 else {n_inst - 1} if n_inst == 3 else {n_inst - 1, n_inst - 2, n_inst - 3}


QUAD_LAYERS, QUAD_COPIES = 100, 3


def quad_inputs(pkg):
    """the minimal BLAS (one quad, n = 2: the root's children are both leaves) placed 300 times: instance k at z = k % 100, so k, k + 100 and k + 200
    coincide; 256 rays along +z through the quad's interior, away from its diagonal and its edges, half of them exactly axial"""
    quad = np.zeros(2, dtype=pkg.meshgen.TRIANGLE)
    quad["v1"][0] = (0, 0, 0); quad["v2"][0] = (1, 0, 0); quad["v3"][0] = (1, 1, 0)
    quad["v1"][1] = (0, 0, 0); quad["v2"][1] = (1, 1, 0); quad["v3"][1] = (0, 1, 0)
    n_inst = QUAD_LAYERS * QUAD_COPIES
    inst = make_instances(pkg, [mat34(np.eye(3), (0.0, 0.0, float(k % QUAD_LAYERS))) for k in range(n_inst)], [0] * n_inst)
    rng = np.random.default_rng(300)
    m = 256
    x = rng.uniform(0.15, 0.85, m)
    y = np.where(rng.random(m) < 0.5, x + rng.uniform(0.06, 0.12, m), x - rng.uniform(0.06, 0.12, m))
    rays = np.zeros(m, dtype=pkg.RAY)
    rays["origin"] = np.stack([x, y, np.full(m, -1.0)], axis=1)
    rays["direction"] = np.stack([rng.normal(0, 1e-5, m), rng.normal(0, 1e-5, m), np.ones(m)], axis=1)
    rays["direction"][: m // 2, :2] = 0.0
    rays["tmax"] = 1e30
    return quad, inst, rays


DEEP_OFFSETS = [(0, 0), (100, 0), (0, 100)]


def deep_inputs(pkg, H):
    """test_gpu_query.caterpillar of height H under 3 translated instances, rays along +z at the instances (test_gpu_scene's deep rays)"""
    tris, nodes, root, n = caterpillar(pkg, H, 3 + H)
    inst = make_instances(pkg, [mat34(np.eye(3), (x, y, 0.0)) for x, y in DEEP_OFFSETS], [0] * len(DEEP_OFFSETS))
    rng = np.random.default_rng(H)
    m = 384
    rays = np.zeros(m, dtype=pkg.RAY)
    base = np.array(DEEP_OFFSETS, dtype=np.float64)[rng.integers(0, len(DEEP_OFFSETS), m)]
    rays["origin"] = np.stack([base[:, 0] + rng.uniform(-1, 1, m), base[:, 1] + rng.uniform(-1, 1, m), np.full(m, -1.0)], axis=1)
    rays["direction"] = np.stack([rng.normal(0, 1e-3, m), rng.normal(0, 1e-3, m), np.ones(m)], axis=1)
    rays["direction"][: m // 4, :2] = 0.0
    rays["tmax"] = 1e30
    rays["tmin"][m // 2:] = rng.uniform(0, 1000 + 2 * H, m - m // 2)
    return tris, nodes, root, n, inst, rays


def moved_inputs(pkg):
    """test_gpu_scene.test_update_after_moves_and_blas_refit's recipe: two meshes, 64 instances as built and as moved, the first mesh jittered for the refit"""
    meshes = [no_negzero(pkg.meshgen.uniform(n, 5 + n)) for n in (150, 120)]
    inst = scene_instances(pkg, np.random.default_rng(21), 64, 2, 1.5)
    moved = scene_instances(pkg, np.random.default_rng(22), 64, 2, 1.7)
    moved["blas"][:8] = 1 - np.minimum(moved["blas"][:8], 1)
    rays = make_rays(pkg, world_tris(pkg, meshes, moved), 1536, 23)
    return meshes, inst, moved, rays, jitter(meshes[0], 3, 2e-2)


def builders_inputs(pkg):
    mesh = no_negzero(pkg.meshgen.uniform(200, 77))
    inst = scene_instances(pkg, np.random.default_rng(9), 64, 1, 1.2)
    return mesh, inst, make_rays(pkg, world_tris(pkg, [mesh], inst), 1536, 5)


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_scene_intersect_all():
    text = header_text()
    assert re.search(r"\bint\s+bvh_scene_intersect_all\s*\(\s*bvh_scene\s*\*\s*\w+\s*,\s*const bvh_ray\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*"
                     r"uint32_t\s*\*\s*\w+\s*,\s*bvh_instance_hit\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"#define\s+BVH_HITS_SORTED\s+1u", text) and "#define BVH_ABI_VERSION 4" in text


def test_library_exports_scene_intersect_all(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "bvh_scene_intersect_all") and "bvh_scene_intersect_all" in pkg.EXPORTS
    assert pkg.lib().bvh_abi_version() == 4 and pkg.INSTANCE_HIT.itemsize == 32 and pkg.HITS_SORTED == HITS_SORTED
    assert callable(getattr(pkg.Scene, "intersect_all"))


def test_scene_intersect_all_errors_without_a_device(pkg):
    """a NULL scene is refused before any device call, whatever else is passed"""
    L = pkg.lib()
    tot = C.c_uint64(0x77)
    assert L.bvh_scene_intersect_all(None, None, 0, 0, None, None, 0, None) == E_INVALID
    assert L.bvh_scene_intersect_all(None, 256, 4, HITS_SORTED, 4096, 8192, 16, C.byref(tot)) == E_INVALID
    assert L.bvh_scene_intersect_all(None, 256, 0, 0, 4096, None, 0, C.byref(tot)) == E_INVALID
    assert tot.value == 0x77


# ---- the brute force ------------------------------------------------------------------------------------------------------------------------------------------
def test_identity_instances_equal_the_flat_brute_force(pkg):
    """with identity instances the scene's records are test_multihit.all_hits_brute_force's on the concatenated triangles, record for record"""
    meshes = [pkg.meshgen.uniform(40, 1), pkg.meshgen.uniform(25, 2)]
    blas_of = [0, 1, 0]
    inst = make_instances(pkg, [identity()] * 3, blas_of)
    flat = np.concatenate([meshes[b] for b in blas_of])
    rays = make_rays(pkg, flat, 512, 3)
    got = scene_all_hits_brute_force(pkg, rays, meshes, inst, chunk_elems=1 << 12)
    ref = all_hits_brute_force(rays, flat)
    assert ref["offsets"][-1] > 200
    assert got["offsets"].tobytes() == ref["offsets"].tobytes() and (got["n_acc"] == ref["n_acc"]).all()
    starts = np.cumsum([0] + [len(meshes[b]) for b in blas_of])
    # (instances 0 and 2 place the same mesh: equal t there, and the flat order (t, flat prim) is then (t, instance, prim) too)
    g, r = got["hits"], ref["hits"]
    for f in ("t", "u", "v"):
        assert g[f].tobytes() == r[f].tobytes()
    assert np.array_equal(starts[g["instance"]] + g["prim"], r["prim"]) and (g["reserved"] == 0).all()
    assert (got["well"] == ref["well"]).all()                     # (the world box holds every triangle box under the identity)
    check_scene_all_hits(pkg, rays, meshes, inst, got, got["offsets"], got["hits"], True, "the brute force itself")


def _first_is_closest(pkg, rays, blas_tris, inst, ref, what):
    bf = scene_brute_force(pkg, rays, blas_tris, inst)
    has = ref["n_acc"] > 0
    assert (has == bf["hit"]).all(), f"{what}: empty slices and the closest-hit brute force's misses differ"
    assert ref["hits"][ref["offsets"][:-1][has]].tobytes() == bf["closest"][has].tobytes(), f"{what}: a slice's first record is not the closest hit"
    miss = bf["closest"][~has]
    assert (miss["prim"] == pkg.INVALID).all() and (miss["instance"] == pkg.INVALID).all() and miss["t"].tobytes() == rays["tmax"][~has].tobytes()
    assert (ref["well"] == bf["well"]).all()
    return bf


@pytest.mark.parametrize("n_inst", EXACT_N_INST)
def test_exact_inputs_are_well_conditioned(pkg, n_inst):
    meshes, inst, rays = exact_inputs(pkg, n_inst)
    ref = scene_all_hits_brute_force(pkg, rays, meshes, inst)
    share, hit = ref["well"].mean(), (ref["n_acc"] > 0).mean()
    print(f"n_inst {n_inst}: well-conditioned {share:.4f}, hit share {hit:.3f}, records {len(ref['hits'])}, most per ray {ref['n_acc'].max()}")
    assert share >= 0.99 and hit > 0.1
    _first_is_closest(pkg, rays, meshes, inst, ref, f"{n_inst} instances")
    assert not set(ref["hits"]["instance"].tolist()) & inactive_of(n_inst)
    check_scene_all_hits(pkg, rays, meshes, inst, ref, ref["offsets"], ref["hits"], True, f"{n_inst} instances")


def test_quad_inputs(pkg):
    """every ray crosses all 300 quads, three at each t, ordered by instance inside a triple"""
    quad, inst, rays = quad_inputs(pkg)
    ref = scene_all_hits_brute_force(pkg, rays, [quad], inst)
    assert ref["well"].all() and (ref["n_acc"] == QUAD_LAYERS * QUAD_COPIES).all()
    h = ref["hits"].reshape(len(rays), QUAD_LAYERS, QUAD_COPIES)
    assert (h["t"][:, :, 0] == h["t"][:, :, 1]).all() and (h["t"][:, :, 1] == h["t"][:, :, 2]).all() and (np.diff(h["t"][:, :, 0], axis=1) > 0).all()
    layer = np.arange(QUAD_LAYERS)[None, :, None]
    assert (h["instance"] == layer + QUAD_LAYERS * np.arange(QUAD_COPIES)[None, None, :]).all()
    assert (h["prim"] == h["prim"][:, :1, :1]).all() and set(np.unique(h["prim"]).tolist()) == {0, 1}
    _first_is_closest(pkg, rays, [quad], inst, ref, "quads")


@pytest.mark.parametrize("H", [70, 250])
def test_deep_inputs(pkg, H):
    tris, nodes, root, n, inst, rays = deep_inputs(pkg, H)
    ref = scene_all_hits_brute_force(pkg, rays, [tris], inst)
    assert ref["well"].all() and ref["n_acc"].max() == n and (ref["n_acc"][: len(rays) // 2] == n).all()
    assert len(set(ref["hits"]["instance"].tolist())) == len(DEEP_OFFSETS)
    _first_is_closest(pkg, rays, [tris], inst, ref, f"caterpillar {H}")


def test_moved_and_builders_inputs_are_well_conditioned(pkg):
    meshes, inst, moved, rays, m0 = moved_inputs(pkg)
    for what, ms in (("moved", meshes), ("refit", [m0, meshes[1]])):
        ref = scene_all_hits_brute_force(pkg, rays, ms, moved)
        assert ref["well"].mean() >= 0.99 and (ref["n_acc"] > 0).mean() > 0.1, what
        _first_is_closest(pkg, rays, ms, moved, ref, what)
    mesh, binst, brays = builders_inputs(pkg)
    ref = scene_all_hits_brute_force(pkg, brays, [mesh], binst)
    assert ref["well"].mean() >= 0.99 and (ref["n_acc"] > 0).sum() > 100
    _first_is_closest(pkg, brays, [mesh], binst, ref, "builders")


# ---- the checker ----------------------------------------------------------------------------------------------------------------------------------------------
def test_checker_catches_tampered_slices(pkg):
    """six instances of two small meshes: 0 and 3 coincide (ties on t between instances), 4 is inactive (blas out of range) but placed like 0"""
    meshes = [pkg.meshgen.uniform(60, 6), pkg.meshgen.uniform(40, 7)]
    mats = [identity(), mat34(np.eye(3), (0.3, 0.0, 0.1)), mat34(np.diag([1.0, -1.0, 1.0]), (0.0, 1.0, 0.2)), identity(), identity(), mat34(np.eye(3) * 0.5, (0.2, 0.2, 0.2))]
    inst = make_instances(pkg, mats, [0, 1, 0, 0, 9, 1])
    rng = np.random.default_rng(8)
    m = 96
    rays = np.zeros(m, dtype=pkg.RAY)
    o = rng.uniform(-0.5, 1.5, (m, 3)); d = rng.uniform(0, 1, (m, 3)) - o
    rays["origin"] = o.astype(F32); rays["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32); rays["tmax"] = 1e30
    ref = scene_all_hits_brute_force(pkg, rays, meshes, inst)
    off, hits = ref["offsets"], ref["hits"]
    assert ref["well"].all() and 4 not in set(hits["instance"].tolist()) and {0, 1, 2, 3, 5} <= set(hits["instance"].tolist())

    def check(o, h, flag):
        check_scene_all_hits(pkg, rays, meshes, inst, ref, o, h, flag)

    def caught(o, h, flags=(True, False)):
        for flag in flags:
            with pytest.raises(AssertionError):
                check(o, h, flag)
    check(off, hits, True)
    shuffled = hits.copy()
    for i in range(m):
        s = shuffled[off[i]:off[i + 1]]; s[:] = s[rng.permutation(len(s))]
    check(off, shuffled, False)                                       # an unsorted answer is fine unsorted ...
    caught(off, shuffled, (True,))                                    # ... and caught when it claims to be sorted
    i = int(np.argmax(np.diff(off.astype(np.int64)) >= 6)); a = int(off[i])
    assert off[i + 1] - off[i] >= 6
    ray = slice_rays(off)
    dropped = np.delete(hits, a + 2); off2 = off.copy(); off2[i + 1:] -= 1
    caught(off2, dropped)                                             # a dropped record
    distinct = np.nonzero((ray[1:] == ray[:-1]) & (hits["t"][1:] > hits["t"][:-1]))[0][0]
    swapped = hits.copy(); swapped[[distinct, distinct + 1]] = swapped[[distinct + 1, distinct]]
    caught(off, swapped, (True,))                                     # two swapped records
    tie = np.nonzero((ray[1:] == ray[:-1]) & (hits["t"][1:] == hits["t"][:-1]))[0][0]
    assert hits["instance"][tie] == 0 and hits["instance"][tie + 1] == 3 and hits["prim"][tie] == hits["prim"][tie + 1]
    tied = hits.copy(); tied[[tie, tie + 1]] = tied[[tie + 1, tie]]
    caught(off, tied, (True,))                                        # equal t, instances in the wrong order
    check(off, tied, False)
    dup = hits.copy(); dup[a + 3] = dup[a + 2]
    caught(off, dup)                                                  # a duplicate
    wrong = hits.copy(); wrong["instance"][tie] = 1                   # a wrong (active) instance index
    caught(off, wrong)
    twin = hits.copy(); twin["instance"][tie] = 3                     # ... even the coincident twin's: the pair then appears twice
    caught(off, twin)
    inactive = hits.copy(); inactive["instance"][tie] = 4             # an inactive instance's index (placed like instance 0: t / u / v would agree)
    caught(off, inactive)
    res = hits.copy(); res["reserved"][a + 1, 2] = 1                  # a non-zero reserved word
    caught(off, res)
    bit = hits.copy(); bit["t"].view(np.uint32)[a + 4] ^= 1
    caught(off, bit)
    off3 = off.copy(); off3[i + 1] += 1                               # ray i + 1's first record handed to ray i
    assert off[i + 2] > off[i + 1]
    caught(off3, hits, (True,))
