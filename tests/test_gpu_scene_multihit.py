"""bvh_scene_intersect_all on the GPU: every accepted hit of every ray over all active instances against the two-level numpy brute force
(tests/test_scene_multihit.py, which also checks these inputs on the CPU): sorted, unsorted and count-only calls over BLASes of every builder and format,
the minimal BLAS under 300 partly coincident instances, one identity instance against bvh_intersect_all, consistency with the scene's closest hit,
independence from the builders, deep BLASes through the stackless pass, the passes and the capacity decision, answers after moves and a BLAS refit, errors."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_multihit import chain_left, left_first_stack
from test_gpu_query import make_rays
from test_gpu_refit import no_negzero
from test_gpu_scene import TLAS_ALGO, Blases, root_boxes
from test_multihit import HITS_SORTED, slice_rays
from test_query import E_INVALID
from test_scene import identity, make_instances, mat34
from test_scene_multihit import (EXACT_N_INST, QUAD_COPIES, QUAD_LAYERS, builders_inputs, check_scene_all_hits, deep_inputs, exact_inputs, inactive_of,
                                 moved_inputs, quad_inputs, scene_all_hits_brute_force)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]
F32 = np.float32
QUERY_STACK = 64                                                  # query.hpp: short-stack entries per lane
_EXACT = {}


def call(pkg, scene, d_rays, m, flags, d_offsets, d_hits, capacity, total=True):
    t = C.c_uint64(0xDEAD)
    rc = pkg.lib().bvh_scene_intersect_all(scene.handle, d_rays, m, flags, d_offsets, d_hits, capacity, C.byref(t) if total else None)
    return rc, t.value


def all_hits(pkg, scene, rays, flags):
    """count-only call, then a fill with the exact capacity; returns (offsets, hits).  The count-only offsets must equal the fill's."""
    ctx, m = scene.ctx, len(rays)
    d_rays, d_off = ctx.upload(rays), ctx.alloc((m + 1) * 4)
    hits = None
    try:
        rc, total = call(pkg, scene, d_rays.ptr, m, flags, d_off.ptr, None, 0)
        assert rc == 0, rc
        counted = d_off.download(np.uint32, m + 1)
        assert counted[0] == 0 and counted[-1] == total
        hits = ctx.alloc(max(total, 1) * 32)
        rc, total2 = call(pkg, scene, d_rays.ptr, m, flags, d_off.ptr, hits.ptr, total)
        assert rc == 0 and total2 == total
        off = d_off.download(np.uint32, m + 1)
        assert off.tobytes() == counted.tobytes(), "count-only and fill calls disagree on the offsets"
        return off, hits.download(pkg.INSTANCE_HIT, total)
    finally:
        d_rays.free(); d_off.free()
        if hits is not None:
            hits.free()


class ExactScene:
    """test_gpu_scene.test_exact_against_brute_force's scene: the four BLAS builders in the three formats under TLAS_ALGO[n_inst]"""

    def __init__(self, pkg, n_inst):
        self.meshes, self.inst, self.rays = exact_inputs(pkg, n_inst)
        self.bl, self.ctx = Blases(pkg), pkg.Context(0)
        try:
            self.blases = [self.bl.add(algo, self.meshes[algo], fmt=algo % 3) for algo in range(4)]
            self.scene = pkg.Scene(self.ctx).build(TLAS_ALGO[n_inst], self.blases, self.inst)
            if n_inst not in _EXACT:                              # (the reference is computed once per recipe and shared, unchanged)
                _EXACT[n_inst] = scene_all_hits_brute_force(pkg, self.rays, self.meshes, self.inst, root_boxes(pkg, self.blases))
            self.ref = _EXACT[n_inst]
        except Exception:
            self.close()
            raise

    def close(self):
        self.bl.close(); self.ctx.close()


@pytest.mark.parametrize("n_inst", EXACT_N_INST)
def test_exact_against_brute_force(pkg, n_inst):
    """1: no top-level tree; 2: a root with two leaf children; 3: the singular instance inactive; 64: all three kinds of inactive instance"""
    s = ExactScene(pkg, n_inst)
    try:
        ref, what = s.ref, f"{n_inst} instances"
        assert ref["well"].mean() >= 0.99 and (ref["n_acc"] > 0).sum() > len(s.rays) // 10
        off, hits = all_hits(pkg, s.scene, s.rays, HITS_SORTED)
        check_scene_all_hits(pkg, s.rays, s.meshes, s.inst, ref, off, hits, True, what + " sorted")
        uoff, uhits = all_hits(pkg, s.scene, s.rays, 0)
        assert uoff.tobytes() == off.tobytes(), f"{what}: sorted and unsorted calls count differently"
        check_scene_all_hits(pkg, s.rays, s.meshes, s.inst, ref, uoff, uhits, False, what + " unsorted")
        assert not (set(hits["instance"].tolist()) | set(uhits["instance"].tolist())) & inactive_of(n_inst), "an inactive instance answered"
        poff, phits = s.scene.intersect_all(s.rays, sorted=True)          # the Python binding, host rays
        assert poff.tobytes() == off.tobytes() and phits.tobytes() == hits.tobytes()
        assert s.scene.intersect_all(s.rays, count_only=True).tobytes() == off.tobytes()
        qoff, qhits = s.scene.intersect_all(s.rays, sorted=False, capacity=3)   # a capacity that is too small is re-allocated
        assert qoff.tobytes() == off.tobytes() and qhits.tobytes() == uhits.tobytes()
        eoff, ehits = s.scene.intersect_all(s.rays[:0])
        assert eoff.tolist() == [0] and len(ehits) == 0 and ehits.dtype == pkg.INSTANCE_HIT
    finally:
        s.close()


def test_minimal_blas_and_long_tied_slices(pkg):
    """a 2-triangle BLAS (the root's children are both leaves) placed 300 times, three coincident copies at each of 100 offsets: every ray has 300 hits, the
    three of a triple tie on t and are ordered by instance, and the sorted bytes are the brute force's under every top-level builder"""
    quad, inst, rays = quad_inputs(pkg)
    ref = scene_all_hits_brute_force(pkg, rays, [quad], inst)
    n_hits = QUAD_LAYERS * QUAD_COPIES
    assert ref["well"].all() and (ref["n_acc"] == n_hits).all()
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(3, quad)
        assert b.result.n_leaves == 2
        for tl in range(4):
            scene = pkg.Scene(sc_ctx).build(tl, [b], inst)
            off, hits = all_hits(pkg, scene, rays, HITS_SORTED)
            assert off.tobytes() == ref["offsets"].tobytes() and hits.tobytes() == ref["hits"].tobytes(), f"top-level builder {tl}"
            h = hits.reshape(len(rays), QUAD_LAYERS, QUAD_COPIES)
            assert (h["t"][:, :, 0] == h["t"][:, :, 2]).all() and (np.diff(h["instance"].astype(np.int64), axis=2) == QUAD_LAYERS).all()
            uoff, uhits = all_hits(pkg, scene, rays, 0)
            check_scene_all_hits(pkg, rays, [quad], inst, ref, uoff, uhits, False, f"top-level builder {tl} unsorted")
            scene.close()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("algo", [1, 3])
def test_one_identity_instance_equals_intersect_all(pkg, algo):
    mesh = no_negzero(pkg.meshgen.sponza_like(20_000, 3))
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        b = bl.add(algo, mesh)
        rays = make_rays(pkg, mesh, 4096, 8)
        scene = pkg.Scene(sc_ctx).build(3, [b], make_instances(pkg, [identity()], [0]))
        for flag in (True, False):
            roff, rhits = b.intersect_all(rays, sorted=flag)
            off, hits = scene.intersect_all(rays, sorted=flag)
            assert len(rhits) > 2000 and off.tobytes() == roff.tobytes(), f"sorted {flag}: offsets differ"
            for f in ("t", "u", "v", "prim"):
                bad = np.nonzero(hits[f].view(np.uint32) != rhits[f].view(np.uint32))[0]
                assert bad.size == 0, f"sorted {flag}: {f} differs on {bad.size} records, e.g. {bad[:4]}: scene {hits[bad[:4]]} intersect_all {rhits[bad[:4]]}"
            assert (hits["instance"] == 0).all() and (hits["reserved"] == 0).all()
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("n_inst", [1, 64])
def test_consistent_with_the_closest_hit(pkg, n_inst):
    s = ExactScene(pkg, n_inst)
    try:
        well = s.ref["well"]
        closest = s.scene.intersect(s.rays, "closest")
        off, hits = s.scene.intersect_all(s.rays, sorted=True)
        empty = np.diff(off.astype(np.int64)) == 0
        assert (empty == (closest["prim"] == pkg.INVALID))[well].all(), "empty slices and closest-hit misses differ"
        has = ~empty & well
        assert has.sum() > 100 and hits[off[:-1][has]].tobytes() == closest[has].tobytes(), "first sorted record != bvh_scene_intersect closest"
    finally:
        s.close()


def test_independent_of_builders(pkg):
    mesh, inst, rays = builders_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        outs = []
        hp = bl.add(3, mesh)
        for tl in range(4):                                       # top-level builders over the same BLAS
            scene = pkg.Scene(sc_ctx).build(tl, [hp], inst)
            outs.append((f"top-level builder {tl}", all_hits(pkg, scene, rays, HITS_SORTED)))
            scene.close()
        for algo in range(4):                                     # BLAS builders and formats of the same mesh
            for fmt in range(3):
                if algo == 3 and fmt == 0:
                    continue                                      # (the BLAS above)
                scene = pkg.Scene(sc_ctx).build(3, [bl.add(algo, mesh, fmt=fmt)], inst)
                outs.append((f"BLAS builder {algo} format {fmt}", all_hits(pkg, scene, rays, HITS_SORTED)))
                scene.close()
        off0, hits0 = outs[0][1]
        assert len(hits0) > 200 and len(outs) == 15
        for what, (off, hits) in outs[1:]:
            assert off.tobytes() == off0.tobytes() and hits.tobytes() == hits0.tobytes(), what
        ref = scene_all_hits_brute_force(pkg, rays, [mesh], inst, root_boxes(pkg, [hp]))
        check_scene_all_hits(pkg, rays, [mesh], inst, ref, off0, hits0, True, "builders")
    finally:
        bl.close(); sc_ctx.close()


@pytest.mark.parametrize("H", [70, 250])
def test_deep_blas_takes_the_stackless_pass(pkg, H):
    tris, nodes, root, n, inst, rays = deep_inputs(pkg, H)
    swapped = chain_left(nodes, n - 1)
    # rays[: m // 2] pass every box of the caterpillar (tmin 0, no tmax): the left-first walk's BLAS stack alone exceeds the short stack
    assert left_first_stack(swapped, root, n - 1) > QUERY_STACK
    ref = scene_all_hits_brute_force(pkg, rays, [tris], inst)
    assert ref["well"].all() and ref["n_acc"].max() == n
    c, sc_ctx = pkg.Context(0), pkg.Context(0)
    try:
        d_tris = c.upload(tris)
        for label, arr in (("as made", nodes), ("chain left", swapped)):
            d_nodes = c.upload(arr)
            r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.d_tris = d_tris.ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 0
            scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(r, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
            sc_ctx.set_profiling(2)
            off, hits = all_hits(pkg, scene, rays, HITS_SORTED)           # (asserts that the count-only and the fill call agree)
            kt = sc_ctx.kernel_times()
            sc_ctx.set_profiling(0)
            assert {"k_scene_hits_count", "k_scene_hits_fill", "k_scene_hits_deep", "k_overlap_scan"} <= set(kt), sorted(kt)
            assert off.tobytes() == ref["offsets"].tobytes() and hits.tobytes() == ref["hits"].tobytes(), f"H {H} {label}"
            uoff, uhits = all_hits(pkg, scene, rays, 0)
            check_scene_all_hits(pkg, rays, [tris], inst, ref, uoff, uhits, False, f"H {H} {label} unsorted")
            scene.close(); d_nodes.free()
        d_tris.free()
    finally:
        sc_ctx.close(); c.close()


def test_passes_and_capacity(pkg):
    s = ExactScene(pkg, 64)
    try:
        ctx, scene, rays, m = s.ctx, s.scene, s.rays, len(s.rays)
        want = {flags: all_hits(pkg, scene, rays, flags) for flags in (HITS_SORTED, 0)}
        exp_off = want[0][0]
        total = int(exp_off[-1])
        assert total > 100 and want[HITS_SORTED][0].tobytes() == exp_off.tobytes() and exp_off.tobytes() == s.ref["offsets"].tobytes()
        extra = 29
        guard_h = np.frombuffer(np.full((total + extra) * 32, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_HIT)
        guard_o = np.full(m + 1 + extra, 0xA5A5A5A5, dtype=np.uint32)
        d_rays, d_off, d_hits = ctx.upload(rays), ctx.upload(guard_o), ctx.upload(guard_h)
        for flags in (HITS_SORTED, 0):
            out = {}
            # count only: d_hits untouched, offsets complete, guard words past n_rays + 1 offsets intact
            d_off.upload(guard_o); d_hits.upload(guard_h)
            assert call(pkg, scene, d_rays.ptr, m, flags, d_off.ptr, None, 0) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_hits.download(pkg.INSTANCE_HIT, total + extra).tobytes() == guard_h.tobytes()
            # capacity total - 1: the fill is skipped, d_offsets still complete, *total_out set
            d_off.upload(guard_o)
            assert call(pkg, scene, d_rays.ptr, m, flags, d_off.ptr, d_hits.ptr, total - 1) == (0, total)
            o = d_off.download(np.uint32, m + 1 + extra)
            assert o[: m + 1].tobytes() == exp_off.tobytes() and o[m + 1:].tobytes() == guard_o[m + 1:].tobytes()
            assert d_hits.download(pkg.INSTANCE_HIT, total + extra).tobytes() == guard_h.tobytes()
            # the exact capacity is filled; guard records past the total intact; twice the same bytes
            for rnd in range(2):
                d_off.upload(guard_o); d_hits.upload(guard_h)
                assert call(pkg, scene, d_rays.ptr, m, flags, d_off.ptr, d_hits.ptr, total) == (0, total)
                o, h = d_off.download(np.uint32, m + 1 + extra), d_hits.download(pkg.INSTANCE_HIT, total + extra)
                assert o[m + 1:].tobytes() == guard_o[m + 1:].tobytes() and h[total:].tobytes() == guard_h[total:].tobytes()
                assert o[: m + 1].tobytes() == exp_off.tobytes() and h[:total].tobytes() == want[flags][1].tobytes()
                out[rnd] = (o.tobytes(), h.tobytes())
            assert out[0] == out[1], "two identical calls give different bytes"
            # total_out == NULL: the same device bytes after a synchronize
            d_off.upload(guard_o); d_hits.upload(guard_h)
            rc, t = call(pkg, scene, d_rays.ptr, m, flags, d_off.ptr, d_hits.ptr, total + extra, total=False)
            assert rc == 0 and t == 0xDEAD
            ctx.synchronize()
            assert (d_off.download(np.uint32, m + 1 + extra).tobytes(), d_hits.download(pkg.INSTANCE_HIT, total + extra).tobytes()) == out[0]
            assert d_rays.download(pkg.RAY, m).tobytes() == rays.tobytes()
        # n_rays == 0: d_offsets[0] = 0, *total_out = 0, nothing else
        d_off.upload(guard_o); d_hits.upload(guard_h)
        assert call(pkg, scene, d_rays.ptr, 0, HITS_SORTED, d_off.ptr, d_hits.ptr, total) == (0, 0)
        o = d_off.download(np.uint32, m + 1 + extra)
        assert o[0] == 0 and o[1:].tobytes() == guard_o[1:].tobytes() and d_hits.download(pkg.INSTANCE_HIT, total + extra).tobytes() == guard_h.tobytes()
        d_rays.free(); d_off.free(); d_hits.free()
    finally:
        s.close()


def test_after_moves_and_blas_refit(pkg):
    meshes, inst, moved, rays, m0 = moved_inputs(pkg)
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1], fmt=pkg.TRI_PACKED36)]
        scene = pkg.Scene(sc_ctx).build(3, blases, inst)
        scene.intersect_all(rays, count_only=True)
        scene.update(moved)
        ref = scene_all_hits_brute_force(pkg, rays, meshes, moved, root_boxes(pkg, blases))
        assert ref["well"].mean() >= 0.99
        off, hits = scene.intersect_all(rays)
        check_scene_all_hits(pkg, rays, meshes, moved, ref, off, hits, True, "after update")
        uoff, uhits = scene.intersect_all(rays, sorted=False)
        check_scene_all_hits(pkg, rays, meshes, moved, ref, uoff, uhits, False, "after update, unsorted")
        foff, fhits = pkg.Scene(sc_ctx).build(3, blases, moved).intersect_all(rays)
        assert foff.tobytes() == off.tobytes() and fhits.tobytes() == hits.tobytes(), "an updated and a freshly built scene differ"
        # refit a BLAS with jittered vertices, then update with the same instances
        blases[0].refit(m0)
        bl.ctxs[0].synchronize()                                  # (the refit ran on the BLAS's own stream: complete before the scene reads the root box)
        scene.update(moved)
        meshes2 = [m0, meshes[1]]
        ref2 = scene_all_hits_brute_force(pkg, rays, meshes2, moved, root_boxes(pkg, blases))
        assert ref2["well"].mean() >= 0.99
        off2, hits2 = scene.intersect_all(rays)
        check_scene_all_hits(pkg, rays, meshes2, moved, ref2, off2, hits2, True, "after BLAS refit")
        assert scene.intersect_all(rays, count_only=True).tobytes() == off2.tobytes()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_errors_write_nothing(pkg):
    mesh = no_negzero(pkg.meshgen.uniform(100, 3))
    bl, sc_ctx = Blases(pkg), pkg.Context(0)
    L = pkg.lib()
    try:
        b = bl.add(3, mesh)
        inst = make_instances(pkg, [identity(), mat34(np.eye(3), (2.0, 0, 0))], [0, 0])
        rays = make_rays(pkg, mesh, 256, 4)
        d_rays = sc_ctx.upload(rays)
        cap = 4096
        guard_h = np.frombuffer(np.full(cap * 32, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.INSTANCE_HIT)
        guard_o = np.full(257, 0x5A5A5A5A, dtype=np.uint32)
        hits, offs = sc_ctx.upload(guard_h), sc_ctx.upload(guard_o)
        tot = C.c_uint64(0x77)
        unbuilt, scene = pkg.Scene(sc_ctx), pkg.Scene(sc_ctx).build(2, [b], inst)

        def go(sc=scene, r=d_rays.ptr, m=256, flags=HITS_SORTED, o=offs.ptr, h=hits.ptr, k=cap):
            return L.bvh_scene_intersect_all(sc.handle if sc is not None else None, r, m, flags, o, h, k, C.byref(tot))
        cases = {
            "null scene": go(sc=None), "unbuilt scene": go(sc=unbuilt), "null rays": go(r=None), "null offsets": go(o=None),
            "flag 2": go(flags=2), "flag 3": go(flags=3), "flag high": go(flags=0x80000000),
            "n_rays 2^30": go(m=1 << 30),
            "offsets in rays": go(o=d_rays.ptr + 64), "hits in rays": go(h=d_rays.ptr + 32), "hits in offsets": go(h=offs.ptr + 32),
            "offsets in hits": go(o=hits.ptr + 32 * (cap - 1)), "rays in hits": go(r=hits.ptr, h=hits.ptr + 32 * 8),
            "unbuilt, n_rays 0": go(sc=unbuilt, m=0),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        assert tot.value == 0x77
        sc_ctx.synchronize()
        assert hits.download(pkg.INSTANCE_HIT, cap).tobytes() == guard_h.tobytes() and offs.download(np.uint32, 257).tobytes() == guard_o.tobytes()
        # a count-only call ignores the capacity's range, and the scene still answers
        assert go(h=None, k=1 << 40) == 0 and tot.value != 0x77
        total = tot.value
        assert offs.download(np.uint32, 257)[-1] == total and hits.download(pkg.INSTANCE_HIT, cap).tobytes() == guard_h.tobytes()
        assert 0 < total <= cap and go() == 0 and tot.value == total
        got = hits.download(pkg.INSTANCE_HIT, cap)
        assert got[total:].tobytes() == guard_h[total:].tobytes()
        ref = scene_all_hits_brute_force(pkg, rays, [mesh], inst, root_boxes(pkg, [b]))
        check_scene_all_hits(pkg, rays, [mesh], inst, ref, offs.download(np.uint32, 257), got[:total], True, "after the errors")
        scene.close(); unbuilt.close(); d_rays.free(); hits.free(); offs.free()
    finally:
        bl.close(); sc_ctx.close()
