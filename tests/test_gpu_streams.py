"""Caller-owned streams and concurrent contexts (include/bvh_mi355x.h: "calls on one ctx are serialised on its stream", "different ctxs are independent",
"asynchronous on the ctx's stream, no read-back"): a context created with bvh_ctx_create_on_stream on a torch stream gives the answers of the oracle / the
numpy brute forces; the library reads what the stream wrote last (a long torch delay and a device copy in front of the call, no host wait) and consumers
enqueued behind the call see its result after one synchronize; the calls the header declares asynchronous return while the delay is still running; four host
threads with a context each reproduce, byte for byte, what one context computed serially; four threads creating the process's first contexts at the same
moment (a fresh child process) all build correct trees.  torch is used for streams, events, tensors and the delay only; every expected answer comes from the
oracle or from the brute forces and generators of the neighbouring test modules."""
import ctypes as C
import hashlib
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from conftest import ROOT
import test_gpu_overlap as go
import test_gpu_point_query as gp
import test_gpu_query as gq
import test_gpu_scene as gs
from test_gpu_extended import indexed, packed36
from test_gpu_refit import jitter, no_negzero
from test_optimize import reference_optimize
from test_overlap import csr_of, make_boxes, overlap_brute_force, sorted_slices
from test_point_query import point_brute_force
from test_query import brute_force
from test_refit import reference_refit
from test_scene import scene_brute_force

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

GUARD = go.GUARD
GUARD_I32 = GUARD - (1 << 32)
MIN_DELAY_MS = 200.0


# ---- torch plumbing: tensors on a stream, the delay ----------------------------------------------------------------------------------------------------------

def to_dev(s, a):
    with torch.cuda.stream(s):
        return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def guarded(s, nbytes):
    assert nbytes % 4 == 0
    with torch.cuda.stream(s):
        return torch.full((max(nbytes // 4, 1),), GUARD_I32, dtype=torch.int32, device="cuda")


def to_host(s, t, dtype, count=None):
    s.synchronize()
    with torch.cuda.stream(s):
        a = t.cpu().numpy().reshape(-1).view(np.uint8)
    a = a[: a.size - a.size % np.dtype(dtype).itemsize].view(dtype)
    return a.copy() if count is None else a[:count].copy()


class Delay:
    """torch work that keeps a stream busy for a chosen time: a chain of 4096 x 4096 f32 matmuls (values stay bounded), sized by a measurement on the stream"""

    def __init__(self):
        n = 4096
        self.a = torch.full((n, n), 1.0 / n, device="cuda"); self.b = torch.ones((n, n), device="cuda"); self.c = torch.empty((n, n), device="cuda")
        torch.cuda.synchronize()
        self.ms_per_rep = None

    def _chain(self, reps):
        for _ in range(reps):
            torch.mm(self.a, self.b, out=self.c); torch.mm(self.a, self.c, out=self.b)

    def calibrate(self, s):
        with torch.cuda.stream(s):
            self._chain(4)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s); self._chain(16); e1.record(s)
        s.synchronize()
        self.ms_per_rep = e0.elapsed_time(e1) / 16.0

    def put(self, s, ms):
        """enqueue at least `ms` of work on s; returns (event before, event behind)"""
        if self.ms_per_rep is None:
            self.calibrate(s)
        reps = int(math.ceil(1.3 * ms / self.ms_per_rep)) + 2
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s); self._chain(reps); e1.record(s)
        return e0, e1


@pytest.fixture(scope="module")
def delay():
    return Delay()


def timed(s, fn):
    """duration of fn's work on the idle stream s (stream events)"""
    s.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s); fn(); e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1)


def ordered(delay, s, what, set_a, stage_b, call, consume, is_async):
    """the pattern of this module.  Inputs hold A and the step is timed on the idle stream; outputs are guard-filled and the inputs set to A again (set_a).  Then,
    with no host wait in between: a delay of at least 10 x the step (and 200 ms), stage_b (a device copy of B into the inputs, on s), the library call, the
    consumers (bvh_dev_copy / clones on s).  An asynchronous call must return while the delay's end event is still pending.  One synchronize, then the
    consumers' tensors are returned."""
    set_a(); s.synchronize()
    step = timed(s, call)
    set_a(); s.synchronize()
    e0, e1 = delay.put(s, max(MIN_DELAY_MS, 10.0 * step))
    with torch.cuda.stream(s):
        stage_b()
    call()
    pending_after_call = not e1.query()
    got = consume()
    pending_after_consumers = not e1.query()
    s.synchronize()
    d = e0.elapsed_time(e1)
    print(f"{what}: delay {d:.1f} ms, step {step:.3f} ms ({d / max(step, 1e-6):.0f} x)")
    assert d >= 10.0 * step and d >= MIN_DELAY_MS, f"{what}: the delay ({d:.1f} ms) does not outlast the step ({step:.3f} ms) tenfold"
    if is_async:
        assert pending_after_call, f"{what}: declared asynchronous, but the call returned only after the delay in front of it had completed (a hidden host wait)"
        assert pending_after_consumers, f"{what}: bvh_dev_copy / the consumers waited for the stream"
    return got


# ---- expected answers ---------------------------------------------------------------------------------------------------------------------------------------------

_ORC = {}


def ref_tree(orc, key, algo, tris, bits=30):
    k = (key, algo, bits)
    if k not in _ORC:
        _ORC[k] = orc.build_tree(algo, tris, morton_bits=bits)
    return _ORC[k]


def check_tree(orc, got, ref, algo, n, what=""):
    """tests/test_gpu_parity.py's bars: LBVH and PLOC++ by bytes, HPLOC by leaves, validity and canonical topology"""
    assert got["root"] == ref["root"], what
    if got.get("sorted_keys") is not None:
        assert np.array_equal(got["sorted_keys"], ref["skeys"]) and np.array_equal(got["sorted_vals"], ref["svals"]), what
    if algo in (0, 1):
        assert got["nodes"].tobytes() == ref["nodes"].tobytes(), f"{what}: Bvh2Node[2n-1] differs from the oracle"
    elif algo == 2:
        assert got["leaves"].tobytes() == ref["leaves"].tobytes() and got["nodes"].tobytes() == ref["nodes"].tobytes(), f"{what}: PLOC++ arrays differ from the oracle"
    else:
        assert got["leaves"].tobytes() == ref["leaves"].tobytes(), what
        assert orc.validate_bvh2(got["nodes"], got["leaves"], 0, n, 1) == 0, what
        assert orc.topology_hash(got["nodes"], got["leaves"], 0, n, 1) == orc.topology_hash(ref["nodes"], ref["leaves"], 0, n, 1), f"{what}: HPLOC topology differs"


def check_hits(pkg, got, bf, what):
    well, ref = bf["well"], bf["closest"]
    assert well.mean() >= 0.99, what
    for f in ("t", "u", "v", "prim"):
        eq = got[f].view(np.uint32) == ref[f].view(np.uint32)
        assert eq[well].all(), f"{what}: closest {f} differs on {np.count_nonzero(~eq & well)} well-conditioned rays"


def check_points(pkg, got, bf, what):
    well = bf["well"]
    assert well.mean() >= 0.99, what
    diff = (got.view(np.uint8).reshape(-1, 32) != bf["closest"].view(np.uint8).reshape(-1, 32)).any(axis=1)
    assert not (diff & well).any(), f"{what}: closest point differs on {np.count_nonzero(diff & well)} well-conditioned queries"


def check_refit(orc, got, before, moved, what):
    """tests/test_gpu_refit.py check_moved on downloaded arrays: links kept, leaf boxes stage E's, internal boxes the numpy reference refit"""
    n = len(moved)
    eb, _ = orc.prim_bounds(moved)
    assert got["root"] == before["root"] and np.array_equal(got["nodes"]["left"], before["nodes"]["left"]) and np.array_equal(got["nodes"]["right"], before["nodes"]["right"]), what
    ref_n, ref_l = reference_refit(before["nodes"], before["leaves"], before["root"], n, before["layout"], eb)
    if before["layout"] == 0:
        assert got["nodes"][n - 1:].tobytes() == ref_n[n - 1:].tobytes(), what
    else:
        assert got["leaves"].tobytes() == ref_l.tobytes(), what
    for f in ("min", "max"):
        assert np.array_equal(got["nodes"][f][:n - 1], ref_n[f][:n - 1]), f"{what}: internal {f} differs from the reference refit"


def check_optimized(got, before, n, layout, rounds, what):
    ref = reference_optimize(before["nodes"], before["leaves"], before["root"], n, layout, rounds)
    for f in ("left", "right", "min", "max"):
        assert np.array_equal(got["nodes"][f], ref[f]), f"{what}: {f} differs from the restatement of bvh_optimize"


def mostly_differ(a, b, what):
    """A and B must be told apart: their expected answers differ on most elements"""
    w = a.dtype.itemsize
    frac = (a.view(np.uint8).reshape(-1, w) != b.view(np.uint8).reshape(-1, w)).any(axis=1).mean()
    assert frac > 0.5, f"{what}: A's and B's answers differ on only {frac:.2f} of the elements"


def mesh_pair(pkg, n, seed):
    return no_negzero(pkg.meshgen.uniform(n, seed)), no_negzero(pkg.meshgen.uniform(n, seed + 100))


class DevTree:
    """torch tensors that receive a result's nodes, leaves and root box through bvh_dev_copy on the ctx's stream (the root box as bench.py copies it)"""

    def __init__(self, pkg, ctx, s, n, layout):
        self.pkg, self.ctx, self.s, self.n, self.layout = pkg, ctx, s, n, layout
        self.count = 2 * n - 1 if layout == 0 else n - 1
        self.nodes = guarded(s, self.count * 32); self.leaves = guarded(s, n * 28) if layout == 1 else None; self.root = guarded(s, 24)

    def reset(self):
        with torch.cuda.stream(self.s):
            for t in (self.nodes, self.leaves, self.root):
                if t is not None:
                    t.fill_(GUARD_I32)

    def copy(self, res):
        L, h = self.pkg.lib(), self.ctx.handle
        assert L.bvh_dev_copy(h, self.nodes.data_ptr(), res.d_nodes, self.count * 32) == 0
        if self.layout == 1:
            assert L.bvh_dev_copy(h, self.leaves.data_ptr(), res.d_leaves, self.n * 28) == 0
        assert L.bvh_dev_copy(h, self.root.data_ptr(), res.d_nodes + 32 * res.root + 8, 24) == 0

    def host(self, res):
        pkg = self.pkg
        nodes = to_host(self.s, self.nodes, pkg.BVH2_NODE, self.count)
        leaves = to_host(self.s, self.leaves, pkg.PRIMREF, self.n) if self.layout == 1 else None
        box = to_host(self.s, self.root, np.float32, 6)
        assert box.tobytes() == nodes[res.root]["min"].tobytes() + nodes[res.root]["max"].tobytes(), "the copied root box is not the copied tree's"
        return {"nodes": nodes, "leaves": leaves, "root": res.root, "layout": self.layout}


# ---- 1. a context on a caller's stream gives the same answers -------------------------------------------------------------------------------------------------------

def test_stream_handle_null_stream_and_close(pkg, orc):
    s = torch.cuda.Stream()
    ctx = pkg.Context(0, s.cuda_stream)
    other = pkg.Context.__new__(pkg.Context); other.handle, other.device, other._scenes = None, 0, set()
    try:
        assert s.cuda_stream != 0 and ctx.stream == s.cuda_stream
        # a NULL stream: as bvh_ctx_create — a stream of its own, and a build works
        own = C.c_void_p()
        assert pkg.lib().bvh_ctx_create_on_stream(0, None, C.byref(own)) == 0
        other.handle = own
        assert other.stream not in (0, s.cuda_stream)
        tris = pkg.meshgen.uniform(3000, 4)
        check_tree(orc, pkg.TwoPassLbvh().build(other, tris).download(), ref_tree(orc, "u3000", 0, tris), 0, len(tris), "NULL-stream ctx")
        check_tree(orc, pkg.HPLOC().build(ctx, tris).download(), ref_tree(orc, "u3000", 3, tris), 3, len(tris), "caller-stream ctx")
    finally:
        other.close(); ctx.close()
    # the caller's stream outlives the context: it was neither destroyed nor left in an error state
    with torch.cuda.stream(s):
        t = torch.arange(1 << 16, device="cuda") * 2
    s.synchronize()
    assert int(t[-1].item()) == 2 * ((1 << 16) - 1)


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_builds_from_torch_tensors(pkg, orc, algo):
    """every builder x {30, 60} Morton bits x {padded, packed36, indexed} from torch tensors on the caller's stream, against the oracle"""
    s = torch.cuda.Stream()
    ctx = pkg.Context(0, s.cuda_stream)
    try:
        for key, tris in (("u20k", pkg.meshgen.uniform(20_000, 17)), ("sponza120k", pkg.meshgen.sponza_like(120_000, 3))):
            n = len(tris)
            verts, idx = indexed(tris)
            d_pad, d_pk, d_v, d_i = to_dev(s, tris), to_dev(s, packed36(tris)), to_dev(s, verts), to_dev(s, idx)
            for bits in (30, 60):
                ref = ref_tree(orc, key, algo, tris, bits)
                for kw in (dict(tris=d_pad), dict(tris=d_pk, tri_format=pkg.TRI_PACKED36),
                           dict(vertices=d_v, indices=d_i, n_vertices=len(verts), tri_format=pkg.TRI_INDEXED)):
                    got = pkg.BUILDERS[algo]().build_ex(ctx, n, morton_bits=bits, **kw).download()
                    check_tree(orc, got, ref, algo, n, f"{key} algo {algo} bits {bits} format {kw.get('tri_format', 0)}")
    finally:
        ctx.close()
    s.synchronize()


def test_two_contexts_on_one_stream(pkg, orc):
    s = torch.cuda.Stream()
    c1, c2 = pkg.Context(0, s.cuda_stream), pkg.Context(0, s.cuda_stream)
    try:
        m1, m2 = pkg.meshgen.uniform(20_000, 17), pkg.meshgen.sponza_like(30_000, 5)
        d1, d2 = to_dev(s, m1), to_dev(s, m2)
        for a1, a2 in ((3, 0), (2, 3), (1, 2), (0, 1)):
            b1 = pkg.BUILDERS[a1]().build(c1, d1, on_device=True, n=len(m1))
            b2 = pkg.BUILDERS[a2]().build(c2, d2, on_device=True, n=len(m2))
            g1, g2 = b1.download(), b2.download()
            check_tree(orc, g1, ref_tree(orc, "u20k", a1, m1), a1, len(m1), f"first ctx algo {a1}")
            check_tree(orc, g2, ref_tree(orc, "sponza30k", a2, m2), a2, len(m2), f"second ctx algo {a2}")
    finally:
        c1.close(); c2.close()


# ---- the sequence of sections 1 and 5: build, checksum, queries, refit, optimise, query again -------------------------------------------------------------------------

class Io:
    """device buffers of one context: torch tensors under its caller's stream, or the C ABI's own allocations when the context owns its stream"""

    def __init__(self, ctx, s):
        self.ctx, self.s = ctx, s

    def up(self, a):
        return to_dev(self.s, a) if self.s is not None else self.ctx.upload(np.ascontiguousarray(a))

    def empty(self, nbytes):
        return guarded(self.s, nbytes) if self.s is not None else self.ctx.upload(np.full(max(nbytes // 4, 1), GUARD, dtype=np.uint32))

    def down(self, buf, dtype, count):
        return to_host(self.s, buf, dtype, count) if self.s is not None else buf.download(dtype, count)


def workload(pkg, n, seed, m):
    tris = no_negzero(pkg.meshgen.uniform(n, seed))
    moved = jitter(tris, seed + 1, 0.25 * 2.0 * n ** (-1.0 / 3.0))
    leaf = go.tri_boxes(tris)
    boxes, _ = make_boxes(leaf, seed + 2, m=m, points=go.vertices(tris))
    return {"n": n, "key": f"u{n}s{seed}", "tris": tris, "moved": moved, "rays": gq.make_rays(pkg, tris, m, seed + 3), "pts": gp.make_points(pkg, tris, m, seed + 4),
            "boxes": boxes, "leaf": leaf}


def _digest(d):
    h = hashlib.sha1()
    for k in sorted(d):
        v = d[k]
        if isinstance(v, dict):
            h.update(_digest(v).encode())
        elif v is not None:
            h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    return h.hexdigest()


def run_rounds(pkg, ctx, s, algo, W, rounds, keep_first=False):
    """-> (digest of every round's outputs, round 0's outputs or None)"""
    L, io, n = pkg.lib(), Io(ctx, s), W["n"]
    ctx.reserve(n)
    d_tris, d_moved, d_rays, d_pts, d_boxes = (io.up(W[k]) for k in ("tris", "moved", "rays", "pts", "boxes"))
    mr, mp, mb = len(W["rays"]), len(W["pts"]), len(W["boxes"])
    d_hits, d_phits, d_off, d_soff = io.empty(mr * 16), io.empty(mp * 32), io.empty((mb + 1) * 4), io.empty((n + 1) * 4)
    digests, first = [], None
    for r in range(rounds):
        b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
        res = C.byref(b.result)
        o = {"checksum": b.checksum(), "built": b.download()}
        assert L.bvh_intersect(ctx.handle, res, None, pkg._ptr(d_rays), mr, pkg._ptr(d_hits), pkg.QUERY_CLOSEST) == 0
        o["hits"] = io.down(d_hits, pkg.HIT, mr)
        assert L.bvh_closest_point(ctx.handle, res, None, pkg._ptr(d_pts), mp, pkg._ptr(d_phits), pkg.QUERY_CLOSEST) == 0
        o["phits"] = io.down(d_phits, pkg.POINT_HIT, mp)
        for name, ptr, m, mode, d_o in (("boxes", pkg._ptr(d_boxes), mb, pkg.OVERLAP_BOXES, d_off), ("self", b.result.d_prim_aabbs, n, pkg.OVERLAP_SELF, d_soff)):
            total = C.c_uint64()
            assert L.bvh_overlap(ctx.handle, res, ptr, m, mode, pkg._ptr(d_o), None, 0, C.byref(total)) == 0          # count, then the exact capacity
            d_prims = io.empty((total.value + 1) * 4)
            assert L.bvh_overlap(ctx.handle, res, ptr, m, mode, pkg._ptr(d_o), pkg._ptr(d_prims), total.value, C.byref(total)) == 0
            o["off_" + name] = io.down(d_o, np.uint32, m + 1); o["prims_" + name] = io.down(d_prims, np.uint32, total.value + 1)
            if s is None:
                d_prims.free()
        b.refit(d_moved, on_device=True, n=n)
        o["refit"] = b.download()
        b.optimize(3)
        o["opt"] = b.download()
        assert L.bvh_intersect(ctx.handle, res, None, pkg._ptr(d_rays), mr, pkg._ptr(d_hits), pkg.QUERY_CLOSEST) == 0
        o["hits2"] = io.down(d_hits, pkg.HIT, mr)
        digests.append(_digest(o))
        if r == 0 and keep_first:
            first = o
    if s is None:
        for buf in (d_tris, d_moved, d_rays, d_pts, d_boxes, d_hits, d_phits, d_off, d_soff):
            buf.free()
    return digests, first


def check_round(pkg, orc, algo, W, o, full):
    """one round's outputs against the oracle and the brute forces.  full: also the whole self-pair set and the restatement of bvh_optimize (numpy: small meshes);
    otherwise 2048 sampled rows of the self-pair answer, and the optimised tree must be valid with a SAH no higher than the refit tree's"""
    n, tris, moved, what = W["n"], W["tris"], W["moved"], f"{W['key']} algo {algo}"
    built = o["built"]; layout = built["layout"]
    check_tree(orc, built, ref_tree(orc, W["key"], algo, tris), algo, n, what)
    assert o["checksum"] == pkg.checksum_host(built["nodes"], built["leaves"], built["root"]), what
    check_hits(pkg, o["hits"], brute_force(W["rays"], tris), what + " intersect")
    check_points(pkg, o["phits"], point_brute_force(pkg, W["pts"], tris), what + " closest_point")
    ref_off, ref_prims = csr_of(overlap_brute_force(W["boxes"], W["leaf"]))
    go.check_answer(o["off_boxes"], o["prims_boxes"], ref_off, ref_prims, what + " overlap")
    off, prims = o["off_self"], o["prims_self"]
    if full:
        so, sp = csr_of(overlap_brute_force(W["leaf"], W["leaf"], self_pairs=True))
        go.check_answer(off, prims, so, sp, what + " self pairs")
    else:
        rows = np.random.default_rng(n).choice(n, size=2048, replace=False)
        sets = overlap_brute_force(W["leaf"][rows], W["leaf"])
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all() and prims[off[-1]] == GUARD
        for i, st in zip(rows, sets):
            assert np.array_equal(np.sort(prims[off[i]:off[i + 1]]), st[st > i]), f"{what}: self pairs of primitive {i}"
    check_refit(orc, o["refit"], built, moved, what + " refit")
    if full:
        check_optimized(o["opt"], o["refit"], n, layout, 3, what + " optimize")
    else:
        assert orc.validate_bvh2(o["opt"]["nodes"], o["opt"]["leaves"], o["opt"]["root"], n, layout) == 0
        sah = lambda t: orc.sah_bvh2(t["nodes"], t["leaves"], t["root"], n, layout)[0]
        assert sah(o["opt"]) <= sah(o["refit"])
    check_hits(pkg, o["hits2"], brute_force(W["rays"], moved), what + " intersect after refit + optimize")


@pytest.mark.parametrize("algo", [0, 3])
def test_calls_on_a_callers_stream(pkg, orc, algo):
    """refit, optimise, collapse, SAH, checksum, the three queries, build_boxes and a small scene on a caller's stream, arena reserved, torch tensors in and out"""
    s = torch.cuda.Stream()
    ctx = pkg.Context(0, s.cuda_stream)
    bl = gs.Blases(pkg)
    try:
        W = workload(pkg, 20_000, 40 + algo, 1536)
        n, tris = W["n"], W["tris"]
        _, o = run_rounds(pkg, ctx, s, algo, W, 1, keep_first=True)
        check_round(pkg, orc, algo, W, o, full=True)
        # collapse, SAH, build_boxes on a fresh build
        d_tris = to_dev(s, tris)
        b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
        got = b.download(); ref = ref_tree(orc, W["key"], algo, tris)
        s_ref = orc.sah_bvh2(ref["nodes"], ref["leaves"], ref["root"], n, ref["layout"])[0]
        assert abs(b.sah_cost() - s_ref) <= 1e-4 * s_ref
        d_w, d_p = guarded(s, n * 128), guarded(s, n * 8)
        nw = C.c_uint32()
        assert pkg.lib().bvh_collapse4(ctx.handle, C.byref(b.result), d_w.data_ptr(), d_p.data_ptr(), C.byref(nw)) == 0
        wide, prims = to_host(s, d_w, pkg.BVH4_NODE, nw.value), to_host(s, d_p, pkg.PRIM_NODE, n)
        ow, opn, ototal = orc.collapse4(got["nodes"], got["leaves"], got["root"], n, got["layout"])
        assert nw.value == ototal and orc.topology_hash4(wide, prims, nw.value, n) == orc.topology_hash4(ow, opn, ototal, n) != 0
        d_boxes = to_dev(s, W["leaf"])                               # (stage E's boxes: the contract gives the triangle build's tree)
        bb = pkg.BUILDERS[algo]().build_boxes(ctx, d_boxes, n=n).download()
        check_tree(orc, bb, ref, algo, n, "build_boxes")
        # a small scene: BLASes on contexts of their own, the scene on the caller's stream, device instances and rays
        rng = np.random.default_rng(3)
        meshes = [no_negzero(pkg.meshgen.uniform(k, 31 + k)) for k in (300, 200)]
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1])]
        inst, moved = gs.scene_instances(pkg, rng, 64, 2, 1.5), gs.scene_instances(pkg, np.random.default_rng(4), 64, 2, 1.7)
        d_inst, d_moved = to_dev(s, inst), to_dev(s, moved)
        scene = pkg.Scene(ctx).build(3, blases, (d_inst, 64))
        boxes = gs.root_boxes(pkg, blases)
        for d_i, ins, label in ((d_inst, inst, "built"), (d_moved, moved, "updated")):
            if label == "updated":
                scene.update((d_i, 64))
            rays = gq.make_rays(pkg, gs.world_tris(pkg, meshes, ins), 1536, 9)
            d_rays, outs = to_dev(s, rays), []
            for q in (pkg.QUERY_CLOSEST, pkg.QUERY_ANY):
                d_hits = guarded(s, len(rays) * 32)
                assert pkg.lib().bvh_scene_intersect(scene.handle, d_rays.data_ptr(), len(rays), d_hits.data_ptr(), q) == 0
                outs.append(to_host(s, d_hits, pkg.INSTANCE_HIT, len(rays)))
            gs.check_exact(pkg, rays, meshes, ins, scene_brute_force(pkg, rays, meshes, ins, boxes), outs[0], outs[1], f"scene {label}")
        scene.close()
    finally:
        ctx.close(); bl.close()
    with torch.cuda.stream(s):
        t = torch.ones(1024, device="cuda").sum()
    s.synchronize()
    assert float(t.item()) == 1024.0


# ---- 2, 3, 4. ordering in, ordering out, asynchrony -----------------------------------------------------------------------------------------------------------------

ORDERED_BUILDS = [("hploc", 3, True), ("hploc_tiles", 3, True), ("lbvh_two", 0, True), ("lbvh_single", 1, False), ("ploc", 2, False)]


@pytest.mark.parametrize("name,algo,is_async", ORDERED_BUILDS, ids=[b[0] for b in ORDERED_BUILDS])
def test_ordered_build(pkg, orc, delay, name, algo, is_async):
    """delay, copy of mesh B over mesh A, build, bvh_dev_copy of the tree: B's tree comes out.  HPLOC and two-pass LBVH return while the delay runs"""
    n = 50_000
    A, B = mesh_pair(pkg, n, 7)
    refA, refB = ref_tree(orc, "pairA", algo, A), ref_tree(orc, "pairB", algo, B)
    mostly_differ(refA["nodes"], refB["nodes"], "build")
    s = torch.cuda.Stream()
    ctx = pkg.Context(0, s.cuda_stream)
    try:
        ctx.reserve(n)
        if name == "hploc_tiles":
            ctx.set_option("hploc", "block")
        dA, dB, d_in = to_dev(s, A), to_dev(s, B), to_dev(s, A)
        out = DevTree(pkg, ctx, s, n, 1 if algo >= 2 else 0)
        b = pkg.BUILDERS[algo]()

        def set_a():
            with torch.cuda.stream(s):
                d_in.copy_(dA)
            out.reset()
        got = ordered(delay, s, f"build {name}", set_a, lambda: d_in.copy_(dB), lambda: b.build(ctx, d_in, on_device=True, n=n), lambda: out.copy(b.result), is_async)
        check_tree(orc, out.host(b.result), refB, algo, n, f"ordered build {name}")
    finally:
        ctx.close()


@pytest.mark.parametrize("algo", [0, 3])
def test_ordered_refit(pkg, orc, delay, algo):
    n = 50_000
    tris = no_negzero(pkg.meshgen.uniform(n, 21))
    scale = 0.25 * 2.0 * n ** (-1.0 / 3.0)
    A, B = jitter(tris, 1, scale), jitter(tris, 2, scale)
    mostly_differ(orc.prim_bounds(A)[0], orc.prim_bounds(B)[0], "refit")
    s = torch.cuda.Stream()
    ctx = pkg.Context(0, s.cuda_stream)
    try:
        ctx.reserve(n)
        d_tris, dA, dB, d_in = to_dev(s, tris), to_dev(s, A), to_dev(s, B), to_dev(s, A)
        b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=n)
        before = b.download()
        out = DevTree(pkg, ctx, s, n, before["layout"])
        lib = pkg.lib()

        def set_a():
            with torch.cuda.stream(s):
                d_in.copy_(dA)
            out.reset()

        def call():
            assert lib.bvh_refit(ctx.handle, C.byref(b.result), d_in.data_ptr(), 1, None) == 0
        ordered(delay, s, f"refit algo {algo}", set_a, lambda: d_in.copy_(dB), call, lambda: out.copy(b.result), True)
        check_refit(orc, out.host(b.result), before, B, f"ordered refit algo {algo}")
    finally:
        ctx.close()


def test_ordered_optimize(pkg, orc, delay):
    """the optimise's input is the tree: a two-pass build of mesh B (asynchronous) right behind the delay, the optimise behind it, the copies behind that"""
    n = 50_000
    A, B = mesh_pair(pkg, n, 7)
    refA, refB = ref_tree(orc, "pairA", 0, A), ref_tree(orc, "pairB", 0, B)
    optA, optB = (reference_optimize(r["nodes"], None, 0, n, 0, 3) for r in (refA, refB))
    mostly_differ(optA, optB, "optimize")
    s = torch.cuda.Stream()
    ctx = pkg.Context(0, s.cuda_stream)
    try:
        ctx.reserve(n)
        dA, dB, d_in = to_dev(s, A), to_dev(s, B), to_dev(s, A)
        out = DevTree(pkg, ctx, s, n, 0)
        b = pkg.TwoPassLbvh()
        lib = pkg.lib()

        def set_a():
            with torch.cuda.stream(s):
                d_in.copy_(dA)
            out.reset()

        def call():
            b.build(ctx, d_in, on_device=True, n=n)
            assert lib.bvh_optimize(ctx.handle, C.byref(b.result), 3, None) == 0
        ordered(delay, s, "optimize", set_a, lambda: d_in.copy_(dB), call, lambda: out.copy(b.result), True)
        got = out.host(b.result)
        assert b.result.root == 0
        for f in ("left", "right", "min", "max"):
            assert np.array_equal(got["nodes"][f], optB[f]), f"ordered optimize: {f} differs from the restatement of bvh_optimize on B's tree"
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def query_case(pkg):
    n, m = 20_000, 2048
    tris = no_negzero(pkg.meshgen.uniform(n, 33))
    other = no_negzero(pkg.meshgen.uniform(n, 34))
    leaf = go.tri_boxes(tris)
    c = {"n": n, "m": m, "tris": tris, "leaf": leaf}
    c["rays"] = [gq.make_rays(pkg, tris, m, sd) for sd in (1, 2)]
    c["bf_rays"] = [brute_force(r, tris) for r in c["rays"]]
    c["pts"] = [gp.make_points(pkg, tris, m, sd) for sd in (3, 4)]
    c["bf_pts"] = [point_brute_force(pkg, p, tris) for p in c["pts"]]
    # box queries: the usual mix (628 boxes, most of them off the mesh: empty answers for A and for B alike), then primitive boxes — A another mesh's, B this one's
    perm = np.random.default_rng(9).permutation(n)[: m - 628]
    c["boxes"] = [np.concatenate([make_boxes(leaf, sd, m=512, points=go.vertices(tris))[0], src[perm]]) for sd, src in ((5, go.tri_boxes(other)), (6, leaf))]
    c["bf_boxes"] = [csr_of(overlap_brute_force(b, leaf)) for b in c["boxes"]]
    c["self"] = [go.tri_boxes(other), leaf]
    c["bf_self"] = [csr_of(overlap_brute_force(b, leaf, self_pairs=True)) for b in c["self"]]
    return c


def _query_ctx(pkg, s, case, algo=3):
    ctx = pkg.Context(0, s.cuda_stream)
    ctx.reserve(case["n"])
    d_tris = to_dev(s, case["tris"])
    b = pkg.BUILDERS[algo]().build(ctx, d_tris, on_device=True, n=case["n"])
    ctx.synchronize()
    return ctx, b, d_tris


def test_ordered_intersect(pkg, delay, query_case):
    c = query_case; m = c["m"]
    mostly_differ(c["bf_rays"][0]["closest"], c["bf_rays"][1]["closest"], "intersect")
    s = torch.cuda.Stream()
    ctx, b, keep = _query_ctx(pkg, s, c)
    try:
        dA, dB, d_in = to_dev(s, c["rays"][0]), to_dev(s, c["rays"][1]), to_dev(s, c["rays"][0])
        d_c, d_a = guarded(s, m * 16), guarded(s, m * 16)
        lib = pkg.lib()

        def set_a():
            with torch.cuda.stream(s):
                d_in.copy_(dA); d_c.fill_(GUARD_I32); d_a.fill_(GUARD_I32)

        def call():
            assert lib.bvh_intersect(ctx.handle, C.byref(b.result), None, d_in.data_ptr(), m, d_c.data_ptr(), pkg.QUERY_CLOSEST) == 0
            assert lib.bvh_intersect(ctx.handle, C.byref(b.result), None, d_in.data_ptr(), m, d_a.data_ptr(), pkg.QUERY_ANY) == 0

        def consume():
            with torch.cuda.stream(s):
                return d_c.clone(), d_a.clone()
        k_c, k_a = ordered(delay, s, "intersect", set_a, lambda: d_in.copy_(dB), call, consume, True)
        gq.check_exact(pkg, c["rays"][1], c["tris"], c["bf_rays"][1], to_host(s, k_c, pkg.HIT, m), to_host(s, k_a, pkg.HIT, m), "ordered intersect")
    finally:
        ctx.close()


def test_ordered_closest_point(pkg, delay, query_case):
    c = query_case; m = c["m"]
    mostly_differ(c["bf_pts"][0]["closest"], c["bf_pts"][1]["closest"], "closest_point")
    s = torch.cuda.Stream()
    ctx, b, keep = _query_ctx(pkg, s, c, algo=0)
    try:
        dA, dB, d_in = to_dev(s, c["pts"][0]), to_dev(s, c["pts"][1]), to_dev(s, c["pts"][0])
        d_c, d_a = guarded(s, m * 32), guarded(s, m * 32)
        lib = pkg.lib()

        def set_a():
            with torch.cuda.stream(s):
                d_in.copy_(dA); d_c.fill_(GUARD_I32); d_a.fill_(GUARD_I32)

        def call():
            assert lib.bvh_closest_point(ctx.handle, C.byref(b.result), None, d_in.data_ptr(), m, d_c.data_ptr(), pkg.QUERY_CLOSEST) == 0
            assert lib.bvh_closest_point(ctx.handle, C.byref(b.result), None, d_in.data_ptr(), m, d_a.data_ptr(), pkg.QUERY_ANY) == 0

        def consume():
            with torch.cuda.stream(s):
                return d_c.clone(), d_a.clone()
        k_c, k_a = ordered(delay, s, "closest_point", set_a, lambda: d_in.copy_(dB), call, consume, True)
        gp.check_exact(pkg, c["pts"][1], c["tris"], c["bf_pts"][1], to_host(s, k_c, pkg.POINT_HIT, m), to_host(s, k_a, pkg.POINT_HIT, m), "ordered closest_point")
    finally:
        ctx.close()


@pytest.mark.parametrize("mode,with_total", [("boxes", False), ("self", False), ("boxes", True)])
def test_ordered_overlap(pkg, delay, query_case, mode, with_total):
    """bvh_overlap: asynchronous without total_out (the fill decides on the device); with total_out it blocks and must still read B"""
    c = query_case
    qs, refs = (c["boxes"], c["bf_boxes"]) if mode == "boxes" else (c["self"], c["bf_self"])
    m = len(qs[1]); assert len(qs[0]) == m
    (oa, pa), (ob, pb) = refs
    frac = np.mean([not np.array_equal(pa[oa[i]:oa[i + 1]], pb[ob[i]:ob[i + 1]]) for i in range(m)])
    assert frac > 0.5, f"A's and B's overlap sets differ on only {frac:.2f} of the queries"
    cap = int(max(refs[0][0][-1], refs[1][0][-1])) + 16
    s = torch.cuda.Stream()
    ctx, b, keep = _query_ctx(pkg, s, c, algo=2)
    try:
        dA, dB, d_in = to_dev(s, qs[0]), to_dev(s, qs[1]), to_dev(s, qs[0])
        d_off, d_prims = guarded(s, (m + 1) * 4), guarded(s, (cap + 1) * 4)
        lib = pkg.lib(); total = C.c_uint64()
        md = pkg.OVERLAP_SELF if mode == "self" else pkg.OVERLAP_BOXES

        def set_a():
            with torch.cuda.stream(s):
                d_in.copy_(dA); d_off.fill_(GUARD_I32); d_prims.fill_(GUARD_I32)

        def call():
            assert lib.bvh_overlap(ctx.handle, C.byref(b.result), d_in.data_ptr(), m, md, d_off.data_ptr(), d_prims.data_ptr(), cap, C.byref(total) if with_total else None) == 0

        def consume():
            with torch.cuda.stream(s):
                return d_off.clone(), d_prims.clone()
        k_off, k_prims = ordered(delay, s, f"overlap {mode}{' + total' if with_total else ''}", set_a, lambda: d_in.copy_(dB), call, consume, not with_total)
        ref_off, ref_prims = refs[1]
        if with_total:
            assert total.value == int(ref_off[-1])
        go.check_answer(to_host(s, k_off, np.uint32, m + 1), to_host(s, k_prims, np.uint32, cap + 1), ref_off, ref_prims, f"ordered overlap {mode}")
    finally:
        ctx.close()


def test_ordered_scene_update_and_intersect(pkg, delay):
    """a device instance array rewritten on the stream in front of bvh_scene_update; bvh_scene_intersect behind it answers for the new placement"""
    rng = np.random.default_rng(21)
    meshes = [no_negzero(pkg.meshgen.uniform(k, 5 + k)) for k in (150, 120)]
    bl = gs.Blases(pkg)
    s = torch.cuda.Stream()
    ctx = pkg.Context(0, s.cuda_stream)
    try:
        blases = [bl.add(3, meshes[0]), bl.add(1, meshes[1])]
        A, B = gs.scene_instances(pkg, rng, 64, 2, 1.5), gs.scene_instances(pkg, np.random.default_rng(22), 64, 2, 1.7)
        m = 2048
        rays = gq.make_rays(pkg, gs.world_tris(pkg, meshes, B), m, 23)
        boxes = gs.root_boxes(pkg, blases)
        bfA, bfB = scene_brute_force(pkg, rays, meshes, A, boxes), scene_brute_force(pkg, rays, meshes, B, boxes)
        hit = bfA["hit"] | bfB["hit"]
        assert hit.sum() > m // 10
        mostly_differ(bfA["closest"][hit], bfB["closest"][hit], "scene (rays that hit in A or B)")
        dA, dB, d_in, d_rays = to_dev(s, A), to_dev(s, B), to_dev(s, A), to_dev(s, rays)
        scene = pkg.Scene(ctx).build(3, blases, (d_in, 64))
        d_c, d_a = guarded(s, m * 32), guarded(s, m * 32)
        lib = pkg.lib()

        def set_a():
            with torch.cuda.stream(s):
                d_in.copy_(dA); d_c.fill_(GUARD_I32); d_a.fill_(GUARD_I32)

        def call():
            assert lib.bvh_scene_update(scene.handle, d_in.data_ptr(), 1, None) == 0
            assert lib.bvh_scene_intersect(scene.handle, d_rays.data_ptr(), m, d_c.data_ptr(), pkg.QUERY_CLOSEST) == 0
            assert lib.bvh_scene_intersect(scene.handle, d_rays.data_ptr(), m, d_a.data_ptr(), pkg.QUERY_ANY) == 0

        def consume():
            with torch.cuda.stream(s):
                return d_c.clone(), d_a.clone()
        k_c, k_a = ordered(delay, s, "scene_update + scene_intersect", set_a, lambda: d_in.copy_(dB), call, consume, True)
        gs.check_exact(pkg, rays, meshes, B, bfB, to_host(s, k_c, pkg.INSTANCE_HIT, m), to_host(s, k_a, pkg.INSTANCE_HIT, m), "ordered scene")
        scene.close()
    finally:
        ctx.close(); bl.close()


# ---- 5. independent contexts from host threads ------------------------------------------------------------------------------------------------------------------------

THREADS = [(5_000, 0, False), (20_000, 3, True), (60_000, 2, False), (300_000, 1, True)]     # (triangles, builder, on a torch stream)
ROUNDS = 5
PROFILED = 0                                                                                # thread 0 (two-pass LBVH) runs with set_profiling(2)


def test_contexts_in_host_threads(pkg, orc):
    works = [workload(pkg, n, 60 + k, 1536 if n <= 60_000 else 256) for k, (n, _, _) in enumerate(THREADS)]
    # serially, on ONE context, checked against the oracle and the brute forces; the kernel names of the profiled sequence likewise
    serial = pkg.Context(0)
    try:
        expect = []
        for W, (n, algo, _) in zip(works, THREADS):
            digests, first = run_rounds(pkg, serial, None, algo, W, ROUNDS, keep_first=True)
            check_round(pkg, orc, algo, W, first, full=n <= 20_000)
            assert len(set(digests)) == 1, "the serial rounds differ from each other"
            expect.append(digests)
        serial.set_profiling(2)
        run_rounds(pkg, serial, None, THREADS[PROFILED][1], works[PROFILED], ROUNDS)
        names_serial = serial.kernel_times()
        serial.set_profiling(0)
    finally:
        serial.close()
    assert names_serial and not any(k.startswith(("k_hploc", "k_ploc", "k_lbvh_single")) for k in names_serial), names_serial
    streams = [torch.cuda.Stream() if on_torch else None for _, _, on_torch in THREADS]
    ctxs, results, errors = [], [None] * len(THREADS), []
    start = threading.Barrier(len(THREADS))

    def body(k):
        try:
            start.wait(60)
            results[k] = run_rounds(pkg, ctxs[k], streams[k], THREADS[k][1], works[k], ROUNDS)[0]
        except BaseException as e:                                # noqa: BLE001 (reported by the main thread)
            errors.append((k, repr(e)))
    try:
        for st in streams:
            ctxs.append(pkg.Context(0, st.cuda_stream) if st is not None else pkg.Context(0))
        for k, c in enumerate(ctxs):
            c.set_profiling(2 if k == PROFILED else 0)
        threads = [threading.Thread(target=body, args=(k,)) for k in range(len(THREADS))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for k in range(len(THREADS)):
            assert results[k] == expect[k], f"thread {k} ({THREADS[k]}): rounds {[i for i in range(ROUNDS) if results[k][i] != expect[k][i]]} differ from the serial run"
        # the thread_local recorder: the profiled context names exactly the kernels of its own calls, with their launch counts; nobody else gained entries
        times = [c.kernel_times() for c in ctxs]
        assert {k: v[1] for k, v in times[PROFILED].items()} == {k: v[1] for k, v in names_serial.items()}
        assert all(not t for k, t in enumerate(times) if k != PROFILED), times
    finally:
        for c in ctxs:
            c.close()


CHILD = r"""
import sys, threading
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np
import bvh_pkg, oracle as orc
pkg = bvh_pkg.load(); pkg.lib(); orc.lib()
cases = [(0, pkg.meshgen.uniform(30_000, 1)), (1, pkg.meshgen.uniform(50_000, 2)), (2, pkg.meshgen.uniform(20_000, 3)), (3, pkg.meshgen.uniform(100_000, 4))]
start = threading.Barrier(4); got = [None] * 4; errors = []
def body(k):
    ctx = None
    try:
        start.wait(60)
        ctx = pkg.Context(0)                                       # four first contexts of the process at the same moment
        got[k] = pkg.BUILDERS[cases[k][0]]().build(ctx, cases[k][1]).download()
    except BaseException as e:
        errors.append((k, repr(e)))
    finally:
        if ctx is not None:
            ctx.close()
threads = [threading.Thread(target=body, args=(k,)) for k in range(4)]
[t.start() for t in threads]; [t.join() for t in threads]
assert not errors, errors
for (algo, tris), g in zip(cases, got):
    n = len(tris); ref = orc.build_tree(algo, tris)
    assert g["root"] == ref["root"] and np.array_equal(g["sorted_keys"], ref["skeys"]) and np.array_equal(g["sorted_vals"], ref["svals"])
    if algo in (0, 1, 2):
        assert g["nodes"].tobytes() == ref["nodes"].tobytes()
    if algo >= 2:
        assert g["leaves"].tobytes() == ref["leaves"].tobytes() and orc.validate_bvh2(g["nodes"], g["leaves"], 0, n, 1) == 0
        assert orc.topology_hash(g["nodes"], g["leaves"], 0, n, 1) == orc.topology_hash(ref["nodes"], ref["leaves"], 0, n, 1)
print("FIRST_CONTEXTS_OK")
"""


def test_first_contexts_of_a_process_from_four_threads():
    """the per-device call_once warm-up: a fresh child process (its own time limit, exit status checked) whose four threads create their contexts together"""
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0 and "FIRST_CONTEXTS_OK" in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
