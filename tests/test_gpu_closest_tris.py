"""bvh_closest_tris on the GPU: nearest-triangle and any-within-radius answers of every builder, both node layouts and all three triangle formats on either
side against the numpy brute force (tests/test_closest_tris.py), the stackless pass on trees deeper than the short stack, calls after a refit, an optimise and
a rebuild, caller-owned trees, the Python binding, consistency with bvh_intersect_tris, buffer hygiene and errors.  All shapes are small: the brute force is
every query triangle against every tree triangle, 15 terms each, computed once per input and shared across radii."""
import ctypes as C

import numpy as np
import pytest

from test_closest_tris import CROSSING, E_INVALID, below, pair_matrix, recompute_tris, tris_brute_force
from test_gpu_point_query import first_descent_pushes
from test_gpu_query import caterpillar, lbvh_result, mesh
from test_gpu_refit import jitter, no_negzero
from test_intersect_tris import as_triangles, shifted, xyz

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

F32 = np.float32
TREES = [f"uniform_{n}" for n in (2, 3, 63, 64, 65, 1000)] + ["sponza_1000", "cornell32", "cornell82", "cornell382"]
NAN_QUERIES = 8


def extent(tris):
    v = xyz(tris).reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    return lo, ext, float(np.linalg.norm(ext))


def make_queries(pkg, tris, seed):
    """768 query triangles for a tree over ``tris``: the tree's own mesh shifted (crossing and near pairs), random small triangles inside and outside the box,
    triangles that share a vertex or an edge with tree triangles, exact copies, copies moved along their normal, scene-spanning triangles, degenerate point and
    segment triangles and, last, NAN_QUERIES triangles with a NaN coordinate"""
    rng = np.random.default_rng(seed)
    t = xyz(tris); n = len(t)
    lo, ext, diag = extent(tris)
    parts = []
    parts.append(xyz(shifted(pkg, tris))[rng.integers(0, n, 240)])
    c = lo - 0.5 * ext + rng.random((200, 1, 3)) * 2.0 * ext                                     # small, inside and outside the box
    parts.append(c + rng.normal(0, 1, (200, 3, 3)) * ext * rng.choice([1e-3, 2e-2, 0.1], size=(200, 1, 1)))
    s = t[rng.integers(0, n, 96)].astype(np.float64)                                             # a shared vertex (first half) or edge (second half)
    s[:, 2] = s[:, 0] + rng.normal(0, 0.05, (96, 3)) * ext
    s[:48, 1] = s[:48, 0] + rng.normal(0, 0.05, (48, 3)) * ext
    parts.append(np.stack([np.roll(x, r, axis=0) for x, r in zip(s, rng.integers(0, 3, 96))]))
    parts.append(t[rng.integers(0, n, 48)])                                                      # exact copies
    k = t[rng.integers(0, n, 96)].astype(np.float64)                                             # copies moved along their normal
    nrm = np.cross(k[:, 1] - k[:, 0], k[:, 2] - k[:, 0]); ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), (0.0, 0.0, 1.0))
    parts.append(k + (nrm * diag * rng.choice([1e-4, 1e-3, 2e-2], size=(96, 1)) * rng.choice([-1.0, 1.0], size=(96, 1)))[:, None, :])
    parts.append(lo - 0.25 * ext + rng.random((24, 3, 3)) * 1.5 * ext)                           # scene-spanning
    p = lo - 0.25 * ext + rng.random((56, 1, 3)) * 1.5 * ext                                     # degenerate: points, then segments
    d = np.repeat(p, 3, axis=1)
    d[28:, 1] += rng.normal(0, 0.05, (28, 3)) * ext; d[42:, 2] = d[42:, 1]
    parts.append(d)
    bad = lo + rng.random((NAN_QUERIES, 3, 3)) * ext
    for j in range(NAN_QUERIES):
        bad[j, j % 3, (j // 3) % 3] = np.nan
    parts.append(bad)
    q = np.concatenate([np.asarray(x, dtype=np.float64) for x in parts]).astype(F32)
    assert len(q) == 768
    return no_negzero(as_triangles(pkg, q))


def radii(tris):
    return {"inf": np.inf, "band": 2e-3 * extent(tris)[2], "zero": 0.0, "negative": -1.0, "nan": np.nan}


_REF = {}


def reference(pkg, name, tris=None, seed=None):
    """(queries, {radius label: (radius, brute force)}) per input, computed once and shared"""
    if name not in _REF:
        tris = mesh(pkg, name) if tris is None else tris
        q = make_queries(pkg, tris, 17 + len(tris) if seed is None else seed)
        pairs = pair_matrix(q, tris)
        _REF[name] = (q, {label: (r, tris_brute_force(pkg, q, tris, r, pairs)) for label, r in radii(tris).items()})
    return _REF[name]


def raw(pkg, ctx, result, d_q, m, radius, kind, tin=None, qin=None):
    hits = ctx.alloc(m * 16)
    try:
        qin = qin if qin is not None else pkg.BuildInput(pkg.TRI_PADDED64, 30, d_q.ptr, None, None, 0, 0)
        rc = pkg.lib().bvh_closest_tris(ctx.handle, C.byref(result), C.byref(tin) if tin is not None else None, C.byref(qin), m, radius, hits.ptr, kind)
        assert rc == 0, rc
        return hits.download(pkg.TRI_HIT, m)
    finally:
        hits.free()


def check_exact(pkg, q, tris, radius, bf, closest, anyhit, what):
    well = bf["well"]
    assert well.mean() >= 0.99, f"{what}: only {well.mean():.4f} of the queries are well-conditioned"
    ref = bf["closest"]
    diff = (closest.view(np.uint8).reshape(-1, 16) != ref.view(np.uint8).reshape(-1, 16)).any(axis=1)
    assert not (diff & well).any(), f"{what}: closest differs on {np.count_nonzero(diff & well)} well-conditioned queries (first {np.nonzero(diff & well)[0][:6]})"
    hit_any = anyhit["prim"] != pkg.INVALID
    assert (hit_any == bf["hit"])[well].all(), f"{what}: any hit/miss differs"
    # every query: reported hits are accepted candidates with bit-equal records, misses the exact miss record; no closest answer below the brute force
    assert recompute_tris(pkg, q, tris, radius, closest).all(), f"{what}: a closest record is not an accepted candidate of its prim (or not the miss record)"
    assert recompute_tris(pkg, q, tris, radius, anyhit).all(), f"{what}: an any record is not an accepted candidate of its prim (or not the miss record)"
    assert not below(pkg, closest, ref).any(), f"{what}: closest below the brute force"


def check_all_radii(pkg, ctx, result, q, d_q, tris, ref, what, tin=None):
    out = {}
    for label, (radius, bf) in ref.items():
        c = raw(pkg, ctx, result, d_q, len(q), radius, pkg.QUERY_CLOSEST, tin)
        a = raw(pkg, ctx, result, d_q, len(q), radius, pkg.QUERY_ANY, tin)
        check_exact(pkg, q, tris, radius, bf, c, a, f"{what} radius {label}")
        out[label] = c
    return out


@pytest.mark.parametrize("name", TREES)
def test_exact_against_brute_force(pkg, ctx, name):
    tris = mesh(pkg, name)
    q, ref = reference(pkg, name)
    inf = ref["inf"][1]
    assert inf["hit"][:-NAN_QUERIES].all() and not inf["hit"][-NAN_QUERIES:].any()
    assert not ref["negative"][1]["hit"].any() and not ref["nan"][1]["hit"].any() and ref["zero"][1]["hit"].any() and not ref["band"][1]["hit"].all()
    assert (inf["closest"]["feature"] == CROSSING).any()
    d_q = ctx.upload(q)
    per_algo = {}
    try:
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(ctx, tris)
            keep = []
            results = [("as built", b.result)]
            if b.result.layout == 1:
                results.append(("lbvh layout", lbvh_result(pkg, ctx, b, keep)))
            for label, res in results:
                got = check_all_radii(pkg, ctx, res, q, d_q, tris, ref, f"{name} algo {algo} {label}")
                per_algo.setdefault(algo, got)
            for k in keep:
                k.free()
    finally:
        d_q.free()
    for label, (_, bf) in ref.items():
        well = bf["well"]
        for algo in (1, 2, 3):
            assert per_algo[algo][label][well].tobytes() == per_algo[0][label][well].tobytes(), f"{name} radius {label}: builders {algo} and 0 differ"


def formats_of(pkg, ctx, t):
    """the three device forms of a mesh: {format: (BuildInput, buffers)}"""
    n = len(t)
    packed = np.ascontiguousarray(xyz(t).reshape(n, 9))
    uniq, inv = np.unique(packed.reshape(-1, 3), axis=0, return_inverse=True)
    # (np.unique sorts NaN rows last and keeps them apart: the indexed form still reproduces every coordinate bit for bit except NaN payloads, which no test reads)
    d_t, d_p, d_v, d_i = ctx.upload(t), ctx.upload(packed), ctx.upload(np.ascontiguousarray(uniq.astype(F32))), ctx.upload(inv.reshape(-1).astype(np.uint32))
    return {
        "padded": pkg.BuildInput(pkg.TRI_PADDED64, 30, d_t.ptr, None, None, 0, 0),
        "packed": pkg.BuildInput(pkg.TRI_PACKED36, 30, d_p.ptr, None, None, 0, 0),
        "indexed": pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, len(uniq), 0),
    }, (d_t, d_p, d_v, d_i)


@pytest.mark.parametrize("name", ["uniform_1000", "cornell382"])
def test_formats_give_identical_bytes(pkg, ctx, name):
    tris = mesh(pkg, name)
    q, ref = reference(pkg, name)
    b = pkg.HPLOC().build(ctx, tris)
    tf, tbuf = formats_of(pkg, ctx, tris)
    qf, qbuf = formats_of(pkg, ctx, q)
    try:
        for label in ("inf", "band"):
            radius, bf = ref[label]
            for kind in (pkg.QUERY_CLOSEST, pkg.QUERY_ANY):
                base = raw(pkg, ctx, b.result, None, len(q), radius, kind, None, qf["padded"])
                for tn, tin in tf.items():
                    for qn, qin in qf.items():
                        got = raw(pkg, ctx, b.result, None, len(q), radius, kind, tin, qin)
                        assert got.tobytes() == base.tobytes(), f"{name} radius {label} kind {kind}: tree {tn} / queries {qn} differ from padded / padded"
        c = raw(pkg, ctx, b.result, None, len(q), np.inf, pkg.QUERY_CLOSEST, tf["indexed"], qf["packed"])
        well = ref["inf"][1]["well"]
        assert c[well].tobytes() == ref["inf"][1]["closest"][well].tobytes()
    finally:
        for x in tbuf + qbuf:
            x.free()


def caterpillar_queries(pkg, H, m=240):
    """small triangles below the face at z = 0 (every box passes an unbounded query: the first descent pushes at every chain node), some ON the face, some with
    a radius' worth of nothing near them, and some among the far triangles"""
    rng = np.random.default_rng(H)
    c = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-3, -0.5, m)], axis=1)
    c[: m // 6, 2] = 0.25                                      # between the faces at z = 0 and z = 0.5
    c[3 * m // 4:, 2] = rng.uniform(1000, 1000 + 2 * H, m - 3 * m // 4)
    q = c[:, None, :] + rng.normal(0, 0.05, (m, 3, 3))
    q[m // 6: m // 3, :, 2] = 0.0                              # coplanar with the face at z = 0: distance exactly 0
    q[m // 3: m // 2, 0, 2] = 0.75; q[m // 3: m // 2, 1:, 2] = -0.5     # through both near faces: proper crossings
    return as_triangles(pkg, q.astype(F32))


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("H", [70, 250])
def test_deep_tree_takes_the_stackless_pass(pkg, H, layout):
    tris, nodes, root, n = caterpillar(pkg, H, 5 + H)
    q = caterpillar_queries(pkg, H)
    m = len(q)
    cen = xyz(q).astype(np.float64).mean(axis=1)
    assert max(first_descent_pushes(nodes, root, n - 1, cen[j]) for j in range(m // 6)) > 64
    pairs = pair_matrix(q, tris)
    c = pkg.Context(0)
    try:
        c.reserve(n)
        bufs = [c.upload(tris), c.upload(q)]
        r = pkg.Result(); r.d_tris = bufs[0].ptr; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = layout
        if layout == 0:
            bufs.append(c.upload(nodes)); r.d_nodes = bufs[-1].ptr
        else:
            leaves = np.zeros(n, dtype=pkg.PRIMREF)
            leaves["prim"] = nodes["left"][n - 1:]; leaves["min"] = nodes["min"][n - 1:]; leaves["max"] = nodes["max"][n - 1:]
            bufs += [c.upload(np.ascontiguousarray(nodes[: n - 1])), c.upload(leaves)]
            r.d_nodes = bufs[-2].ptr; r.d_leaves = bufs[-1].ptr
        for radius in (np.inf, 5.0):
            bf = tris_brute_force(pkg, q, tris, radius, pairs)
            assert bf["well"].all() and bf["hit"].any() and (bf["closest"]["feature"] == CROSSING).any()
            c.set_profiling(2)
            closest = raw(pkg, c, r, bufs[1], m, radius, pkg.QUERY_CLOSEST)
            anyhit = raw(pkg, c, r, bufs[1], m, radius, pkg.QUERY_ANY)
            kt = c.kernel_times()
            c.set_profiling(0)
            assert {"k_closest_tris", "k_closest_tris_deep", "k_refit_plan"} <= set(kt)
            assert closest.tobytes() == bf["closest"].tobytes()
            assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"]).all() and recompute_tris(pkg, q, tris, radius, anyhit).all()
        for b in bufs:
            b.free()
    finally:
        c.close()


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
def test_after_refit_optimize_and_rebuild(pkg, algo):
    a = mesh(pkg, "uniform_1000"); moved = jitter(a, 19, 2e-3)
    other = mesh(pkg, "sponza_1000")
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, a)
        q, ref = reference(pkg, "uniform_1000_jittered", moved, 8)
        d_q = c.upload(q)
        b.closest_tris(q)                                     # (the plan of the ctx's own tree is made here and kept)
        b.refit(moved)
        check_all_radii(pkg, c, b.result, q, d_q, moved, ref, f"refit algo {algo}")
        b.optimize(3)
        check_all_radii(pkg, c, b.result, q, d_q, moved, ref, f"optimize algo {algo}")
        d_q.free()
        b2 = pkg.BUILDERS[algo]().build(c, other)
        q2, ref2 = reference(pkg, "sponza_1000")
        d_q2 = c.upload(q2)
        check_all_radii(pkg, c, b2.result, q2, d_q2, other, ref2, f"rebuild algo {algo}")
        d_q2.free()
    finally:
        c.close()


def test_caller_owned_trees_use_a_per_call_plan(pkg):
    """two caller-owned layout-0 copies of different trees and the ctx's own tree, queried in turn on one ctx: each call must walk with its own tree's plan"""
    ta, tb = mesh(pkg, "uniform_1000"), mesh(pkg, "sponza_1000")
    qa, ra = reference(pkg, "uniform_1000"); qb, rb = reference(pkg, "sponza_1000")
    c = pkg.Context(0)
    try:
        ba = pkg.PLOCNew().build(c, ta)
        keep = []
        ca = lbvh_result(pkg, c, ba, keep)
        d_ta = c.upload(ta); ca.d_tris = d_ta.ptr
        bb = pkg.PLOCNew().build(c, tb)                       # the ctx's own tree is now b's; a's arrays live on in the caller's buffer
        cb = lbvh_result(pkg, c, bb, keep)
        d_qa, d_qb = c.upload(qa), c.upload(qb)
        radius, bfa = ra["inf"]; _, bfb = rb["inf"]
        for _ in range(2):
            for res, q, d_q, bf in ((ca, qa, d_qa, bfa), (bb.result, qb, d_qb, bfb), (cb, qb, d_qb, bfb), (ca, qa, d_qa, bfa)):
                # the deep pass is what reads the plan: a radius of inf on 1000 triangles rarely overflows, so the plan is also checked through its kernel
                c.set_profiling(2)
                got = raw(pkg, c, res, d_q, len(q), radius, pkg.QUERY_CLOSEST)
                kt = c.kernel_times()
                c.set_profiling(0)
                assert got[bf["well"]].tobytes() == bf["closest"][bf["well"]].tobytes()
                if res is not bb.result:
                    assert "k_refit_plan" in kt               # caller-owned arrays: the plan is made on every call
        for x in keep + [d_ta, d_qa, d_qb]:
            x.free()
    finally:
        c.close()


def test_binding_and_distance_to(pkg, ctx):
    tris = mesh(pkg, "sponza_1000")
    q, ref = reference(pkg, "sponza_1000")
    b = pkg.SinglePassLbvh().build(ctx, tris)
    d_q = ctx.upload(q)
    try:
        for label, (radius, bf) in ref.items():
            for kind, word in ((pkg.QUERY_CLOSEST, "closest"), (pkg.QUERY_ANY, "any")):
                want = raw(pkg, ctx, b.result, d_q, len(q), radius, kind).tobytes()
                assert b.closest_tris(q, radius=radius, query=word).tobytes() == want
                assert b.closest_tris(d_q, radius=radius, query=kind).tobytes() == want                       # a device buffer of TRIANGLE records
                assert b.closest_tris(xyz(q).reshape(-1, 9), radius=radius, query=word).tobytes() == want      # host floats: uploaded as PACKED36
        assert b.closest_tris(q).tobytes() == raw(pkg, ctx, b.result, d_q, len(q), np.inf, pkg.QUERY_CLOSEST).tobytes()   # radius None: unbounded
        assert len(b.closest_tris(q[:0])) == 0
        # distance_to: the brute force's global minimum — on queries free of copies and contacts too, so that the minimum is not 0
        bf = ref["inf"][1]
        for sel in (np.arange(len(q)), np.nonzero(bf["closest"]["dist2"] > 0)[0]):
            rec, well = bf["closest"][sel], bf["well"][sel]
            idx = np.nonzero(rec["prim"] != pkg.INVALID)[0]
            i = int(idx[np.argmin(rec["dist2"][idx])])
            assert well[i]
            dist, qi, prim = b.distance_to(q[sel])
            assert (dist, qi, prim) == (float(np.sqrt(np.float64(rec["dist2"][i]))), i, int(rec["prim"][i]))
        assert ref["inf"][1]["closest"]["dist2"].min() == 0 and dist > 0
    finally:
        d_q.free()


@pytest.mark.parametrize("name", ["uniform_1000", "cornell382", "sponza_1000"])
def test_consistent_with_intersect_tris(pkg, ctx, name):
    tris = mesh(pkg, name)
    q, ref = reference(pkg, name)
    bf = ref["inf"][1]
    b = pkg.HPLOC().build(ctx, tris)
    got = b.closest_tris(q)
    offsets, prims = b.intersect_tris(q)
    rows = np.diff(offsets.astype(np.int64)) > 0
    assert rows.any()
    in_row = np.array([got["prim"][i] in prims[offsets[i]:offsets[i + 1]] for i in range(len(q))])
    crossing = (got["dist2"] == 0) & (got["feature"] == CROSSING) & (got["prim"] != pkg.INVALID)
    well = bf["well"]
    assert (crossing == in_row)[well].all(), f"{name}: feature 15 and the crossing rows disagree on {np.count_nonzero((crossing != in_row) & well)} queries"
    assert (got["dist2"][rows] == 0).all() and (got["prim"][rows] != pkg.INVALID).all()      # every query that crosses something is at distance 0


def test_buffers_untouched_outside_the_hits(pkg, ctx):
    tris = mesh(pkg, "uniform_1000")
    q, ref = reference(pkg, "uniform_1000")
    m, extra = len(q) - 5, 37                                 # (a count that is no multiple of the workgroup)
    b = pkg.HPLOC().build(ctx, tris)
    d_q = ctx.upload(q)
    sentinel = np.frombuffer(np.full((m + 2 * extra) * 16, 0xA5, dtype=np.uint8).tobytes(), dtype=pkg.TRI_HIT)
    hits = ctx.upload(sentinel)
    qin = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_q.ptr, None, None, 0, 0)
    L = pkg.lib()
    try:
        for kind in (0, 1):
            for label in ("inf", "band", "nan"):
                radius = ref[label][0]
                hits.upload(sentinel)
                assert L.bvh_closest_tris(ctx.handle, C.byref(b.result), None, C.byref(qin), m, radius, hits.ptr + extra * 16, kind) == 0
                out = hits.download(pkg.TRI_HIT, m + 2 * extra)
                assert out[:extra].tobytes() == sentinel[:extra].tobytes() and out[extra + m:].tobytes() == sentinel[extra + m:].tobytes()
                assert recompute_tris(pkg, q[:m], tris, radius, out[extra: extra + m]).all()
                assert d_q.download(pkg.meshgen.TRIANGLE, len(q)).tobytes() == q.tobytes()
        hits.upload(sentinel)
        assert L.bvh_closest_tris(ctx.handle, C.byref(b.result), None, C.byref(qin), 0, np.inf, hits.ptr, 0) == 0       # n_queries == 0: nothing touched
        ctx.synchronize()
        assert hits.download(pkg.TRI_HIT, m + 2 * extra).tobytes() == sentinel.tobytes()
    finally:
        d_q.free(); hits.free()


def test_errors_write_nothing(pkg):
    tris = mesh(pkg, "uniform_1000"); n = len(tris)
    q, _ = reference(pkg, "uniform_1000")
    m = 256
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        d_q = c.upload(q)
        d_v, d_i = c.upload(np.ascontiguousarray(xyz(q).reshape(-1, 3))), c.upload(np.arange(3 * len(q), dtype=np.uint32))
        sentinel = np.frombuffer(np.full(m * 16, 0x5A, dtype=np.uint8).tobytes(), dtype=pkg.TRI_HIT)
        hits = c.upload(sentinel)
        L = pkg.lib()
        padded = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_q.ptr, None, None, 0, 0)
        none = object()

        def call(res=b.result, inp=None, qin=padded, k=m, radius=1.0, h=hits.ptr, kind=0, ctx=c.handle):
            return L.bvh_closest_tris(ctx, C.byref(res) if res is not None else None, C.byref(inp) if inp is not None else None,
                                      C.byref(qin) if qin is not none else None, k, radius, h, kind)

        def variant(**kw):
            r = pkg.Result.from_buffer_copy(b.result)
            for key, v in kw.items():
                setattr(r, key, v)
            return r
        nodes_bytes = (n - 1) * 32
        cases = {
            "null ctx": call(ctx=None), "null tree": call(res=None), "null hits": call(h=None), "null queries": call(qin=none),
            "n_leaves 1": call(res=variant(n_leaves=1)), "layout 2": call(res=variant(layout=2)), "null nodes": call(res=variant(d_nodes=None)),
            "layout 1 without leaves": call(res=variant(d_leaves=None)), "root not internal": call(res=variant(root=n - 1)),
            "no triangles": call(res=variant(d_tris=None)), "bad tree format": call(inp=pkg.BuildInput(7, 30, b.result.d_tris, None, None, 0, 0)),
            "tree packed unaligned": call(inp=pkg.BuildInput(pkg.TRI_PACKED36, 30, b.result.d_tris + 4, None, None, 0, 0)),
            "tree indexed without vertices": call(inp=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, None, b.result.d_tris, 3, 0)),
            "bad query format": call(qin=pkg.BuildInput(7, 30, d_q.ptr, None, None, 0, 0)),
            "queries null tris": call(qin=pkg.BuildInput(pkg.TRI_PADDED64, 30, None, None, None, 0, 0)),
            "queries packed unaligned": call(qin=pkg.BuildInput(pkg.TRI_PACKED36, 30, d_q.ptr + 4, None, None, 0, 0)),
            "queries indexed without indices": call(qin=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, None, 3 * len(q), 0)),
            "queries indexed without vertices": call(qin=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, None, d_i.ptr, 3 * len(q), 0)),
            "queries indexed n_vertices 0": call(qin=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, 0, 0)),
            "too many queries": call(k=1 << 30), "query 2": call(kind=2), "query -1": call(kind=-1),
            "hits over the queries": call(h=d_q.ptr + 64), "hits end in the queries": call(qin=pkg.BuildInput(pkg.TRI_PADDED64, 30, hits.ptr + 16 * (m - 1), None, None, 0, 0)),
            "hits over the query vertices": call(qin=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, 3 * len(q), 0), h=d_v.ptr + 16),
            "hits over the query indices": call(qin=pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, 3 * len(q), 0), h=d_i.ptr + 16),
            "hits over the nodes": call(h=b.result.d_nodes + nodes_bytes - 16), "hits over the tree triangles": call(h=b.result.d_tris + 64),
            "hits over the leaves": call(h=b.result.d_leaves + 28 * 4) if b.result.layout == 1 else E_INVALID,
            "above capacity": call(res=variant(n_leaves=n + 1_000_000, root=0)),
        }
        assert all(rc == E_INVALID for rc in cases.values()), {k: v for k, v in cases.items() if v != E_INVALID}
        c.synchronize()
        assert hits.download(pkg.TRI_HIT, m).tobytes() == sentinel.tobytes()
        # on a fresh ctx (capacity 0) a caller tree is refused until bvh_ctx_reserve
        c2 = pkg.Context(0)
        try:
            assert L.bvh_closest_tris(c2.handle, C.byref(b.result), None, C.byref(padded), m, 1.0, hits.ptr, 0) == E_INVALID
        finally:
            c2.close()
        assert hits.download(pkg.TRI_HIT, m).tobytes() == sentinel.tobytes()
        assert call() == 0                                    # the same arguments without a fault go through
        for x in (d_q, d_v, d_i, hits):
            x.free()
    finally:
        c.close()
