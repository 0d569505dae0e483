"""The stackless *_deep query kernels on the GPU, on the trees and calls the other deep tests leave out: layout-1 trees (a hand-made caterpillar in caller-owned
arrays, PLOC++ / HPLOC trees over the staircase of tests/test_deep_trees.py in the ctx's arena), every triangle format, the cached parent plan across refit /
refit_subset / optimize / rebuild, calls above the deep kernels' grid (65 536 queries), deep top-level and bottom-level trees of scenes, and the conservative box
tests at other scales than the unit cube.

Every answer is compared with the numpy brute force of its family: bit-exact on the well-conditioned queries (tobytes() where all of them are), recompute on
all.  Before each comparison the tree about to be queried is downloaded and the walk restatements of tests/test_deep_trees.py assert that the call holds
overflowing queries (and, on the staircase, quiet ones in the same waves): the deep kernels are launched on every call, so their names in kernel_times() prove
nothing."""
import ctypes as C

import numpy as np
import pytest

from test_deep_trees import (F32, LEFT_FIRST, M_PLAN, QUERY_STACK, SCALES, STAIR_SHIFTS, assert_mixed, caterpillar_case, caterpillar_scene,
                             caterpillar_self_boxes, combined, height, needs, plan_case, quiet_queries, reference, scale_reference, scene_needs, stair_case, stairs,
                             staircase_scene, tlas_scene, to_layout1)
from test_gpu_knn import check_exact as knn_check_exact
from test_gpu_knn import knn
from test_gpu_multihit import all_hits, chain_left
from test_gpu_overlap import check_answer, overlap, tri_boxes
from test_gpu_point_query import check_exact as point_check_exact
from test_gpu_point_query import query as point_query
from test_gpu_query import check_exact as ray_check_exact
from test_gpu_query import mesh
from test_gpu_query import query as ray_query
from test_gpu_radius import search
from test_gpu_scene import Blases
from test_knn import truncate
from test_multihit import HITS_SORTED, check_all_hits
from test_overlap import csr_of, overlap_brute_force, sorted_slices
from test_radius import RADIUS_SORTED, check_radius
from test_scene import scene_brute_force, scene_recompute

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

FAMILIES = ("intersect", "intersect_all", "closest_point", "knn", "radius", "overlap")
KS = (1, 8, 32)


# ---- one family: its brute force, its calls through the C ABI, its checks ------------------------------------------------------------------------------------

def run(pkg, ctx, res, family, q, inp=None):
    """every variant of the family on tree `res`: closest and any; count-only (inside all_hits / search / overlap), unsorted and sorted fills; k = 1, 8, 32"""
    if family == "intersect":
        return {"closest": ray_query(pkg, ctx, res, q, pkg.QUERY_CLOSEST, inp), "any": ray_query(pkg, ctx, res, q, pkg.QUERY_ANY, inp)}
    if family == "intersect_all":
        return {"sorted": all_hits(pkg, ctx, res, q, HITS_SORTED, inp), "unsorted": all_hits(pkg, ctx, res, q, 0, inp)}
    if family == "closest_point":
        return {"closest": point_query(pkg, ctx, res, q, pkg.QUERY_CLOSEST, inp), "any": point_query(pkg, ctx, res, q, pkg.QUERY_ANY, inp)}
    if family == "knn":
        return {k: knn(pkg, ctx, res, q, k, inp) for k in KS}
    if family == "radius":
        return {"sorted": search(pkg, ctx, res, q, RADIUS_SORTED, inp), "unsorted": search(pkg, ctx, res, q, 0, inp)}
    rc, off, prims, total = overlap(pkg, ctx, res, q, guard=8)              # (a count-only call first, then the fill with the exact capacity)
    assert rc == 0
    return {"offsets": off, "prims": prims, "total": total}


def check(pkg, family, q, tris, ref, got, what):
    exact = bool(ref["well"].all())
    if family == "intersect":
        ray_check_exact(pkg, q, tris, ref, got["closest"], got["any"], what)
        if exact:
            assert got["closest"].tobytes() == ref["closest"].tobytes(), what
    elif family == "intersect_all":
        check_all_hits(q, tris, ref, got["sorted"][0], got["sorted"][1], True, what + " sorted")
        check_all_hits(q, tris, ref, got["unsorted"][0], got["unsorted"][1], False, what + " unsorted")
        if exact:
            assert got["sorted"][0].tobytes() == got["unsorted"][0].tobytes() == ref["offsets"].tobytes() and got["sorted"][1].tobytes() == ref["hits"].tobytes(), what
    elif family == "closest_point":
        point_check_exact(pkg, q, tris, ref, got["closest"], got["any"], what)
        if exact:
            assert got["closest"].tobytes() == ref["closest"].tobytes(), what
    elif family == "knn":
        for k, (h, c) in got.items():
            bf = ref if k == 32 else truncate(pkg, ref, k)
            knn_check_exact(pkg, q, tris, bf, h, c, f"{what} k {k}")
            if exact:
                assert h.tobytes() == bf["hits"].tobytes() and c.tobytes() == bf["counts"].astype(np.uint32).tobytes(), f"{what} k {k}"
    elif family == "radius":
        check_radius(q, tris, ref, got["sorted"][0], got["sorted"][1], True, what + " sorted")
        check_radius(q, tris, ref, got["unsorted"][0], got["unsorted"][1], False, what + " unsorted")
        if exact:
            assert got["sorted"][0].tobytes() == got["unsorted"][0].tobytes() == ref["offsets"].tobytes() and got["sorted"][1].tobytes() == ref["hits"].tobytes(), what
    else:
        assert got["total"] == int(ref["offsets"][-1]), what
        if got.get("guarded", True):                              # the C ABI call on guard-filled arrays: nothing written past the total either
            check_answer(got["offsets"], got["prims"], ref["offsets"], ref["prims"], what)
        else:                                                     # the binding returns exactly the total
            assert got["offsets"].tobytes() == ref["offsets"].tobytes() and len(got["prims"]) == got["total"], what
            assert sorted_slices(got["offsets"], got["prims"]).tobytes() == ref["prims"].tobytes(), what


def comparable(family, got):
    """the bytes of an answer that do not depend on the order of the walk"""
    if family in ("intersect", "closest_point"):
        return got["closest"].tobytes()
    if family == "knn":
        return b"".join(h.tobytes() + c.tobytes() for h, c in got.values())
    return got["sorted"][0].tobytes() + got["sorted"][1].tobytes()


# ---- trees ------------------------------------------------------------------------------------------------------------------------------------------------------

def built_tree(pkg, b):
    """the builder's tree as it is on the device now: (combined array, root, n)"""
    d = b.download()
    return combined(pkg, d["nodes"], d["leaves"]), int(d["root"]), int(b.result.n_leaves)


class Owned:
    """a layout-1 tree in caller-owned device arrays"""

    def __init__(self, pkg, ctx, nodes0, root, n, d_tris=None):
        inner, leaves = to_layout1(pkg, nodes0, n)
        self.pkg, self.n, self.root = pkg, n, root
        self.d_nodes, self.d_leaves = ctx.upload(inner), ctx.upload(leaves)
        r = pkg.Result()
        r.d_nodes = self.d_nodes.ptr; r.d_leaves = self.d_leaves.ptr; r.d_tris = d_tris; r.root = root; r.n_internal = n - 1; r.n_leaves = n; r.layout = 1
        self.result = r

    def tree(self):
        """downloaded from the arrays the queries read"""
        return combined(self.pkg, self.d_nodes.download(self.pkg.BVH2_NODE, self.n - 1), self.d_leaves.download(self.pkg.PRIMREF, self.n)), self.root, self.n

    def free(self):
        self.d_nodes.free(); self.d_leaves.free()


def assert_overflows(pkg, family, tree, q, what):
    """by the walk restatement on `tree`: the call holds at least 64 queries the short stack cannot serve, 64 it can, and both kinds in every wave"""
    lower, upper = needs(pkg, family, tree[0], tree[1], tree[2], q)
    assert_mixed(lower, upper, what)
    return lower, upper


# ---- 1. the layout-1 caterpillar in caller-owned arrays -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES)
def test_layout1_caterpillar_in_caller_owned_arrays(pkg, family):
    tris, inner, leaves, root, n, nodes0, q = caterpillar_case(pkg, family)      # (the left-first families get the chain_left form)
    assert n == 142
    ref = reference(pkg, family, q, tris)
    assert ref["well"].all()
    c = pkg.Context(0)
    try:
        c.reserve(n)
        d_tris = c.upload(tris)
        t = Owned(pkg, c, nodes0, root, n, d_tris.ptr)
        assert_overflows(pkg, family, t.tree(), q, f"caterpillar {family}")
        check(pkg, family, q, tris, ref, run(pkg, c, t.result, family, q), f"layout-1 caterpillar {family}")
        if family == "overlap":                                 # self mode takes d_boxes[i] AS primitive i's box
            grown = caterpillar_self_boxes(tris)
            self_off, self_prims = csr_of(overlap_brute_force(grown, tri_boxes(tris), self_pairs=True))
            assert self_off[1] == n - 1
            assert_overflows(pkg, family, t.tree(), grown, "caterpillar self")
            d_grown = c.upload(grown)
            rc, off, prims, total = overlap(pkg, c, t.result, (d_grown.ptr, n), mode=pkg.OVERLAP_SELF, guard=8)
            assert rc == 0 and total == int(self_off[-1])
            check_answer(off, prims, self_off, self_prims, "layout-1 caterpillar self")
            d_grown.free()
        t.free(); d_tris.free()
    finally:
        c.close()


def test_layout1_caterpillar_as_a_blas(pkg):
    tris, nodes0, root, n, inst, rays, aimed = caterpillar_scene(pkg)
    c, sc_ctx = pkg.Context(0), pkg.Context(0)
    try:
        c.reserve(n)
        d_tris = c.upload(tris)
        t = Owned(pkg, c, nodes0, root, n, d_tris.ptr)
        scene = pkg.Scene(sc_ctx).build(3, [pkg.Blas(t.result, pkg.BuildInput(0, 30, None, None, None, 0, 0))], inst)
        bf = scene_brute_force(pkg, rays, [tris], inst)
        assert bf["well"].all() and bf["hit"].sum() > len(rays) // 4
        # the BLAS's own pushes alone overflow the stack (the top level's entries come on top of them): each ray in the space of the instance it is aimed at
        assert_mixed(*scene_needs(pkg, t.tree(), inst, rays, aimed), "caterpillar as a BLAS")
        closest, anyhit = scene.intersect(rays, "closest"), scene.intersect(rays, "any")
        assert closest.tobytes() == bf["closest"].tobytes()
        assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"]).all() and scene_recompute(pkg, rays, [tris], inst, anyhit).all()
        scene.close(); t.free(); d_tris.free()
    finally:
        sc_ctx.close(); c.close()


# ---- 2. builder-made deep trees in the ctx's arena -----------------------------------------------------------------------------------------------------------

def binding_answers(pkg, b, family, q, **fmt):
    if family == "intersect":
        return {"closest": b.intersect(q, "closest", **fmt), "any": b.intersect(q, "any", **fmt)}
    if family == "intersect_all":
        off, hits = b.intersect_all(q, sorted=True, **fmt)
        assert b.intersect_all(q, count_only=True, **fmt).tobytes() == off.tobytes()
        return {"sorted": (off, hits), "unsorted": b.intersect_all(q, sorted=False, **fmt)}
    if family == "closest_point":
        return {"closest": b.closest_point(q, query="closest", **fmt), "any": b.closest_point(q, query="any", **fmt)}
    if family == "knn":
        return {k: b.knn(q, k, **fmt) for k in KS}
    if family == "radius":
        off, hits = b.radius_search(q, sorted=True, **fmt)
        assert b.radius_search(q, count_only=True, **fmt).tobytes() == off.tobytes()
        return {"sorted": (off, hits), "unsorted": b.radius_search(q, sorted=False, **fmt)}
    off, prims = b.overlap(q)
    return {"offsets": off, "prims": prims, "total": int(off[-1]), "guarded": False}


@pytest.mark.parametrize("algo", [2, 3])
def test_builder_made_deep_trees(pkg, orc, algo):
    tris = stairs(pkg); n = len(tris)
    c = pkg.Context(0)
    try:
        b = pkg.BUILDERS[algo]().build(c, tris)
        assert b.result.layout == 1 and b.result.d_nodes and b.result.d_leaves
        tree = built_tree(pkg, b)
        assert orc.validate_bvh2(tree[0][: n - 1].copy(), to_layout1(pkg, tree[0], n)[1], tree[1], n, 1) == 0
        report = []
        for family in FAMILIES:
            q, ref = stair_case(pkg, family)
            lower, upper = needs(pkg, family, tree[0], tree[1], n, q)
            report.append(f"{family} {int(lower.max())}")
            own = None
            if family in LEFT_FIRST and (lower > QUERY_STACK).sum() < 64:
                # the walk's need depends on which child is the left one: the same tree with the deeper child on the left, as caller-owned layout-1 arrays
                own = Owned(pkg, c, chain_left(tree[0], n - 1), tree[1], n, b.result.d_tris)
                assert_overflows(pkg, family, own.tree(), q, f"algo {algo} {family} chain left")
                check(pkg, family, q, tris, ref, run(pkg, c, own.result, family, q), f"staircase algo {algo} {family} chain left")
                own.free()
                continue
            assert_mixed(lower, upper, f"algo {algo} {family}")
            check(pkg, family, q, tris, ref, run(pkg, c, b.result, family, q), f"staircase algo {algo} {family} C ABI")
            assert built_tree(pkg, b)[0].tobytes() == tree[0].tobytes()        # (the tree the simulator saw is the tree that was queried)
            check(pkg, family, q, tris, ref, binding_answers(pkg, b, family, q), f"staircase algo {algo} {family} binding")
        print(f"algo {algo}: simulated need on the GPU tree: " + ", ".join(report))
    finally:
        c.close()


@pytest.mark.parametrize("algo", [2, 3])
def test_formats_on_deep_trees(pkg, algo):
    """one tree built FROM each triangle format and queried WITH it: the answers are the brute force's and byte-identical across the formats"""
    tris = stairs(pkg); n = len(tris)
    packed = np.ascontiguousarray(np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1).astype(F32).reshape(n, 9))
    uniq, inv = np.unique(packed.reshape(-1, 3), axis=0, return_inverse=True)
    idx = inv.reshape(-1).astype(np.uint32)
    c = pkg.Context(0)
    try:
        d_p, d_v, d_i = c.upload(packed), c.upload(np.ascontiguousarray(uniq.astype(F32))), c.upload(idx)
        B = pkg.BUILDERS[algo]
        forms = {
            "padded": (lambda: B().build(c, tris), None),
            "packed": (lambda: B().build_ex(c, n, tris=d_p, tri_format=pkg.TRI_PACKED36), pkg.BuildInput(pkg.TRI_PACKED36, 30, d_p.ptr, None, None, 0, 0)),
            "indexed": (lambda: B().build_ex(c, n, vertices=d_v, indices=d_i, n_vertices=len(uniq), tri_format=pkg.TRI_INDEXED),
                        pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, len(uniq), 0)),
        }
        per = {}
        for name, (build, inp) in forms.items():
            b = build()
            tree = built_tree(pkg, b)
            for family in ("intersect", "closest_point", "knn", "intersect_all"):
                q, ref = stair_case(pkg, family)
                assert_overflows(pkg, family, tree, q, f"algo {algo} {name} {family}")
                got = run(pkg, c, b.result, family, q, inp)
                check(pkg, family, q, tris, ref, got, f"staircase algo {algo} {name} {family}")
                per.setdefault(family, {})[name] = comparable(family, got)
        for family, by_form in per.items():
            assert by_form["padded"] == by_form["packed"] == by_form["indexed"], f"{family}: the formats differ"
        for x in (d_p, d_v, d_i):
            x.free()
    finally:
        c.close()


# ---- 3. the cached plan of the deep ctx-own tree ------------------------------------------------------------------------------------------------------------

def plan_answer(pkg, b, family, d_q, m):
    """the family through the binding with queries already on the device: no upload through the ctx, which would end the cached plan"""
    if family == "intersect":
        return {"closest": b.intersect(d_q, "closest", n_rays=m), "any": b.intersect(d_q, "any", n_rays=m)}
    if family == "closest_point":
        return {"closest": b.closest_point(d_q, query="closest", n_points=m), "any": b.closest_point(d_q, query="any", n_points=m)}
    off, prims = b.overlap(d_q, n=m, capacity=200 * m)
    return {"offsets": off, "prims": prims, "total": int(off[-1]), "guarded": False}


@pytest.mark.parametrize("family", ["intersect", "closest_point", "overlap"])
@pytest.mark.parametrize("algo", [2, 3])
def test_cached_plan_follows_the_deep_tree(pkg, algo, family):
    """query (the plan is made and kept), refit, refit_subset, optimize (topology changes, parent[] maintained), rebuilds of the same n with the unrotated
    staircase and with the other builder: after every step the answers are the brute force's of the current triangles, the queried tree needs the stackless
    pass, and k_refit_plan ran exactly where the plan had to be renewed.  Everything the steps read is put on the device before the first query: an upload through the ctx ends the cached plan."""
    meshes, dirty, qs, refs = plan_case(pkg, algo, family)     # (tests/test_deep_trees.py asserts every leg's mix on the CPU restatements too)
    a, moved, moved2, perm = meshes["built"], meshes["refit"], meshes["subset"], meshes["permuted"]
    n = len(a)
    other = 5 - algo
    c = pkg.Context(0)
    try:
        d_q = {name: c.upload(q) for name, q in qs.items()}
        d_moved2, d_dirty, d_perm = c.upload(moved2), c.upload(dirty), c.upload(perm)
        b = pkg.BUILDERS[algo]().build(c, a)

        def leg(name, builder, plan_renewed):
            tree = built_tree(pkg, builder)
            assert_overflows(pkg, family, tree, qs[name], f"algo {algo} {family} {name}")
            c.set_profiling(2)
            got = plan_answer(pkg, builder, family, d_q[name], M_PLAN)
            kt = c.kernel_times()
            c.set_profiling(0)
            assert ("k_refit_plan" in kt) == plan_renewed, f"{name}: {sorted(kt)}"
            assert refs[name]["well"].mean() >= 0.99
            check(pkg, family, qs[name], meshes[name], refs[name], got, f"algo {algo} {family} {name}")
        leg("built", b, True)
        b.refit(moved)
        leg("refit", b, False)
        b.refit_subset(d_dirty, n_dirty=len(dirty), tris=d_moved2)
        leg("subset", b, False)
        before = built_tree(pkg, b)[0]
        b.optimize(1)
        after = built_tree(pkg, b)[0]
        rewritten = int((after["left"][: n - 1] != before["left"][: n - 1]).sum() + (after["right"][: n - 1] != before["right"][: n - 1]).sum())
        assert rewritten > 0, "bvh_optimize changed nothing: the leg tests nothing"     # (a plan that did not follow the new links would be walked wrong)
        leg("optimized", b, False)
        before = built_tree(pkg, b)[0]
        b.build(c, d_perm, on_device=True, n=n)                  # the same n, another deep tree: the plan must not survive
        after = built_tree(pkg, b)[0]
        assert after["left"][: n - 1].tobytes() != before["left"][: n - 1].tobytes() or after["right"][: n - 1].tobytes() != before["right"][: n - 1].tobytes()
        leg("permuted", b, True)
        b2 = pkg.BUILDERS[other]().build(c, a)
        leg("other builder", b2, True)
        for x in list(d_q.values()) + [d_moved2, d_dirty, d_perm]:
            x.free()
    finally:
        c.close()


# ---- 4. more queries than the deep kernels' grid covers at once ---------------------------------------------------------------------------------------------

N_QUIET, N_DEEP = 65_536, 1024


def expand(pkg, family, ref, src, tris):
    """the brute force of the distinct queries -> that of the whole call (query i is distinct query src[i])"""
    if family in ("intersect", "closest_point"):
        return {"closest": ref["closest"][src], "hit": ref["hit"][src], "well": ref["well"][src]}
    if family == "knn":
        return {k: ref[k][src] for k in ("hits", "counts", "well", "entry_well")}
    counts = np.diff(ref["offsets"].astype(np.int64))[src]
    off = np.zeros(len(src) + 1, dtype=np.uint32); off[1:] = np.cumsum(counts)
    key = "prims" if family == "overlap" else "hits"
    starts = ref["offsets"].astype(np.int64)[src]
    take = np.concatenate([np.arange(s, s + k) for s, k in zip(starts[counts > 0], counts[counts > 0])]) if counts.any() else np.zeros(0, dtype=np.int64)
    out = {"offsets": off, key: ref[key][take], "well": ref["well"][src]}
    if family == "intersect_all":
        out["n_acc"] = ref["n_acc"][src]
    if family == "radius":
        out["counts"] = ref["counts"][src]
    return out


def assert_quiet_bytes(pkg, family, got, ref, lo, hi):
    """the records of the quiet queries [lo, hi) byte for byte: miss records, empty lists, empty slices"""
    if family in ("intersect", "closest_point"):
        assert got["closest"][lo:hi].tobytes() == got["any"][lo:hi].tobytes() == ref["closest"][lo:hi].tobytes()
        assert (got["closest"]["prim"][lo:hi] == pkg.INVALID).all()
    elif family == "knn":
        for k, (h, c) in got.items():
            assert h[lo:hi].tobytes() == np.ascontiguousarray(ref["hits"][lo:hi, :k]).tobytes() and not c[lo:hi].any() and (h["prim"][lo:hi] == pkg.INVALID).all()
    else:
        offs = [got["offsets"]] if family == "overlap" else [got["sorted"][0], got["unsorted"][0]]
        for off in offs:
            assert off[lo:hi + 1].tobytes() == ref["offsets"][lo:hi + 1].tobytes() and off[lo] == off[hi]


@pytest.mark.parametrize("order", ["deep last", "deep first"])
@pytest.mark.parametrize("family", FAMILIES)
def test_more_queries_than_the_deep_grid(pkg, family, order):
    """66 560 queries: the deep kernels' grid is capped at 1024 workgroups of 64, so the 1024 overflowing queries at one end of the call are reached by the
    second trip of the grid-stride loop when they come last, and by the first when they come first.  The 65 536 others (256 distinct ones, repeated) neither
    hit nor overflow; their miss records and empty slices are compared byte for byte like the rest."""
    tris = stairs(pkg); n = len(tris)
    deep_q, deep_ref = stair_case(pkg, family, N_DEEP)
    quiet = quiet_queries(pkg, family, tris, 256)
    distinct = np.concatenate([deep_q, quiet])
    ref_d = reference(pkg, family, distinct, tris)
    assert ref_d["well"][N_DEEP:].all()
    if family == "knn":
        assert (ref_d["counts"][N_DEEP:] == 0).all()
    elif family in ("intersect", "closest_point"):
        assert not ref_d["hit"][N_DEEP:].any()
    else:
        assert (np.diff(ref_d["offsets"].astype(np.int64))[N_DEEP:] == 0).all()
    quiet_src = N_DEEP + np.arange(N_QUIET) % 256
    src = np.concatenate([quiet_src, np.arange(N_DEEP)]) if order == "deep last" else np.concatenate([np.arange(N_DEEP), quiet_src])
    q = distinct[src]
    ref = expand(pkg, family, ref_d, src, tris)
    assert len(q) == 66_560 and ref["well"].mean() >= 0.99
    c = pkg.Context(0)
    try:
        b = pkg.PLOCNew().build(c, tris)
        tree = built_tree(pkg, b)
        lower, upper = needs(pkg, family, tree[0], tree[1], n, distinct)
        own = None
        if family in LEFT_FIRST and (lower[:N_DEEP] > QUERY_STACK).sum() < 64:
            own = Owned(pkg, c, chain_left(tree[0], n - 1), tree[1], n, b.result.d_tris)
            tree = own.tree()
            lower, upper = needs(pkg, family, tree[0], tree[1], n, distinct)
        lower, upper = lower[src], upper[src]
        far = slice(N_QUIET, None) if order == "deep last" else slice(0, N_DEEP)
        near = slice(0, N_QUIET) if order == "deep last" else slice(N_DEEP, None)
        assert (lower[far] > QUERY_STACK).sum() >= 256 and (upper[near] == 0).all(), (int(lower.max()), int(upper[near].max()))
        got = run(pkg, c, own.result if own else b.result, family, q)
        check(pkg, family, q, tris, ref, got, f"{family} {order}")
        assert_quiet_bytes(pkg, family, got, ref, near.start or 0, near.stop or len(q))
        if own:
            own.free()
    finally:
        c.close()


# ---- 5. scenes ----------------------------------------------------------------------------------------------------------------------------------------------------

def download_tlas(pkg, ctx, t):
    nodes = np.empty(t.n_leaves - 1, dtype=pkg.BVH2_NODE); leaves = np.empty(t.n_leaves, dtype=pkg.PRIMREF)
    assert pkg.lib().bvh_download(ctx.handle, C.byref(t), nodes.ctypes.data, leaves.ctypes.data, None, None, None) == 0
    return combined(pkg, nodes, leaves), int(t.root), int(t.n_leaves)


@pytest.mark.parametrize("tlas_algo", [2, 3])
def test_deep_top_level_tree(pkg, tlas_algo):
    small = mesh(pkg, "uniform_64")
    inst, rays = tlas_scene(pkg, tlas_algo)
    m = len(rays)
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blas = bl.add(3, small)
        scene = pkg.Scene(sc_ctx).build(tlas_algo, [blas], inst)
        t = scene.tlas()
        assert t.n_leaves == 180 and t.layout == 1
        tree = download_tlas(pkg, sc_ctx, t)
        blas_tree = built_tree(pkg, blas)
        # lower: the top level's pushes before the first instance is entered; upper: its static bound plus the bottom-level tree's height
        lower, upper = scene_needs(pkg, blas_tree, inst, rays, None, top=tree, blas_bound=height(blas_tree[0], blas_tree[1], blas_tree[2] - 1))
        print(f"tlas algo {tlas_algo}: near-first need at the top level up to {lower.max()}")
        assert_mixed(lower, upper, f"tlas algo {tlas_algo}")
        bf = scene_brute_force(pkg, rays, [small], inst)
        assert bf["well"].mean() >= 0.99 and bf["hit"].sum() > m // 4
        closest, anyhit = scene.intersect(rays, "closest"), scene.intersect(rays, "any")
        w = bf["well"]
        assert closest[w].tobytes() == bf["closest"][w].tobytes()
        assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"])[w].all()
        assert scene_recompute(pkg, rays, [small], inst, closest).all() and scene_recompute(pkg, rays, [small], inst, anyhit).all()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


def test_deep_layout1_blas_under_instances(pkg):
    """the staircase built by PLOCNew (layout 1, in its own ctx's arena) under five translated instances; every overflowing ray starts at its instance's
    origin, which maps to the BLAS's origin exactly, so the BLAS's own pushes overflow the stack whatever the top level adds"""
    tris, inst, rays, aimed = staircase_scene(pkg)             # (tests/test_deep_trees.py asserts the mix on the oracle's tree too)
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blas = bl.add(2, tris)
        assert blas.result.layout == 1
        scene = pkg.Scene(sc_ctx).build(3, [blas], inst)
        tree = built_tree(pkg, blas)
        assert_mixed(*scene_needs(pkg, tree, inst, rays, aimed), "staircase as a BLAS")
        bf = scene_brute_force(pkg, rays, [tris], inst)
        assert bf["well"].mean() >= 0.99 and bf["hit"][::2].all()
        assert len(set(bf["closest"]["instance"][::2].tolist())) == len(STAIR_SHIFTS)
        closest, anyhit = scene.intersect(rays, "closest"), scene.intersect(rays, "any")
        wl = bf["well"]
        assert closest[wl].tobytes() == bf["closest"][wl].tobytes()
        assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"])[wl].all()
        assert scene_recompute(pkg, rays, [tris], inst, closest).all() and scene_recompute(pkg, rays, [tris], inst, anyhit).all()
        scene.close()
    finally:
        bl.close(); sc_ctx.close()


# ---- 6. the conservative box tests at other scales -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SCALES))
def test_other_scales(pkg, name):
    """uniform_1000 unchanged, translated by 1e6, scaled by 1e-12 and by 1e12, with the rays (origins, tmin, tmax) and the points (and radii) mapped alike: the
    growth of the boxes is relative to their coordinates, so the answers stay the brute force's.  tests/test_deep_trees.py asserts on the CPU that all four
    sets, the closest-point ones included, are well-conditioned with the scale factors 1e-12 and 1e12 as they stand."""
    tris, rays, bf, pts, pbf = scale_reference(pkg, name)
    c = pkg.Context(0)
    try:
        for algo in (0, 1, 2, 3):
            b = pkg.BUILDERS[algo]().build(c, tris)
            ray_check_exact(pkg, rays, tris, bf, b.intersect(rays, "closest"), b.intersect(rays, "any"), f"{name} algo {algo} rays")
            point_check_exact(pkg, pts, tris, pbf, b.closest_point(pts), b.closest_point(pts, query="any"), f"{name} algo {algo} points")
    finally:
        c.close()
