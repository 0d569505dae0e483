"""The seven query entry points on the GPU against non-finite, huge, far-offset and denormal meshes and queries with infinite, huge, denormal, -0 and zero
components (inputs and their premises: tests/test_query_extremes.py).  Every mesh is built by all four builders, the layout-1 trees also as their layout-0 copy;
the answers go through the existing checkers unchanged: bit-equal to the numpy brute forces on the well-conditioned queries, and on every query the
unconditional guarantees (each record an accepted candidate of its primitive, nothing below the truth, sets subsets of the truth, nothing written past the
total).  What this pins that the near-origin unit meshes of the other files cannot: the (key, prim) tie rule (offset_2p20, huge_offset, the all-inf distances),
NaN-vertex rejection, and traversal through boxes with planes at +-inf and +-FLT_MAX."""
import numpy as np
import pytest

from test_gpu_knn import check_exact as check_knn
from test_gpu_knn import knn
from test_gpu_multihit import all_hits
from test_gpu_overlap import check_answer, overlap
from test_gpu_point_query import check_exact as check_points
from test_gpu_point_query import query as closest_query
from test_gpu_query import check_exact as check_rays
from test_gpu_query import lbvh_result, query
from test_gpu_radius import search
from test_gpu_scene import Blases, root_boxes
from test_gpu_scene import check_exact as check_scene
from test_knn import below as knn_below
from test_knn import recompute_knn
from test_multihit import HITS_SORTED, check_all_hits, slice_rays
from test_overlap import csr_of, leaf_boxes_of, overlap_brute_force
from test_point_query import below as point_below
from test_point_query import recompute_points
from test_query_extremes import (KS, MESH_NAMES, POINT_EXACT, POINT_MESHES, RAY_MESHES, SCENE_BLASES, SPECIAL_MESHES, extreme_boxes, mesh, point_reference,
                                 points_of, ray_reference, rays_of, replaced, scene_instances, scene_rays)
from test_radius import RADIUS_SORTED, check_radius, host_sort, slice_queries
from test_scene import scene_brute_force

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


def trees_of(pkg, ctx, tris, algo):
    """(label, builder, result) of one builder's tree, a layout-1 tree also as bvh_to_lbvh_layout's copy"""
    b = pkg.BUILDERS[algo]().build(ctx, tris)
    keep = []
    try:
        yield f"algo {algo} as built", b, b.result
        if b.result.layout == 1:
            yield f"algo {algo} lbvh layout", b, lbvh_result(pkg, ctx, b, keep)
    finally:
        for k in keep:
            k.free()


def each_tree(pkg, ctx, tris):
    """(algo, label, builder, result) of all four builders; one tree lives at a time"""
    for algo in (0, 1, 2, 3):
        for label, b, res in trees_of(pkg, ctx, tris, algo):
            yield algo, label, b, res


@pytest.mark.parametrize("name", RAY_MESHES)
def test_ray_families(pkg, ctx, name):
    """bvh_intersect (CLOSEST, ANY) and bvh_intersect_all (sorted, unsorted)"""
    tris = mesh(pkg, name)
    rays, fam, bf, ref = ray_reference(pkg, name)
    well = bf["well"]
    wrec = well[slice_rays(ref["offsets"])]
    per = {}
    for algo, label, b, res in each_tree(pkg, ctx, tris):
        what = f"{name} {label}"
        c, a = query(pkg, ctx, res, rays, pkg.QUERY_CLOSEST), query(pkg, ctx, res, rays, pkg.QUERY_ANY)
        check_rays(pkg, rays, tris, bf, c, a, what)
        off, hits = all_hits(pkg, ctx, res, rays, HITS_SORTED)
        check_all_hits(rays, tris, ref, off, hits, True, what + " sorted")
        uoff, uhits = all_hits(pkg, ctx, res, rays, 0)
        assert uoff.tobytes() == off.tobytes(), f"{what}: sorted and unsorted calls count differently"
        check_all_hits(rays, tris, ref, uoff, uhits, False, what + " unsorted")
        has = np.diff(off.astype(np.int64)) > 0                       # a sorted slice starts with the closest hit
        assert (has == (c["prim"] != pkg.INVALID))[well].all() and hits[off[:-1][has & well]].tobytes() == c[has & well].tobytes(), what
        per.setdefault(algo, (c, off, hits))
    for algo in (1, 2, 3):                                            # one answer on the well-conditioned rays, whatever the builder
        c, off, hits = per[algo]
        assert c[well].tobytes() == per[0][0][well].tobytes(), f"{name}: builders {algo} and 0 differ"
        assert hits[well[slice_rays(off)]].tobytes() == per[0][2][well[slice_rays(per[0][1])]].tobytes() == ref["hits"][wrec].tobytes()
    if name in ("denormals", "scale_2p60"):                           # every product underflows / the cubic terms overflow: every ray misses
        assert all(int(off[-1]) == 0 and (c["prim"] == pkg.INVALID).all() for c, off, _ in per.values())


def points_unconditionally(pkg, pts, tris, bf, closest, anyhit, what):
    assert recompute_points(pkg, pts, tris, closest).all(), f"{what}: a closest record is not an accepted candidate of its prim (or not the miss record)"
    assert recompute_points(pkg, pts, tris, anyhit).all(), f"{what}: an any record is not an accepted candidate of its prim (or not the miss record)"
    assert not point_below(pkg, closest, bf["closest"]).any(), f"{what}: closest below the brute force"


def point_answers(pkg, ctx, res, pts):
    """every point family on one tree: (closest, any, {k: (lists, counts)}, sorted (offsets, hits), unsorted (offsets, hits))"""
    c, a = closest_query(pkg, ctx, res, pts, pkg.QUERY_CLOSEST), closest_query(pkg, ctx, res, pts, pkg.QUERY_ANY)
    return c, a, {k: knn(pkg, ctx, res, pts, k) for k in KS}, search(pkg, ctx, res, pts, RADIUS_SORTED), search(pkg, ctx, res, pts, 0)


_BUILDER0 = {}                                                        # builder 0's answers per mesh: what builders 1 to 3 must equal


def builder0_answers(pkg, ctx, name):
    if name not in _BUILDER0:
        b = pkg.BUILDERS[0]().build(ctx, mesh(pkg, name))
        _BUILDER0[name] = point_answers(pkg, ctx, b.result, points_of(pkg, name)[0])
    return _BUILDER0[name]


@pytest.mark.parametrize("algo", [0, 1, 2, 3])
@pytest.mark.parametrize("name", POINT_MESHES)
def test_point_families(pkg, ctx, name, algo):
    """bvh_closest_point (CLOSEST, ANY), bvh_knn (k = 1, 8, 32) and bvh_radius_search (sorted, unsorted), and the three against each other.  One builder per
    case: a sorted fill of the 4000-record slices (an infinite radius, or r2 = inf) is quadratic in the slice and takes about a second per tree."""
    tris = mesh(pkg, name)
    pts, fam, bf, kbf, rad = point_reference(pkg, name)
    exact = name in POINT_EXACT
    if not exact:                                                     # only the unconditional guarantees: no query counts as well-conditioned
        rad = dict(rad, well=np.zeros(len(pts), dtype=bool))
        print(f"{name}: well-conditioned share of the point families {bf['well'].mean():.3f}")
    mine = None
    for label, b, res in trees_of(pkg, ctx, tris, algo):
        what = f"{name} {label}"
        ans = c, a, lists, (off, hits), (uoff, uhits) = point_answers(pkg, ctx, res, pts)
        if exact:
            check_points(pkg, pts, tris, bf, c, a, what)
        else:
            points_unconditionally(pkg, pts, tris, bf, c, a, what)
        for k in KS:
            h, cnt = lists[k]
            if exact:
                check_knn(pkg, pts, tris, kbf[k], h, cnt, f"{what} k {k}")
            else:
                assert recompute_knn(pkg, pts, tris, h, cnt).all(), f"{what} k {k}: a list does not recompute"
                assert not knn_below(pkg, h, kbf[k]["hits"]).any(), f"{what} k {k}: a list below the brute force"
        h1, c1 = lists[1]                                             # k = 1 is bvh_closest_point's (dist2, prim), bit for bit
        assert h1["dist2"][:, 0].tobytes() == c["dist2"].tobytes() and h1["prim"][:, 0].tobytes() == c["prim"].tobytes(), f"{what}: k = 1 != bvh_closest_point"
        assert (c1 == (c["prim"] != pkg.INVALID)).all()
        check_radius(pts, tris, rad, off, hits, True, what + " sorted")
        assert uoff.tobytes() == off.tobytes(), f"{what}: sorted and unsorted calls count differently"
        check_radius(pts, tris, rad, uoff, uhits, False, what + " unsorted")
        h8, c8 = lists[8]                                             # the first min(8, count) sorted records are the kNN list
        take = np.minimum(np.diff(off.astype(np.int64)), 8)
        assert (take == c8).all(), f"{what}: min(count, 8) != bvh_knn's d_counts"
        head = np.arange(8)[None] < take[:, None]
        assert hits[(off[:-1].astype(np.int64)[:, None] + np.arange(8)[None])[head]].tobytes() == h8[head].tobytes(), f"{what}: sorted slices do not start with the kNN list"
        mine = mine or ans
    if algo == 0:
        _BUILDER0.setdefault(name, mine)
    elif exact:                                                       # one answer on the well-conditioned queries, whatever the builder
        well = bf["well"] & kbf[32]["well"] & rad["well"]
        c0, _, lists0, (off0, hits0), _ = builder0_answers(pkg, ctx, name)
        c, _, lists, (off, hits), _ = mine
        assert c[well].tobytes() == c0[well].tobytes(), f"{name}: builders {algo} and 0 differ"
        assert all(lists[k][0][well].tobytes() == lists0[k][0][well].tobytes() for k in KS), f"{name}: builders {algo} and 0 differ"
        assert hits[well[slice_queries(off)]].tobytes() == hits0[well[slice_queries(off0)]].tobytes(), f"{name}: builders {algo} and 0 differ"


@pytest.mark.parametrize("name", MESH_NAMES)
def test_overlap(pkg, ctx, name):
    """bvh_overlap, boxes mode and BVH_OVERLAP_SELF, against the brute force on the leaf boxes the tree holds (stage E's: a NaN coordinate dropped, the planes
    clamped; never the NaN-propagating numpy min / max)"""
    tris = mesh(pkg, name); n = len(tris)
    first = None
    for algo, label, b, res in each_tree(pkg, ctx, tris):
        what = f"{name} {label}"
        if first is None:
            d = b.download()
            leaf = leaf_boxes_of(d["nodes"], d["leaves"], n, b.result.layout)
            boxes = extreme_boxes(leaf, 3000 + MESH_NAMES.index(name), skip=replaced(pkg, name) if name in SPECIAL_MESHES else None)
            ref = csr_of(overlap_brute_force(boxes, leaf))
            self_ref = csr_of(overlap_brute_force(leaf, leaf, self_pairs=True))
            print(f"{name}: {ref[0][-1]} results of {len(boxes)} boxes, {self_ref[0][-1]} overlapping pairs")
            first = (leaf, boxes, ref, self_ref)
        leaf, boxes, ref, self_ref = first
        if label.endswith("as built"):                                # every builder holds stage E's boxes
            d = b.download()
            assert leaf_boxes_of(d["nodes"], d["leaves"], n, b.result.layout).tobytes() == leaf.tobytes(), f"{what}: leaf boxes differ from builder 0's"
        rc, off, prims, total = overlap(pkg, ctx, res, boxes, guard=16)
        assert rc == 0 and total == int(ref[0][-1]), what
        check_answer(off, prims, ref[0], ref[1], what)
        rc, off, prims, total = overlap(pkg, ctx, res, (b.result.d_prim_aabbs, n), mode=pkg.OVERLAP_SELF, guard=8)
        assert rc == 0 and total == int(self_ref[0][-1]), what
        check_answer(off, prims, self_ref[0], self_ref[1], what + " self")
        assert (prims[:total] > np.repeat(np.arange(n), np.diff(off.astype(np.int64)))).all()


@pytest.mark.parametrize("name", ["nan_vertex", "ff_filled_triangle"])
def test_formats_give_identical_answers(pkg, ctx, name):
    """PADDED64, PACKED36 and INDEXED input: byte-identical answers of every family (the pattern of test_gpu_query.test_formats_give_identical_hits; the vertices
    are shuffled instead of deduplicated: a NaN vertex equals nothing)"""
    tris = mesh(pkg, name); n = len(tris)
    rays, _ = rays_of(pkg, name)
    pts, _ = points_of(pkg, name)
    short = pts[~np.isinf(pts["radius"])]
    b = pkg.HPLOC().build(ctx, tris)
    packed = np.ascontiguousarray(np.stack([tris["v1"], tris["v2"], tris["v3"]], axis=1).astype(np.float32).reshape(n, 9))
    idx = np.random.default_rng(7).permutation(3 * n).astype(np.uint32)
    verts = np.zeros((3 * n, 3), dtype=np.float32)
    verts.view(np.uint32)[idx] = packed.reshape(-1, 3).view(np.uint32)       # (bit copies: the NaN payloads survive)
    d_p, d_v, d_i = ctx.upload(packed), ctx.upload(verts), ctx.upload(idx)
    try:
        inputs = [None, pkg.BuildInput(pkg.TRI_PACKED36, 30, d_p.ptr, None, None, 0, 0), pkg.BuildInput(pkg.TRI_INDEXED, 30, None, d_v.ptr, d_i.ptr, 3 * n, 0)]
        answers = []
        for inp in inputs:
            got = [query(pkg, ctx, b.result, rays, kind, inp) for kind in (pkg.QUERY_CLOSEST, pkg.QUERY_ANY)]
            got += list(all_hits(pkg, ctx, b.result, rays, HITS_SORTED, inp))
            got += [closest_query(pkg, ctx, b.result, pts, kind, inp) for kind in (pkg.QUERY_CLOSEST, pkg.QUERY_ANY)]
            got += list(knn(pkg, ctx, b.result, pts, 8, inp))
            got += list(search(pkg, ctx, b.result, short, RADIUS_SORTED, inp))      # (sorted fills of the short slices; the 4000-record ones host-sorted)
            off, hits = search(pkg, ctx, b.result, pts, 0, inp)
            got += [off, host_sort(off, hits)]
            answers.append(b"".join(x.tobytes() for x in got))
        assert answers[0] == answers[1] == answers[2]
        assert len(answers[0]) > (len(rays) + len(pts)) * 16
    finally:
        for x in (d_p, d_v, d_i):
            x.free()


def test_scene_with_non_finite_blases(pkg):
    """bvh_scene_intersect over BLASes with a NaN vertex, an infinite vertex and a huge triangle (root boxes with planes at +inf and +-3e38), instances placed by
    exact transforms, one of them 2^20 away; top-level builders 0 and 1"""
    meshes = [mesh(pkg, name) for name in SCENE_BLASES]
    inst = scene_instances(pkg)
    rays = scene_rays(pkg, inst)
    bl = Blases(pkg)
    sc_ctx = pkg.Context(0)
    try:
        blases = [bl.add(algo, meshes[algo]) for algo in range(4)]
        bf = scene_brute_force(pkg, rays, meshes, inst, root_boxes(pkg, blases))
        assert bf["hit"].mean() >= 0.5
        outs = []
        for tl in (0, 1):
            scene = pkg.Scene(sc_ctx).build(tl, blases, inst)
            closest, anyhit = scene.intersect(rays, "closest"), scene.intersect(rays, "any")
            check_scene(pkg, rays, meshes, inst, bf, closest, anyhit, f"top-level builder {tl}")
            outs.append(closest)
            scene.close()
        assert outs[0][bf["well"]].tobytes() == outs[1][bf["well"]].tobytes()
    finally:
        bl.close(); sc_ctx.close()
