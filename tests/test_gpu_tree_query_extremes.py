"""The five tree-level queries that came after tests/test_gpu_query_extremes.py — bvh_intersect_tris, bvh_closest_tris, bvh_radius_tris, bvh_winding_prepare /
bvh_winding_number and bvh_cull — on the GPU against that file's twelve meshes: non-finite, huge, far-offset and denormal vertices, trees whose boxes have
planes at +-inf and +-3e38 or are the reset box of an all-NaN triangle (inputs, brute forces and their premises: tests/test_tree_query_extremes.py).  Every
mesh is built by all four builders, the layout-1 trees also as their layout-0 copy.  On every query of every mesh, with no cap: each record is an accepted
candidate of its primitive with bit-equal fields, nothing lies below the brute force, sets are subsets of the brute force's, misses are the exact miss record,
a primitive appears once per slice, count-only, unsorted and sorted calls agree, nothing is written past the total, a capacity one short fills nothing.
What is NOT run on every query of every tree, all of it in bvh_radius_tris: the SORTED fill of an answer with a slice longer than 500 records (an infinite
r2, and every radius >= 0 on `denormals`: the insertion sort is quadratic in the slice — 0.2 s per call at 1000 records, 3 s at 4000, however few queries
the call has) runs on all queries on builder 0's tree, at every such radius (+inf and 1e30 among them), and at radius +inf on every tenth query on the
as-built trees of builders 1 to 3, whose visit order differs; not on the layout-0 copies, which have their tree's topology and visit order (the self mode of
`denormals`, 999 records in the longest slice: sorted on builder 0's tree).  For such
answers the fill between guard words is unsorted.  The count, the unsorted fill, the guard words and the capacity one short run on every query of every tree
at every radius, and so does the sorted fill of every answer with shorter slices.
Where the contract says exact — every crossing query, the well-conditioned distance queries of every mesh but `denormals`, every cull volume none of whose
plane values on that tree is a NaN — the answer is the brute force's, byte for byte, whatever the builder.  The winding number answers the canonical NaN
exactly where the header's formula does and lies within the existing bound of tests/test_gpu_winding.py elsewhere."""
import numpy as np
import pytest

from test_closest_tris import below, recompute_tris
from test_cull import Tree, by_prim, group_walk
from test_gpu_closest_tris import raw as closest_raw
from test_gpu_cull import AUTO, GROUP, LANE, check_answer as check_cull, run_cull, untouched
from test_gpu_intersect_tris import GUARD, DeviceMesh, tris_call
from test_gpu_query_extremes import each_tree
from test_gpu_radius_tris import call as radius_call
from test_gpu_radius_tris import host_sorted, search
from test_gpu_winding import TOL_FACTOR, TOL_FLOOR, prepare, winding
from test_gpu_winding import trees_of as trees_with_nodes
from test_overlap import sorted_slices
from test_query_extremes import FRAMES, MESH_NAMES, mesh
from test_radius_tris import accepted_matrix, recompute_records
from test_tree_query_extremes import (N_VOLUMES, PLANE_COUNTS, TRI_EXACT, nan_free, pairs_of, self_reference, tri_reference, volumes_of, walk_host_sum64,
                                      wind_reference)
from test_winding import WIND_NAN_BITS, moments_host, walk_host

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
F64 = np.float64
HEAVY = 100_000                                                     # records above which an answer is compared as a dense matrix (records_against_pairs)
LONG = 500                                                          # slice length above which a sorted fill (quadratic in the slice) is not run on every tree


# ---- bvh_intersect_tris ---------------------------------------------------------------------------------------------------------------------------------------------

def crossing_checks(pkg, ctx, res, queries, mode, ref, what):
    """count, fill with the exact capacity between guard words, and a capacity one short: the whole answer equals the brute force (every record a crossing
    pair, no pair missing, no primitive twice), nothing is written past the total, and one record short the total is reported and nothing filled"""
    ref_off, ref_prims = ref
    total = int(ref_off[-1])
    rc, off, prims, t = tris_call(pkg, ctx, res, queries, mode=mode, guard=8)
    assert rc == 0 and t == total and off.tobytes() == ref_off.tobytes(), f"{what}: {t} pairs, the brute force has {total}"
    assert sorted_slices(off, prims[:total]).tobytes() == ref_prims.tobytes(), f"{what}: another set"
    assert (prims[total:] == GUARD).all(), f"{what}: d_prims written past the total"
    if total:
        rc, off, prims, t = tris_call(pkg, ctx, res, queries, mode=mode, capacity=total - 1, guard=8)
        assert rc == 0 and t == total and off.tobytes() == ref_off.tobytes() and (prims == GUARD).all(), f"{what}: one record short"


@pytest.mark.parametrize("name", MESH_NAMES)
def test_intersect_tris(pkg, ctx, name):
    """exact on every query of every mesh (the completeness condition holds for every build), BVH_TRIS_SELF on the four frames"""
    tris = mesh(pkg, name); n = len(tris)
    q, fam, per, (sets, ref), _ = tri_reference(pkg, name)
    dm = DeviceMesh(pkg, ctx, q)
    try:
        for algo, label, b, res in each_tree(pkg, ctx, tris):
            crossing_checks(pkg, ctx, res, dm, 0, ref, f"{name} {label}")
            if name in FRAMES:
                crossing_checks(pkg, ctx, res, n, 1, self_reference(pkg, name)[0][1], f"{name} {label} self")
    finally:
        dm.free()
    print(f"{name}: {int(ref[0][-1])} crossing pairs of {len(q)} query triangles")


# ---- bvh_closest_tris and bvh_radius_tris ----------------------------------------------------------------------------------------------------------------------------

def closest_unconditionally(pkg, q, tris, radius, bf, closest, anyhit, what):
    """test_gpu_closest_tris.check_exact without the 99 % floor: bit-equal on the well-conditioned queries, and on every query the unconditional guarantees"""
    well, ref = bf["well"], bf["closest"]
    diff = (closest.view(np.uint8).reshape(-1, 16) != ref.view(np.uint8).reshape(-1, 16)).any(axis=1)
    assert not (diff & well).any(), f"{what}: closest differs on {np.count_nonzero(diff & well)} well-conditioned queries (first {np.nonzero(diff & well)[0][:6]})"
    assert ((anyhit["prim"] != pkg.INVALID) == bf["hit"])[well].all(), f"{what}: any hit/miss differs"
    assert recompute_tris(pkg, q, tris, radius, closest).all(), f"{what}: a closest record is not an accepted candidate of its prim (or not the miss record)"
    assert recompute_tris(pkg, q, tris, radius, anyhit).all(), f"{what}: an any record is not an accepted candidate of its prim (or not the miss record)"
    assert not below(pkg, closest, ref).any(), f"{what}: closest below the brute force"
    if not bf["hit"].any():                                           # a negative or NaN radius, NaN queries: nothing but miss records
        assert (closest["prim"] == pkg.INVALID).all() and (anyhit["prim"] == pkg.INVALID).all(), what


def slice_rows(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))


def dense_key(dist2, feature):
    return (dist2.view(np.uint32).astype(np.uint64) << np.uint64(8)) | feature.astype(np.uint64)


NO_RECORD = np.uint64(1) << np.uint64(63)


def records_against_pairs(pkg, q, tris, radius, pairs, bf, off, hits, sorted_, what, self_pairs=False, skip_shared=False):
    """radius_unconditionally for the long answers (every triangle in every slice: an infinite r2, the denormal frame), against the pair matrix the brute force
    was made from instead of 15 terms per record again, and without a sort on the host: the records are scattered into a dense (query, prim) matrix of
    (dist2 bits, feature) and compared with the matrix of the contract's accepted pairs (test_radius_tris.accepted_matrix: dist2 <= r2 on live queries, j > i
    and no shared vertex in self mode).  No prim twice in a slice; every record an accepted pair with bit-equal dist2, the same feature and reserved 0 — so
    every slice is a subset of the brute force's —; the well-conditioned queries' rows equal the brute force's; a sorted slice ascends in (dist2, prim).
    Returns the dense matrix"""
    d2, feat = pairs
    m, n = d2.shape
    o = off.astype(np.int64)
    assert len(o) == m + 1 and o[0] == 0 and (np.diff(o) >= 0).all() and o[-1] == len(hits), f"{what}: the offsets are not a scan that ends at the number of records"
    rows = slice_rows(off); pr = hits["prim"].astype(np.int64)
    assert (pr < n).all(), f"{what}: a prim out of range"
    assert (hits["reserved"] == 0).all(), f"{what}: a reserved word is not 0"
    cell = rows * n + pr
    assert len(cell) == 0 or np.bincount(cell, minlength=m * n).max() <= 1, f"{what}: a prim twice in one slice"
    got = np.full(m * n, NO_RECORD, dtype=np.uint64)
    got[cell] = dense_key(hits["dist2"], hits["feature"])
    got = got.reshape(m, n)
    acc = accepted_matrix(q, tris, radius, pairs, self_pairs, skip_shared)
    want = np.where(acc, dense_key(d2.reshape(-1), feat.reshape(-1)).reshape(m, n), NO_RECORD)
    there = got != NO_RECORD
    assert (got[there] == want[there]).all(), f"{what}: {int((got[there] != want[there]).sum())} records are not accepted pairs with bit-equal dist2 and the same feature"
    well = bf["well"]
    assert (got[well] == want[well]).all(), f"{what}: a well-conditioned query's slice differs on {int((got[well] != want[well]).any(axis=1).sum())} queries"
    if sorted_ and len(hits) > 1:
        same_row = rows[1:] == rows[:-1]
        d, p = hits["dist2"], hits["prim"]
        assert (~same_row | (d[1:] > d[:-1]) | ((d[1:] == d[:-1]) & (p[1:] > p[:-1]))).all(), f"{what}: a sorted slice does not ascend in (dist2, prim)"
    return got


def radius_unconditionally(pkg, q, tris, radius, bf, off, hits, sorted_, what, self_pairs=False, skip_shared=False):
    """test_gpu_radius_tris' comparison without a floor: every record recomputes (accepted, bit-equal dist2 and feature, no prim twice, j > i and no shared vertex
    in self mode), every slice is a subset of the brute force's, a sorted slice ascends in (dist2, prim), and the well-conditioned queries' slices are the brute
    force's byte for byte"""
    n = len(tris)
    msg = recompute_records(pkg, q, tris, radius, off, hits, self_pairs, skip_shared)
    assert msg is None, f"{what}: {msg}"
    rows = slice_rows(off)
    ref_rows = slice_rows(bf["offsets"])
    mine = rows * n + hits["prim"].astype(np.int64); theirs = ref_rows * n + bf["hits"]["prim"].astype(np.int64)
    assert np.isin(mine, theirs).all(), f"{what}: a record the brute force does not have"
    srt = hits if sorted_ else host_sorted(off, hits)
    if sorted_ and len(hits) > 1:
        same_row = rows[1:] == rows[:-1]
        d, p = hits["dist2"], hits["prim"]
        assert (~same_row | (d[1:] > d[:-1]) | ((d[1:] == d[:-1]) & (p[1:] > p[:-1]))).all(), f"{what}: a sorted slice does not ascend in (dist2, prim)"
    well = bf["well"]
    assert (np.diff(off.astype(np.int64)) == bf["counts"])[well].all(), f"{what}: a well-conditioned query's count differs"
    assert srt[well[rows]].tobytes() == bf["hits"][well[ref_rows]].tobytes(), f"{what}: a well-conditioned query's slice differs"


def rows_of(bf, idx):
    """the radius brute force of the queries ``idx`` alone"""
    o = bf["offsets"].astype(np.int64)
    counts = bf["counts"][idx]
    hits = np.concatenate([bf["hits"][o[i]:o[i + 1]] for i in idx]) if len(idx) else bf["hits"][:0]
    return {"offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32), "hits": hits, "counts": counts, "well": bf["well"][idx]}


def radius_guarded(pkg, ctx, res, qin, m, radius, flags, capacity, guard=8):
    """one bvh_radius_tris call on guard-filled arrays: (total, offsets, hits as u32 words of capacity + guard records)"""
    d_off = ctx.upload(np.full(m + 1 + 4, GUARD, dtype=np.uint32))
    d_hits = ctx.upload(np.full(4 * (capacity + guard), GUARD, dtype=np.uint32))
    try:
        rc, total = radius_call(pkg, ctx, res, qin, m, radius, flags, d_off.ptr, d_hits.ptr, capacity)
        ctx.synchronize()
        assert rc == 0, rc
        off = d_off.download(np.uint32, m + 1 + 4)
        assert (off[m + 1:] == GUARD).all(), "d_offsets written past n_queries + 1 words"
        return total, off[: m + 1], d_hits.download(np.uint32, 4 * (capacity + guard))
    finally:
        d_off.free(); d_hits.free()


def radius_all_ways(pkg, ctx, res, qin, m, q, tris, radius, bf, what, with_sorted, self_flags=0, pairs=None):
    """count-only + unsorted fill, a sorted fill (with_sorted), a fill between guard words and one a record short, on all of the queries.  An answer above
    HEAVY records goes through records_against_pairs; returns (offsets, the answer in sorted form — None for those)"""
    self_pairs = bool(self_flags & pkg.RADIUS_TRIS_SELF); skip = bool(self_flags & pkg.RADIUS_TRIS_SKIP_SHARED)
    big = int(bf["offsets"][-1]) > HEAVY

    def check(off, hits, sorted_, w):
        if big:
            return records_against_pairs(pkg, q, tris, radius, pairs, bf, off, hits, sorted_, w, self_pairs, skip)
        radius_unconditionally(pkg, q, tris, radius, bf, off, hits, sorted_, w, self_pairs, skip)
    uoff, uhits = search(pkg, ctx, res, qin, m, radius, self_flags)              # (asserts that the count-only offsets equal the fill call's)
    dense = check(uoff, uhits, False, what + " unsorted")
    usrt = None if big else host_sorted(uoff, uhits)
    total = int(uoff[-1])
    if with_sorted:
        off, hits = search(pkg, ctx, res, qin, m, radius, self_flags | pkg.RADIUS_TRIS_SORTED)
        assert off.tobytes() == uoff.tobytes(), f"{what}: sorted and unsorted calls count differently"
        sdense = check(off, hits, True, what + " sorted")
        assert (sdense == dense).all() if big else hits.tobytes() == usrt.tobytes(), f"{what}: the sorted and the unsorted fill are different sets"
    # exactly enough between guard words (sorted where the slices are short: a sorted fill of a long slice takes seconds)
    gflags = self_flags | (pkg.RADIUS_TRIS_SORTED if with_sorted and int(bf["counts"].max(initial=0)) <= LONG else 0)
    t, goff, words = radius_guarded(pkg, ctx, res, qin, m, radius, gflags, total)
    assert t == total and goff.tobytes() == uoff.tobytes() and (words[4 * total:] == GUARD).all(), f"{what}: past the total"
    ghits = words[: 4 * total].view(pkg.TRI_HIT)
    if big:
        assert (check(goff, ghits, bool(gflags & pkg.RADIUS_TRIS_SORTED), what + " between guard words") == dense).all(), f"{what}: the guarded fill is another answer"
    else:
        assert host_sorted(goff, ghits).tobytes() == usrt.tobytes(), f"{what}: the guarded fill is another answer"
    if total:
        t, goff, words = radius_guarded(pkg, ctx, res, qin, m, radius, self_flags, total - 1)
        assert t == total and goff.tobytes() == uoff.tobytes() and (words == GUARD).all(), f"{what}: one record short"
    return uoff, usrt


@pytest.mark.parametrize("name", MESH_NAMES)
def test_closest_and_radius_tris(pkg, ctx, name):
    """bvh_closest_tris (CLOSEST, ANY) and bvh_radius_tris (sorted, unsorted) at every radius of the CPU file, and the two against each other; on the frames
    BVH_RADIUS_TRIS_SELF | SKIP_SHARED on every tree.  `denormals` is held to the unconditional guarantees only (its well-conditioned
    share is printed).  The one thing sampled is the sorted fill of slices above LONG records: see the file's docstring"""
    tris = mesh(pkg, name); n = len(tris)
    q, fam, per, _, _ = tri_reference(pkg, name)
    m = len(q)
    exact = name in TRI_EXACT
    print(f"{name}: well-conditioned share " + ", ".join(f"{label} {cbf['well'].mean():.3f} / {rbf['well'].mean():.3f}" for label, (_, cbf, rbf) in per.items()))
    if exact:
        assert all(cbf["well"].mean() >= 0.99 and rbf["well"].mean() >= 0.99 for _, cbf, rbf in per.values())
    d_q = ctx.upload(q)
    idx = np.arange(0, m, 10)                                         # the queries whose LONG slices are sorted again on the later trees: every tenth
    q_sub = np.ascontiguousarray(q[idx]); d_sub = ctx.upload(q_sub)
    pairs = pairs_of(pkg, name); pairs_sub = (pairs[0][idx], pairs[1][idx])
    first = {}
    try:
        qin = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_q.ptr, None, None, 0, 0)
        qin_sub = pkg.BuildInput(pkg.TRI_PADDED64, 30, d_sub.ptr, None, None, 0, 0)
        for algo, label, b, res in each_tree(pkg, ctx, tris):
            for rl, (radius, cbf, rbf) in per.items():
                what = f"{name} {label} radius {rl}"
                c = closest_raw(pkg, ctx, res, d_q, m, radius, pkg.QUERY_CLOSEST)
                a = closest_raw(pkg, ctx, res, d_q, m, radius, pkg.QUERY_ANY)
                closest_unconditionally(pkg, q, tris, radius, cbf, c, a, what)
                long_ = int(rbf["counts"].max(initial=0)) > LONG
                # every query on every tree: count, unsorted fill, guard words, one short; the sorted fill too, except that LONG slices (a sorted fill of
                # them takes up to seconds) are sorted in full on the first tree only and, at the infinite radius, on every tenth query on builders 1 to 3
                off, srt = radius_all_ways(pkg, ctx, res, qin, m, q, tris, radius, rbf, what, with_sorted=not long_ or rl not in first, pairs=pairs)
                if long_ and rl in first and rl == "inf" and label.endswith("as built"):
                    sbf = rows_of(rbf, idx)
                    soff, shits = search(pkg, ctx, res, qin_sub, len(idx), radius, pkg.RADIUS_TRIS_SORTED)
                    assert np.array_equal(np.diff(soff.astype(np.int64)), np.diff(off.astype(np.int64))[idx]), f"{what}: every tenth query counts differently"
                    records_against_pairs(pkg, q_sub, tris, radius, pairs_sub, sbf, soff, shits, True, what + ", every tenth query sorted")
                # the two entry points on the well-conditioned queries: a sorted slice starts with the closest answer, ANY hits iff the slice is not empty
                well = cbf["well"] & rbf["well"]
                has = np.diff(off.astype(np.int64)) > 0
                assert (has == (c["prim"] != pkg.INVALID))[well].all() and (has == (a["prim"] != pkg.INVALID))[well].all(), what
                if srt is not None:
                    assert srt[off[:-1][has & well]].tobytes() == c[has & well].tobytes(), f"{what}: the first sorted record is not bvh_closest_tris' answer"
                if rl not in first:
                    first[rl] = (c, off, srt)
                else:                                                 # one answer on the well-conditioned queries, whatever the builder and the layout
                    c0, off0, srt0 = first[rl]
                    assert c[cbf["well"]].tobytes() == c0[cbf["well"]].tobytes(), f"{what}: differs from builder 0"
                    assert (np.diff(off.astype(np.int64)) == np.diff(off0.astype(np.int64)))[rbf["well"]].all(), f"{what}: counts differ from builder 0's"
                    if srt is not None:                               # (the answers above HEAVY: each equals the brute force's matrix on these queries)
                        assert srt[rbf["well"][slice_rows(off)]].tobytes() == srt0[rbf["well"][slice_rows(off0)]].tobytes(), f"{what}: differs from builder 0"
            if name in FRAMES:
                for rl, (radius, sbf) in self_reference(pkg, name)[1].items():
                    radius_all_ways(pkg, ctx, res, None, n, tris, tris, radius, sbf, f"{name} {label} self radius {rl}",
                                    with_sorted=int(sbf["counts"].max(initial=0)) <= LONG or label == "algo 0 as built",
                                    self_flags=pkg.RADIUS_TRIS_SELF | pkg.RADIUS_TRIS_SKIP_SHARED, pairs=pairs_of(pkg, name, True))
    finally:
        d_q.free(); d_sub.free()


# ---- bvh_winding_prepare and bvh_winding_number ----------------------------------------------------------------------------------------------------------------------

def moments_checks(pkg, dev, host, what):
    """bit for bit where the restatement is not a NaN, a NaN exactly where it has one"""
    d = dev.view(np.float32).reshape(len(dev), -1); h = host.view(np.float32).reshape(len(host), -1)
    dn, hn = np.isnan(d), np.isnan(h)
    assert (dn == hn).all(), f"{what}: moments: NaN in {int(dn.sum())} words, the restatement in {int(hn.sum())} (first difference at word {np.argwhere(dn != hn)[:1].tolist()})"
    assert (d.view(np.uint32)[~hn] == h.view(np.uint32)[~hn]).all(), f"{what}: moments differ on {int((d.view(np.uint32) != h.view(np.uint32))[~hn].sum())} words that are not NaN"


def winding_checks(pkg, what, tris, nodes, leaves, layout, root, host, xyz_, well, got, beta):
    """NaN exactly where the header's formula — the f32 terms accumulated in f64 — gives NaN, and then the canonical one; where the answer and every restatement
    are finite, test_gpu_winding.check_walk's bound, unchanged: |gpu - walk_host(f64)| <= TOL_FACTOR * max |walk_host(f32) - walk_host(f64)| (floor TOL_FLOOR)
    over the points farther than 1e-4 of the diagonal from the surface.  Returns (bound, error, how many points it covers, NaN answers)"""
    want = walk_host_sum64(nodes, leaves, layout, root, tris, host, xyz_, beta)
    nan_got, nan_want = np.isnan(got), np.isnan(want)
    assert (nan_got == nan_want).all(), (f"{what} beta {beta}: NaN on {int(nan_got.sum())} points, the restatement on {int(nan_want.sum())}; device only "
                                         f"{np.nonzero(nan_got & ~nan_want)[0][:6].tolist()}, restatement only {np.nonzero(~nan_got & nan_want)[0][:6].tolist()}")
    assert (got.view(np.uint32)[nan_got] == WIND_NAN_BITS).all(), f"{what} beta {beta}: a NaN answer is not 0x7FC00000"
    with np.errstate(all="ignore"):
        w64 = walk_host(nodes, leaves, layout, root, tris, host, xyz_, beta, np.float64)
        w32 = walk_host(nodes, leaves, layout, root, tris, host, xyz_, beta, np.float32).astype(F64)
    sel = well & np.isfinite(got) & np.isfinite(want) & np.isfinite(w64) & np.isfinite(w32)
    if not sel.any():
        return float("nan"), float("nan"), 0, int(nan_got.sum())
    tol = max(TOL_FACTOR * float(np.abs(w32[sel] - w64[sel]).max()), TOL_FLOOR)
    err = float(np.abs(got[sel].astype(F64) - w64[sel]).max())
    assert err <= tol, f"{what} beta {beta}: {err:.3e} > {tol:.3e}"
    return tol, err, int(sel.sum()), int(nan_got.sum())


@pytest.mark.parametrize("name", MESH_NAMES)
def test_winding(pkg, ctx, name):
    tris = mesh(pkg, name); n = len(tris)
    xyz_, live, well, plain, bf = wind_reference(pkg, name)
    pts = np.zeros(len(xyz_), dtype=pkg.POINT_QUERY)
    pts["point"] = xyz_; pts["radius"] = np.inf
    rows = []
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        keep = []
        try:
            for label, res, nodes, leaves, layout in trees_with_nodes(pkg, ctx, b, keep):
                what = f"{name} algo {algo} {label}"
                mom = prepare(pkg, ctx, res); keep.append(mom)
                host = moments_host(pkg, nodes, leaves, layout, res.root, tris)
                moments_checks(pkg, mom.download(pkg.WINDING_MOMENT, n - 1), host, what)
                for beta in (2.0, np.inf):
                    got = winding(pkg, ctx, res, mom, pts, beta)
                    assert (got.view(np.uint32)[~live] == WIND_NAN_BITS).all(), f"{what}: a NaN point does not answer the canonical NaN"
                    rows.append((beta,) + winding_checks(pkg, what, tris, nodes, leaves, layout, res.root, host, xyz_, well, got, beta))
                    if np.isinf(beta):                                # beta = +inf is the plain sum over all triangles, whatever the tree
                        assert (np.isnan(got) == np.isnan(plain)).all(), f"{what}: beta inf: the NaN answers are not the plain sum's"
        finally:
            for k in keep:
                k.free()
    for beta in (2.0, np.inf):
        mine = [r for r in rows if r[0] == beta]
        print(f"wind   {name:20s} beta {beta}: bound {np.nanmax([r[1] for r in mine]):.3e}, error {np.nanmax([r[2] for r in mine]):.3e} on {max(r[3] for r in mine)} points, "
              f"NaN answers {min(r[4] for r in mine)} to {max(r[4] for r in mine)} of {len(xyz_)}" if any(r[3] for r in mine) else
              f"wind   {name:20s} beta {beta}: no finite answer to bound, NaN answers {min(r[4] for r in mine)} to {max(r[4] for r in mine)} of {len(xyz_)}")


# ---- bvh_cull --------------------------------------------------------------------------------------------------------------------------------------------------------

_CULL_REF = {}


def cull_reference(pkg, name, per, leaf):
    if (name, per) not in _CULL_REF:
        _CULL_REF[(name, per)] = (leaf, pkg.cull_brute_force(volumes_of(pkg, name, per), leaf))
    assert _CULL_REF[(name, per)][0].tobytes() == leaf.tobytes(), f"{name}: the leaf boxes differ from the first tree's"
    return _CULL_REF[(name, per)][1]


def expected_on(pkg, tree, vols, ref):
    """(offsets, records) bvh_cull must answer on this tree: the brute force's slice where no plane value of any node is a NaN (the contract's exactness
    condition), the host restatement of the walk on this very tree elsewhere — which must be a subset of the brute force's.  Also how many volumes are exact"""
    ok = nan_free(pkg, tree, vols)
    off, hits = ref
    if ok.all():
        return off, hits, len(vols)
    parts = []
    for i in range(len(vols)):
        mine = hits[off[i]:off[i + 1]]
        if not ok[i]:
            walked = by_prim(group_walk(pkg, tree, vols[i])[0])
            assert np.isin(walked.view(np.uint64), mine.view(np.uint64)).all()
            mine = walked
        parts.append(mine)
    counts = np.array([len(p) for p in parts], dtype=np.uint64)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32), np.concatenate(parts), int(ok.sum())


@pytest.mark.parametrize("name", MESH_NAMES)
def test_cull(pkg, ctx, name):
    """records and straddle masks byte for byte.  On every as-built tree: both forced walks and AUTO, at 1, 65 and all volumes of 6 planes and at all volumes
    of 1 and 8 planes.  On the layout-0 copies of the layout-1 trees (caller-filled arrays: the same kernels instantiated for the other layout): both forced
    walks at all volumes of every plane count — AUTO only chooses between the two by n_volumes and n_leaves, which a copy does not change, and the volume counts
    only change how many lanes or workgroups a launch has"""
    tris = mesh(pkg, name); n = len(tris)
    figures = []
    for algo in (0, 1, 2, 3):
        b = pkg.BUILDERS[algo]().build(ctx, tris)
        keep = []
        try:
            for label, res, nodes, leaves, layout in trees_with_nodes(pkg, ctx, b, keep):
                tree = Tree(nodes, leaves, res.root, n, layout)
                built = label == "as built"
                for per in PLANE_COUNTS:
                    vols = volumes_of(pkg, name, per)
                    ref = cull_reference(pkg, name, per, tree.leaf_boxes)
                    off, hits, n_exact = expected_on(pkg, tree, vols, ref)
                    figures.append((per, n_exact, int(off[-1])))
                    for count in ((1, 65, len(vols)) if per == 6 and built else (len(vols),)):
                        want = (off[: count + 1], hits[: off[count]])
                        for path in ((LANE, GROUP, AUTO) if built else (LANE, GROUP)):
                            what = f"{name} algo {algo} {label}, {count} volumes x {per} planes, path {path}"
                            rc, goff, ghits, total = run_cull(pkg, ctx, res, vols[:count], path, guard=4)
                            assert rc == 0 and total == int(want[0][-1]), f"{what}: {total} records, expected {int(want[0][-1])}"
                            check_cull(pkg, goff, ghits, want[0], want[1], what)
                    total = int(off[-1])                              # one record short: the total is reported, nothing is filled
                    for path in (LANE, GROUP):
                        rc, goff, ghits, t = run_cull(pkg, ctx, res, vols, path, capacity=total - 1, guard=4)
                        assert rc == 0 and t == total and goff.tobytes() == off.tobytes() and untouched(ghits), f"{name} algo {algo} {label} x {per}: one record short"
        finally:
            for k in keep:
                k.free()
    for per in PLANE_COUNTS:
        mine = [f for f in figures if f[0] == per]
        print(f"cull   {name:20s} x {per} planes: {mine[0][2]} records, volumes exact on a tree {min(f[1] for f in mine)} to {max(f[1] for f in mine)} of {N_VOLUMES + 16}")
        assert all(f[2] == mine[0][2] for f in mine) or name == "huge_offset"


def test_cull_a_box_that_lies_at_infinity(pkg):
    """caller-filled arrays: the base mesh's LBVH tree with one leaf moved to x = +inf (lo.x = hi.x = +inf, which no box of this library has) and its
    ancestors' boxes grown to hold it.  Such a box takes the kernels' plain form of the plane test; a zero coefficient still contributes a zero there — the
    volumes hold +0 and -0 coefficients on x (the padding planes, extreme volumes 3 to 7 of the CPU file: the all -0 plane among them) —, so no plane value
    is a NaN and both walks equal the brute force over the leaf boxes for every volume of the CPU file.  (A context of its own: the tree is the caller's, and
    the session context's own tree and cached plan stay what the other tests left.)"""
    tris = mesh(pkg, "base"); n = len(tris)
    c = pkg.Context(0)
    d_nodes = None
    try:
        b = pkg.BUILDERS[1]().build(c, tris)
        assert b.result.layout == 0
        nodes = b.download()["nodes"].copy()
        ni = n - 1
        parent = np.full(2 * n - 1, -1, dtype=np.int64)
        parent[nodes["left"][:ni]] = np.arange(ni); parent[nodes["right"][:ni]] = np.arange(ni)
        v = ni + n // 3
        moved = int(nodes["left"][v])
        nodes["min"][v, 0] = np.inf; nodes["max"][v, 0] = np.inf
        while parent[v] >= 0:
            v = int(parent[v]); nodes["max"][v, 0] = np.inf
        tree = Tree(nodes, None, b.result.root, n, 0)
        assert np.isinf(tree.leaf_boxes["min"]).sum() == 1
        d_nodes = c.upload(nodes)
        r = pkg.Result(); r.d_nodes = d_nodes.ptr; r.root = b.result.root; r.n_internal = ni; r.n_leaves = n; r.layout = 0
        for per in PLANE_COUNTS:
            vols = volumes_of(pkg, "base", per)
            ref = pkg.cull_brute_force(vols, tree.leaf_boxes)
            assert nan_free(pkg, tree, vols).sum() == len(vols) - 1          # (all but the volume with a NaN offset, which is empty)
            ext = [ref[1][ref[0][N_VOLUMES + k]:ref[0][N_VOLUMES + k + 1]]["prim"] for k in range(16)]
            # x >= centre and the all -0 plane pass the moved leaf, x <= centre fails it, and +0 / -0 on x (volumes 3 and 7: a half-space in y) decide alike
            assert moved in ext[1] and moved in ext[5] and moved in ext[6] and moved not in ext[2] and (moved in ext[3]) == (moved in ext[7])
            for path in (LANE, GROUP):
                rc, goff, ghits, total = run_cull(pkg, c, r, vols, path, guard=4)
                assert rc == 0 and total == int(ref[0][-1])
                check_cull(pkg, goff, ghits, ref[0], ref[1], f"a leaf at x = +inf, {per} planes, path {path}")
    finally:
        if d_nodes is not None:
            d_nodes.free()
        c.close()
