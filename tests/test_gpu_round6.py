"""Round-6 GPU tests: the HPLOC schedulers build the same trees, also when one context switches between them, and BVH_OPT_HPLOC_SCHEDULER = 3 (round 6's
overlapped schedule, measured slower and removed, LEADS.md row 87) is still accepted and means the tile schedule; PLOC++ with chunk tickets only
(BVH_OPT_PLOC_SCHEDULER = 1, what the batched builder's lanes use) builds the same trees as the default; several PLOC++ builds at once on one device."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


def _mesh(pkg, kind, n, seed):
    return pkg.meshgen.uniform(n, seed) if kind == "uniform" else pkg.meshgen.sponza_like(n, seed) if kind == "sponza" else pkg.meshgen.bunny_like(n, seed)


@pytest.mark.parametrize("kind,n", [("uniform", 2_100_000), ("sponza", 1_000_000), ("bunny", 900_000), ("uniform", 1500), ("uniform", 10_000_000)])
def test_hploc_schedules_build_the_same_tree(pkg, ctx, kind, n):
    """the HPLOC schedulers agree byte for byte (node numbering follows from the topology alone: equal checksums = equal arrays), also when one context switches
    between them repeatedly; 3 (the removed overlapped schedule) reads back as 2 and runs the tile kernel, then the external climb"""
    tris = _mesh(pkg, kind, n, 7)
    with ctx.options(hploc="async"):
        ref = pkg.HPLOC().build(ctx, tris).checksum()
    got = []
    for mode in ("block", 3, "async", "block", 3, "block"):
        with ctx.options(hploc=mode):
            got.append(pkg.HPLOC().build(ctx, tris).checksum())
    assert got == [ref] * len(got), [f"{g:016x}" for g in got]
    with ctx.options(hploc=3):
        assert ctx.get_option("hploc") == 2
        try:
            ctx.set_profiling(2)
            pkg.HPLOC().build(ctx, tris)
            kt = ctx.kernel_times()
        finally:
            ctx.set_profiling(0)
    assert {k for k in kt if k.startswith("k_hploc")} == {"k_hploc_block", "k_hploc_ext"}, kt


def test_hploc_schedules_60_bit_keys(pkg, ctx):
    import torch
    tris = pkg.meshgen.uniform(1_300_000, 9)
    d = torch.from_numpy(tris.view(np.uint8).reshape(-1)).cuda()
    cks = {}
    for mode in ("block", 3, "async"):
        with ctx.options(hploc=mode):
            cks[mode] = pkg.HPLOC().build_ex(ctx, len(tris), tris=d, morton_bits=60).checksum()
    assert cks["block"] == cks[3] == cks["async"]


def test_hploc_tile_schedule_soak(pkg, ctx):
    """200 back-to-back tile-schedule builds without a synchronisation in between (each build's first kernel clears the queue heads behind the previous build's
    climb), then the last tree is checked against the one-launch schedule's"""
    tris = pkg.meshgen.uniform(2_000_000, 100)
    with ctx.options(hploc="async"):
        ref = pkg.HPLOC().build(ctx, tris).checksum()
    import torch
    d = torch.from_numpy(tris.view(np.uint8).reshape(-1)).cuda()
    with ctx.options(hploc="block"):
        b = pkg.HPLOC()
        for _ in range(200):
            b.build(ctx, d, on_device=True, n=len(tris))
        assert b.checksum() == ref


@pytest.mark.parametrize("kind,n", [("sponza", 262_144), ("uniform", 1_100_000), ("uniform", 700)])
def test_ploc_tickets_only_builds_the_same_tree(pkg, ctx, kind, n):
    tris = _mesh(pkg, kind, n, 3)
    cks = []
    for v in (0, 1, 2):                 # 2: ABI 4's removed cooperative launch — still accepted, means 0
        ctx.set_option("ploc", v)
        cks.append(pkg.PLOCNew().build(ctx, tris).checksum())
    ctx.set_option("ploc", 0)
    assert ctx.get_option("ploc") == 0 and cks[0] == cks[1] == cks[2]


def test_batched_ploc_lanes_soak(pkg, ctx):
    """the batched builder runs up to three lanes (contexts, streams) per device at once; its lanes take chunk tickets in every PLOC++ iteration (no reliance
    on a grid being co-resident).  Nine meshes of three sizes, five rounds: every tree equals the single build's."""
    meshes = [pkg.meshgen.sponza_like(262_144, 3 + m) if m % 3 == 0 else pkg.meshgen.uniform(150_000 + 1000 * m, 40 + m) if m % 3 == 1 else pkg.meshgen.uniform(1_050_000, 60 + m)
              for m in range(9)]
    ref = [pkg.PLOCNew().build(ctx, t).checksum() for t in meshes]
    batch = pkg.Batch((0,))
    try:
        for _ in range(5):
            rep = batch.build(meshes, pkg.ALGO_PLOCPP, checksums=True)
            assert [int(c) for c in rep["checksums"]] == ref
        assert rep["lanes_per_device"] >= 2
    finally:
        batch.close()
