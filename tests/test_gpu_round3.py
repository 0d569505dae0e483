"""GPU, round 3: the bench's real multi-GPU code path before the driver runs it (process group, staging copy, RCCL all-gather, max-over-ranks
reduction) at world size 1 and — where the box has them — 2 ranks; the 2-rank gloo flavour on one device; the per-context option API that
replaced the library's getenv knobs; the bvh_timings.sampled flag."""
import ctypes as C
import importlib.util
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _run_bench(nproc, extra_env, args=("--tris", "200000", "--steps", "3", "--warmup", "1", "--cpu-sample", "0")):
    env = dict(os.environ); env.update(extra_env); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), *args]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                   # rank 0 prints ONE JSON line
    return json.loads(lines[0])


def test_bench_nccl_gather_path_world1():
    """`bench.py` as the driver launches it (torch.distributed.run), the nccl branch of the exchange forced on at world size 1"""
    out = _run_bench(1, {"BVH_BENCH_FORCE_GATHER": "1"})
    assert out["n_gpus"] == 1 and out["allgather_us"] is not None and out["allgather_us"]["bytes_per_rank"] == 24 and out["allgather_us"]["mean"] > 0
    assert out["value"] > 0 and out["roofline"]["kernel"].startswith("k_")


def test_bench_nccl_two_ranks_when_two_devices():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device: the 2-rank RCCL run needs two")
    out = _run_bench(2, {})
    assert out["n_gpus"] == 2 and out["allgather_us"] is not None and out["scaling"] == "weak"


def test_bench_nccl_two_ranks_sharing_one_device_attempt():
    """no multi-GPU node is available to the builder, so `all_gather_into_tensor` at world size 2 and the config-5 block of bench.py have never run on
    hardware.  Try it with both RCCL ranks on the ONE visible device (bench.py maps LOCAL_RANK modulo the device count).  RCCL is entitled to refuse two ranks on one GPU
    ("Duplicate GPU detected"): the outcome is recorded either way — a pass executes the world-2 path end to end, a refusal is an expected failure with RCCL's message."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two devices are visible: test_bench_nccl_two_ranks_when_two_devices covers the real thing")
    env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0"); env["NCCL_DEBUG"] = "WARN"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--tris", "200000", "--steps", "3", "--warmup", "1", "--full", "--cpu-sample", "0"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.xfail("2 RCCL ranks on one device: the rendezvous did not complete within 300 s")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or len(lines) != 1:
        msg = [l for l in (r.stderr + r.stdout).splitlines() if "uplicate" in l or "NCCL WARN" in l or "ncclInvalidUsage" in l or "Error" in l][:3]
        pytest.xfail("RCCL refuses two ranks on one device: " + " | ".join(msg)[:400])
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["allgather_us"] is not None and out["scaling"] == "weak"
    assert out.get("config5") is None or out["config5"]["tris_per_gpu"] == 2_000_000


def test_bench_gloo_two_ranks_on_one_device():
    """the N > 1 control flow (per-rank meshes, barrier, max over ranks, one JSON line from rank 0) with two ranks sharing the device"""
    out = _run_bench(2, {"BVH_BENCH_BACKEND": "gloo"})
    assert out["n_gpus"] == 2 and out["allgather_us"] is not None
    assert out["config"]["tris_per_gpu"] == 200000 and out["value"] > 0


def test_bench_dump_outputs(pkg, orc, ctx, tmp_path):
    """bench.py --dump-outputs DIR (the benchmark's own command line, no launcher): --steps timed builds, then the last one's result as float .npy files,
    equal to the same build made here (node rows are numbering independent) and to the oracle's sort"""
    d = tmp_path / "bench"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--tris", "200000", "--steps", "3", "--warmup", "1", "--cpu-sample", "0",
           "--no-secondary", "--dump-outputs", str(d)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["config"]["builder"] == "HPLOC"
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    tris = pkg.meshgen.uniform(200_000, 1, offset=(0.0, 0.0, 0.0))              # rank 0's mesh
    here = bench.dump_outputs(pkg.HPLOC().build(ctx, tris).download(), str(tmp_path / "here"))
    assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
    for name, a in here.items():
        got = np.load(d / (name + ".npy"))
        assert got.dtype in (np.float32, np.float64) and got.dtype == a.dtype and np.array_equal(got, a), name
    fe = orc.front_end(tris, 30)
    assert np.array_equal(here["sorted_keys"], fe["skeys"].astype(np.float64)) and np.array_equal(here["sorted_vals"], fe["svals"].astype(np.float64))


FULL_ONLY = ("stage_ms", "sah_bvh2", "cpu_baseline", "secondary", "config5")          # what a line carries only when the run was asked for it with --full


def _run_plain_bench(*args):
    """bench.py in a new process, the benchmark's own command line: (its one JSON line, seconds from start to exit)"""
    import time
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), wall


def test_bench_plain_run_is_lean():
    """`bench.py --gpus 1 --steps N --warmup W` at the benchmark's own size: the headline fields, what the timed region's events give, and none of the legs that
    take runs of their own; the whole process, start to exit, spends at most 30 s outside its N + W steps"""
    steps, warmup = 20, 5
    out, wall = _run_plain_bench("--gpus", "1", "--steps", str(steps), "--warmup", str(warmup))
    assert out["metric"] == "bvh_build_throughput" and out["unit"] == "Mtris/s" and out["higher_is_better"] is True and out["dtype"] == "f32+u32"
    assert out["steps"] == steps and out["warmup"] == warmup and out["full"] is False and out["config"]["workload"] == "uniform_10000000_tris_hploc"
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(10_000_000 / out["ms_per_step"] / 1e3, rel=1e-3)
    assert out["roofline"]["kernel"].startswith("k_") and out["kernel_ms_per_step"]
    assert all(out[k] is None for k in FULL_ONLY), {k: out[k] for k in FULL_ONLY}
    outside = wall - (steps + warmup) * out["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.2f} s from start to exit, {outside:.2f} s outside its steps (mesh generation {out['mesh_gen_s']} s)")
    assert outside <= 30.0


def test_bench_full_runs_every_leg():
    """--full: the same line with the stage-timed build, the SAH cost, the other configs' loops and the CPU baseline (a small mesh and sample keep the test short)"""
    out, _ = _run_plain_bench("--gpus", "1", "--tris", "200000", "--steps", "3", "--warmup", "1", "--full", "--cpu-sample", "20000")
    assert out["full"] is True and out["steps"] == 3 and out["ms_per_step"] > 0 and out["roofline"]["kernel"].startswith("k_")
    assert out["stage_ms"]["TotalTime"] > 0 and out["sah_bvh2"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["sample"].startswith("first 20000 triangles")
    assert [e["workload"] for e in out["secondary"]] == ["sponza_262144_tris_lbvh_single", "sponza_262144_tris_ploc", "uniform_2000000_tris_hploc"]
    assert all(e["ms_per_step"] > 0 and e["cold_first_build_ms"] > 0 for e in out["secondary"]) and out["config5"] is None      # (config5 belongs to N > 1)
    # the options that shape those legs still switch them off one by one
    out, _ = _run_plain_bench("--gpus", "1", "--tris", "200000", "--steps", "3", "--warmup", "1", "--full", "--cpu-sample", "0", "--no-secondary")
    assert out["full"] is True and out["stage_ms"]["TotalTime"] > 0 and out["sah_bvh2"] > 0 and out["cpu_baseline"] is None and out["secondary"] is None


def test_ctx_options_replace_env_knobs(pkg, orc, ctx):
    L = pkg.lib()
    v = C.c_int64()
    for opt in range(4):
        assert L.bvh_ctx_get_option(ctx.handle, opt, C.byref(v)) == 0 and v.value == 0          # defaults: decide by size, no test knobs
    assert L.bvh_ctx_set_option(ctx.handle, pkg.OPT_HPLOC_SCHEDULER, 4) == -10001            # 0 auto, 1 one launch, 2 tiles then climb (3, round 6's overlapped schedule, is accepted and means 2)
    assert L.bvh_ctx_set_option(ctx.handle, pkg.OPT_PLOC_SCHEDULER, 3) == -10001
    assert L.bvh_ctx_set_option(ctx.handle, pkg.OPT_PLOC_SCHEDULER, 2) == 0 and L.bvh_ctx_get_option(ctx.handle, pkg.OPT_PLOC_SCHEDULER, C.byref(v)) == 0 and v.value == 0
    # (2, round 4's resident launch, was removed in round 5; an ABI-4 caller that still sets it gets the default — same trees — instead of an error: ADVICE r05)
    assert L.bvh_ctx_set_option(ctx.handle, pkg.OPT_PLOC_SCHEDULER, 0) == 0
    assert L.bvh_ctx_set_option(ctx.handle, pkg.OPT_SORT_TEST_KNOBS, 1) == -10001               # only the result-preserving knobs exist in the release library
    assert L.bvh_ctx_set_option(ctx.handle, 17, 0) == -10001 and L.bvh_ctx_get_option(ctx.handle, 17, C.byref(v)) == -10001
    # a stray environment variable must not change anything (round 2's library read BVH_HPLOC_MODE / BVH_LBVH_MODE / BVH_SORT_DEBUG)
    tris = pkg.meshgen.uniform(40_000, 5)
    ref = pkg.HPLOC().build(ctx, tris).checksum()
    os.environ["BVH_HPLOC_MODE"] = "block"; os.environ["BVH_SORT_DEBUG"] = "3"
    try:
        ctx.set_profiling(2)
        assert pkg.HPLOC().build(ctx, tris).checksum() == ref
        assert "k_hploc" in ctx.kernel_times() and "k_hploc_block" not in ctx.kernel_times()     # 40 k: the one-launch kernel, whatever the environment says
    finally:
        del os.environ["BVH_HPLOC_MODE"], os.environ["BVH_SORT_DEBUG"]; ctx.set_profiling(0)
    with ctx.options(hploc="block"):
        ctx.set_profiling(2)
        assert pkg.HPLOC().build(ctx, tris).checksum() == ref and "k_hploc_block" in ctx.kernel_times()
        ctx.set_profiling(0)
    assert ctx.get_option("hploc") == 0


def test_timings_sampled_flag(pkg, ctx):
    """bvh_ctx_set_kernel_sampling(k): k - 1 of k builds are un-instrumented and say so (sampled = 0, ms_* = 0)"""
    tris = pkg.meshgen.uniform(30_000, 6)
    ctx.set_kernel_sampling(3); ctx.set_profiling(1)
    flags = []
    for _ in range(6):
        b = pkg.SinglePassLbvh().build(ctx, tris)
        flags.append((b.timings.sampled, b.timings.ms_total > 0))
    ctx.set_kernel_sampling(1); ctx.set_profiling(0)
    assert flags == [(1, True), (0, False), (0, False)] * 2
    assert pkg.SinglePassLbvh().build(ctx, tris).timings.sampled == 0                              # profiling off


def test_batch_allgather_is_timed_outside_the_group(pkg):
    """the events around the RCCL all-gather were recorded inside ncclGroupStart/End and measured nothing for n_dev > 1"""
    import torch
    nd = torch.cuda.device_count()
    mg = pkg.meshgen
    meshes = [mg.uniform(20_000, 50 + m) for m in range(max(nd, 2))]
    L = pkg.lib()
    h = C.c_void_p(); devs = (C.c_int * nd)(*range(nd))
    assert L.bvh_batch_create(nd, devs, C.byref(h)) == 0
    try:
        ptrs = (C.c_void_p * len(meshes))(*[m.ctypes.data for m in meshes]); ns = (C.c_uint32 * len(meshes))(*[len(m) for m in meshes])
        roots = (C.c_float * (6 * len(meshes)))()
        rep = pkg.BatchReport(); rep.root_aabbs = C.cast(roots, C.POINTER(C.c_float))
        assert L.bvh_batch_build(h, 3, ptrs, ns, len(meshes), C.byref(rep)) == 0
        assert rep.allgather_us > 0.5, rep.allgather_us            # a collective (or its one-rank copy) takes microseconds, not an empty interval
    finally:
        L.bvh_batch_destroy(h)


def test_ploc_first_batch_follows_the_previous_build(pkg, orc, ctx):
    """run_ploc aims its first batch of launches one above the previous same-size build's iteration count (csrc/api.hip; the reference reads back after
    every iteration, src/PLOC++Bvh.cpp:132-152).  Same n, different meshes: a scene that needs MORE iterations than its predecessor (second batch), fewer,
    and the same again — node arrays byte-identical to the oracle's and the iteration counts the oracle's every time."""
    n = 40_000
    meshes = [pkg.meshgen.uniform(n, 3), pkg.meshgen.sponza_like(n, 5)[:n], pkg.meshgen.bunny_like(n, 7)[:n], pkg.meshgen.uniform(n, 3)]
    flat = pkg.meshgen.uniform(n, 9).copy(); flat.view(np.float32).reshape(n, -1)[:, [2, 5, 8]] *= 1e-4          # a nearly flat scene: many more iterations
    meshes.insert(2, flat)
    iters = []
    for tris in meshes:
        assert len(tris) == n
        b = pkg.PLOCNew().build(ctx, tris)
        got = b.download(); ref = orc.build_tree(2, tris)
        assert got["nodes"].tobytes() == ref["nodes"].tobytes() and got["leaves"].tobytes() == ref["leaves"].tobytes()
        assert b.timings.ploc_iterations == ref["stats"]["iterations"]
        iters.append(b.timings.ploc_iterations)
    assert iters[0] == iters[-1] and len(set(iters)) > 1, iters      # (the sequence really exercised a change of the count)


def test_scene_extent_is_fresh_for_every_build(pkg, orc):
    """The build path double-buffers the scene extent (the Morton kernel of one build resets the extent the NEXT build reduces into, csrc/api.hip) and clears
    its bookkeeping inside stage E's kernel.  A scene nested inside the previous one, a different builder, a failed build in between and a re-allocation
    must all see a clean extent: scene box and sorted keys equal to the oracle's (CalculateSceneExtents / CalculateMortonCodes, src/CommonBlocksKernel.h:92-114,374-385)."""
    ctx = pkg.Context(0)
    try:
        big = pkg.meshgen.uniform(30_000, 5)
        small = pkg.meshgen.uniform(20_000, 6).copy()
        v = small.view(np.float32).reshape(len(small), -1)
        v[:, :9] = v[:, :9] * 0.01 + 0.4                                  # a scene well inside the first one's extent
        seq = [(big, 3), (small, 3), (small, 1), (big, 2), (small, 0), (big, 3)]
        for k, (tris, algo) in enumerate(seq):
            if k == 3:                                                      # a build that fails before anything is enqueued ...
                with pytest.raises(pkg.BvhError):
                    pkg.BUILDERS[algo]().build_ex(ctx, 10, tris=None)
            if k == 4:                                                      # ... and a re-allocation of the arena
                ctx.reserve(200_000)
            got = pkg.BUILDERS[algo]().build(ctx, tris).download()
            ref = orc.build_tree(algo, tris)
            assert got["scene"].tobytes() == ref["scene"].tobytes(), f"step {k}"
            assert np.array_equal(got["sorted_keys"], ref["skeys"]) and np.array_equal(got["sorted_vals"], ref["svals"]), f"step {k}"
    finally:
        ctx.close()
