"""CPU: the data files bench.py prices its roofline with are consistent with their sources — the exact algorithmic bytes follow SURVEY.md §8(d)'s
formulas from the committed oracle statistics, the task share and the issue counters are well formed, and bench.py's helpers pick them up."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_exact_bytes_follow_the_survey_formulas():
    tab = json.load(open(os.path.join(ROOT, "profiles", "algorithmic_bytes.json")))
    gold = json.load(open(os.path.join(GOLDEN, "reference_outputs.json")))["_fullsize"]["uniform10000000_s1"]
    n = gold["n"]
    st = gold["hploc"]["stats"]
    emit = 4 + 16 + 4 * (st["cluster_loads"] + st["cluster_stores"]) / n + 28 * st["cluster_loads"] / n + 32      # keys + parentIdx exchange + ids + AABB loads + node
    e = tab["uniform_10000000_tris_hploc"]
    assert e["emit_bytes_per_prim"] == pytest.approx(emit, abs=2e-3) and e["pipeline_bytes_per_prim"] == pytest.approx(88 + 32 + 68 + 64 + emit, abs=2e-3)
    assert 380 < e["pipeline_bytes_per_prim"] < 395                      # SURVEY.md's estimate: ~386
    sp = gold["ploc"]["stats"]
    emit_p = (32 * sp["cluster_loads"] + 4 * sp["cluster_stores"]) / n + 32
    assert tab["uniform_10000000_tris_ploc"]["emit_bytes_per_prim"] == pytest.approx(emit_p, abs=2e-3)


def test_bench_helpers_read_the_data_files():
    b = _bench()
    ex = b.exact_bytes("uniform_10000000_tris_hploc")
    assert ex is not None and ex[1] == 64.0
    share = json.load(open(os.path.join(ROOT, "profiles", "hploc_task_share.json")))
    assert share["merge_tasks_total"] == 918014 and 0.8 < share["tile_kernel_share"] < 0.95
    blk, src = b.kernel_bytes_per_prim("k_hploc_block", "hploc", "uniform_10000000_tris_hploc")
    ext, _ = b.kernel_bytes_per_prim("k_hploc_ext", "hploc", "uniform_10000000_tris_hploc")
    assert blk + ext == pytest.approx(64.0 + ex[0], abs=1e-6) and "share" in src          # the two kernels split SetupClusters + emit, nothing lost
    assert b.kernel_bytes_per_prim("k_extents", "hploc", "uniform_10000000_tris_hploc")[0] == 88.0
    assert b.kernel_bytes_per_prim("k_hploc_block", "hploc", "no_such_workload")[0] == 177.9   # falls back to the survey constants


def test_bench_full_is_an_option_and_off_by_default():
    b = _bench()
    plain = b.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False and (plain.gpus, plain.steps, plain.warmup, plain.dump_outputs) == (1, 20, 5, None)
    full = b.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert full.full is True and {k: v for k, v in vars(full).items() if k != "full"} == {k: v for k, v in vars(plain).items() if k != "full"}


def test_issue_counter_file_is_recomputable():
    ic = json.load(open(os.path.join(ROOT, "profiles", "issue_counters.json")))
    e = ic["k_hploc_block@10000000"]
    cyc = e["SQ_BUSY_CYCLES"] / e["shader_engines"]
    valu = e["SQ_INSTS_VALU"] * e["cycles_per_valu_inst"] / (e["simds"] * cyc)
    lds = e["SQ_INSTS_LDS"] * e["cycles_per_lds_inst"] / (e["cus"] * cyc)
    assert 0.3 < valu <= 1.0 and 0.3 < lds < 1.0 and 0.3 < e["SQ_WAIT_ANY"] / e["SQ_WAVE_CYCLES"] < 0.8


def _as_result(ref):
    return {"nodes": ref["nodes"], "leaves": ref["leaves"], "sorted_keys": ref["skeys"], "sorted_vals": ref["svals"], "scene": ref["scene"],
            "root": ref["root"], "layout": ref["layout"]}


def _renumbered(res, seed):
    """the same tree with its internal nodes stored in another order (as HPLOC / PLOC++ may number them from run to run)"""
    nodes = res["nodes"]
    ni = len(res["sorted_vals"]) - 1
    perm = np.random.default_rng(seed).permutation(ni)                 # new position of old node i
    out = nodes.copy()
    out[perm] = nodes[:ni]
    for f in ("left", "right"):
        c = out[f][:ni]
        out[f][:ni] = np.where(c < ni, perm[np.minimum(c, ni - 1)], c)
    return dict(res, nodes=out, root=int(perm[res["root"]]))


@pytest.mark.parametrize("algo", [1, 3])
def test_dump_outputs_is_numbering_independent(pkg, orc, tmp_path, algo):
    """bench.py --dump-outputs: float32 / float64 files only, the whole result at this size, the same files for a renumbered tree and
    different ones for a tree with two children swapped"""
    b = _bench()
    tris = pkg.meshgen.uniform(5000, 7)
    n = len(tris)
    res = _as_result(orc.build_tree(algo, tris))
    got = b.dump_outputs(res, str(tmp_path / "a"))
    assert set(got) == {"sorted_keys", "sorted_vals", "leaves", "internal_nodes", "root_aabb", "scene", "meta"}
    for name, a in got.items():
        back = np.load(tmp_path / "a" / (name + ".npy"))
        assert back.dtype in (np.float32, np.float64) and np.array_equal(back, a, equal_nan=True)
    assert np.array_equal(got["sorted_keys"], res["sorted_keys"].astype(np.float64)) and np.array_equal(got["leaves"][:, 0], res["sorted_vals"].astype(np.float64))
    assert got["internal_nodes"].shape == (n - 1, 18) and got["leaves"].shape == (n, 7)
    nd = res["nodes"][res["root"]]
    assert np.array_equal(got["root_aabb"], np.concatenate([nd["min"], nd["max"]]))
    assert list(got["meta"]) == [n, n - 1, res["layout"], 32]

    again = b.dump_outputs(_renumbered(res, 1), str(tmp_path / "b"))
    assert all(np.array_equal(got[k], again[k]) for k in got)

    swapped = dict(res, nodes=res["nodes"].copy())
    swapped["nodes"]["left"][res["root"]], swapped["nodes"]["right"][res["root"]] = res["nodes"]["right"][res["root"]], res["nodes"]["left"][res["root"]]
    assert not np.array_equal(b.dump_outputs(swapped, str(tmp_path / "c"))["internal_nodes"], got["internal_nodes"])


def test_dump_outputs_sample_is_fixed_and_bounded(pkg, orc, tmp_path, monkeypatch):
    """larger outputs are cut to a fixed, seeded sample of rows: the same rows every run, at most 64 MB at the benchmark's 10 M triangles"""
    b = _bench()
    monkeypatch.setattr(b, "DUMP_ROWS", 256)
    res = _as_result(orc.build_tree(3, pkg.meshgen.uniform(4000, 3)))
    one = b.dump_outputs(res, str(tmp_path / "a"))
    two = b.dump_outputs(_renumbered(res, 2), str(tmp_path / "b"))
    assert all(np.array_equal(one[k], two[k]) for k in one)
    assert one["internal_nodes"].shape == (256, 18) and one["leaves"].shape == (256, 7) and one["sorted_keys"].shape == (256,)
    assert np.all(np.diff(one["sorted_keys"]) >= 0)
    s = b._sample_rows(4000, 256)
    assert np.array_equal(one["sorted_vals"], res["sorted_vals"][s].astype(np.float64))
    k = _bench().DUMP_ROWS                  # at the benchmark's size (10 M triangles, u32 keys): keys + values + leaves + internal nodes + the small arrays
    assert k * (2 * 8 + 7 * 8 + 18 * 4) + 4096 < 64 << 20
