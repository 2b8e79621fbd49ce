"""CPU-side checks of the per-instance statistics (lbft_batch_instance_stats): the entry point is declared, exported and bound, the
launcher lives in liblbft_commit_times.so alone, NULL arguments are refused before any HIP call, the Python methods check `since`
before any library call, the grid tool knows the option, the kernel is in the side library's code object exactly once, without scratch
or spills and with an LDS footprint that lets two workgroups share a compute unit, and seed_spread -- numpy alone -- gives the means,
deviations, extremes and seeds of a table written by hand."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import instance_stats_reference as ref
from support import Stub, hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "librabft_simulator_amd", "csrc")
NAME = "lbft_batch_instance_stats"
LAUNCHER = "lbft_ct_launch_instances"


def test_symbol_is_declared_exported_and_bound(hiplib):
    from librabft_simulator_amd import build
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    assert NAME in declared and NAME in hiplib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(hiplib.LIB_PATH), NAME)
    assert len(getattr(hiplib.lib(), NAME).argtypes) == 3
    assert re.search(r"#define LBFT_INSTANCE_STATS 44\b", header) and re.search(r"#define LBFT_INSTANCE_FAMILIES 11\b", header)
    assert hiplib.INSTANCE_STATS == 44 == ref.INSTANCE_STATS == 4 * len(hiplib.INSTANCE_FAMILIES) and tuple(hiplib.INSTANCE_FAMILIES) == ref.NAMES
    assert len(set(hiplib.INSTANCE_FAMILIES)) == 11 == ref.FAMILIES
    # the launcher: in the commit-time library, in no other, in the table and in the typedefs
    assert LAUNCHER in build.TABLE[2].launchers and build.TABLE[2].tag == "commit_times"
    assert hasattr(ctypes.CDLL(build.CT_OUT), LAUNCHER)
    for other in (hiplib.LIB_PATH, *other_libs("commit_times")):
        assert not hasattr(ctypes.CDLL(other), LAUNCHER), other
    assert "lbft_ct_instances_fn" in open(os.path.join(CSRC, "lbft_commit_times.h")).read()
    rules = os.path.join(CSRC, "lbft_instance_stats.h")
    assert rules in build.CT_DEPS and rules not in build.DEPS  # liblbft_hip.so includes nothing of it: its device code stays as it is
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", open(rules).read())
    assert sorted(includes) == ["lbft_chain_rules.h", "lbft_commit_finality.h", "lbft_commit_timeline.h", "lbft_group_stats.h", "stdint.h"]
    main = open(os.path.join(CSRC, "lbft_hip.hip")).read()
    assert main.count("load_side_lib(") == 6 and len(build.TABLE) == 6  # its definition and five calls; six libraries


def test_null_arguments_are_refused_without_a_gpu(hiplib):
    L = hiplib.lib()
    rows = np.full(44, 7, dtype=np.uint64)
    since = np.zeros(1, dtype=np.int64)
    for s in (None, since.ctypes.data):
        assert getattr(L, NAME)(None, s, rows.ctypes.data) == hiplib.LBFT_ERR_INVALID
        assert getattr(L, NAME)(None, s, None) == hiplib.LBFT_ERR_INVALID
    assert (rows == 7).all()


def test_python_methods_refuse_a_bad_since_before_the_device():
    from librabft_simulator_amd.simulator import BatchResult
    res = BatchResult(Stub())
    for since in (-1, 1001, [0, 0], [], "partition_start", [1001]):
        with pytest.raises(ValueError):
            res.instance_stats(since=since)
        with pytest.raises(ValueError):
            res.seed_spread(since=since)


def test_grid_spread_option_is_parsed():
    from librabft_simulator_amd import grid
    with pytest.raises(SystemExit):  # a bad option ends the tool before it creates a batch
        grid.main(["--spread", "--seeds-per-point", "0"])
    with pytest.raises(SystemExit):
        grid.main(["--spread=yes"])
    assert "--spread" in grid.__doc__


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_kernel_is_in_the_commit_time_library_without_scratch(hiplib):
    """LDS: the tile of 4 wavefronts x 32 nodes x 64 entries x 4 B = 32 KiB and 32 rights: 32 896 B; a compute unit has 160 KiB, so two
    workgroups share it when each takes at most 80 KiB."""
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    ct = _kernel_metadata(build.CT_OUT)
    mine = [(k, v) for k, v in ct.items() if "lbft_k_ct_instances" in k]
    assert len(mine) == 1 and len([k for k in ct if re.search(r"\d+lbft_k_ct_instancesN", k)]) == 1, sorted(ct)
    name, meta = mine[0]
    for word in ("run", "finality", "timeline", "latency_hist"):  # the substrings the other ABI tests pick their kernels by
        assert word not in name, name
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta.get("sgpr_spill_count", 0) == 0, meta
    assert meta["group_segment_fixed_size"] == 4 * 32 * 64 * 4 + 32 * 4 <= 80 * 1024, meta
    assert meta["vgpr_count"] <= 128, meta  # four wavefronts per SIMD: the two workgroups a unit's LDS admits at the very least
    for other in other_libs("commit_times"):
        assert not any("lbft_k_ct_instances" in k for k in _kernel_metadata(other)), other


# ---- seed_spread on a table written by hand: no device ----
def hand_table():
    """Six instances: group 0 = {0, 2, 3, 5}, group 1 = {1}, group 2 = {4}; instance 3 faulted (its row all zero); instance 5 without a
    latency or finality sample (it committed nothing); instances 0 and 2 tie on the longest stall and on the commit count."""
    S = np.zeros((6, 11, 4), dtype=np.uint64)

    def put(i, f, samples, total, lo, hi):
        S[i, f] = (samples, total, lo, hi)
    for i, (lat, stall, rec, fq, spr, opn) in {0: ((10, 400, 20, 70), 300, 40, (5, 250, 30, 90), 12, 2), 2: ((8, 400, 25, 95), 300, 55, (4, 100, 20, 30), 7, 0),
                                               1: ((6, 120, 10, 30), 100, 9, (3, 60, 15, 25), 3, 1), 4: ((2, 50, 20, 30), 700, 0, (1, 44, 44, 44), 0, 5)}.items():
        put(i, ref.LATENCY, *lat)
        put(i, ref.GAPS, 3, 30, 5, 15)
        put(i, ref.FIRST, 4, 4 * rec, rec, rec)
        put(i, ref.TAIL, 4, 40, 10, 10)
        put(i, ref.LONGEST, 4, 4 * stall, stall, stall)
        put(i, ref.FIN_QUORUM, *fq)
        put(i, ref.SPREAD, 2, 2 * spr, spr, spr)
        put(i, ref.OPEN, 1, opn, opn, opn)
    put(5, ref.TAIL, 4, 4000, 1000, 1000)
    put(5, ref.LONGEST, 4, 4000, 1000, 1000)
    put(5, ref.OPEN, 1, 0, 0, 0)
    counts = np.array([[9, 7, 8, 9], [3, 3, 3, 3], [7, 9, 9, 9], [50, 50, 50, 50], [1, 2, 2, 2], [0, 0, 0, 0]], dtype=np.uint32)
    faults = np.array([0, 0, 0, 8, 0, 0], dtype=np.uint32)
    set_of = np.array([0, 1, 0, 0, 2, 0], dtype=np.uint32)
    seeds = np.array([101, 102, 103, 104, 105, 106], dtype=np.uint64)
    return S, counts, faults, set_of, seeds


def test_seed_spread_of_a_hand_made_table(monkeypatch):
    from librabft_simulator_amd.simulator import BatchResult, ParamSet
    S, counts, faults, set_of, seeds = hand_table()

    class Sets(Stub):
        param_sets = [ParamSet(), ParamSet(), ParamSet(), ParamSet()]
        num_instances = 6
        set_of_instance = set_of
    Sets.seeds = seeds
    asked = []
    monkeypatch.setattr(BatchResult, "instance_stats", lambda self, since=None: (asked.append(since), S.copy())[1])
    monkeypatch.setattr(BatchResult, "commit_counts", property(lambda self: counts))
    monkeypatch.setattr(BatchResult, "faults", property(lambda self: faults))
    rows = BatchResult(Sets()).seed_spread(since=[0, 1, 2, 3])
    assert asked == [[0, 1, 2, 3]] and [r["set"] for r in rows] == [0, 1, 2, 3]
    assert [(r["instances"], r["faulted"]) for r in rows] == [(4, 1), (1, 0), (1, 0), (0, 0)]
    keys = {"instances", "mean", "std", "stderr", "min", "max", "min_seed", "max_seed"}
    metrics = ("commits", "latency_mean", "latency_max", "longest_stall", "recovery", "finality_quorum_mean", "finality_quorum_max", "spread_max", "open")
    for r in rows:
        assert set(r) == {"set", "instances", "faulted", *metrics} and all(set(r[name]) == keys for name in metrics)
    g0 = rows[0]
    # commits: the minimum over the nodes, of instances 0, 2 and 5 (3 is faulted): 7, 7, 0 -- the tie on 7 goes to instance 0
    c = g0["commits"]
    assert (c["instances"], c["min"], c["max"], c["min_seed"], c["max_seed"]) == (3, 0.0, 7.0, 106, 101)
    assert c["mean"] == pytest.approx(14 / 3) and c["std"] == pytest.approx(np.std([7, 7, 0], ddof=1)) and c["stderr"] == pytest.approx(c["std"] / math.sqrt(3))
    # latency: instances 0 and 2 have samples, 5 has none: means 40 and 50
    lm = g0["latency_mean"]
    assert (lm["instances"], lm["mean"], lm["min"], lm["max"], lm["min_seed"], lm["max_seed"]) == (2, 45.0, 40.0, 50.0, 101, 103)
    assert lm["std"] == pytest.approx(math.sqrt(50)) and lm["stderr"] == pytest.approx(5.0)
    assert (g0["latency_max"]["max"], g0["latency_max"]["max_seed"], g0["latency_max"]["instances"]) == (95.0, 103, 2)
    # the longest stall: 300, 300 and instance 5's 1000; the tie on the minimum goes to instance 0
    ls = g0["longest_stall"]
    assert (ls["instances"], ls["min"], ls["min_seed"], ls["max"], ls["max_seed"]) == (3, 300.0, 101, 1000.0, 106)
    assert (g0["recovery"]["instances"], g0["recovery"]["max"], g0["recovery"]["max_seed"]) == (2, 55.0, 103)  # instance 5 has no `first` sample
    fq = g0["finality_quorum_mean"]
    assert (fq["instances"], fq["min"], fq["max"], fq["min_seed"], fq["max_seed"]) == (2, 25.0, 50.0, 103, 101)
    assert (g0["finality_quorum_max"]["max"], g0["spread_max"]["max"], g0["spread_max"]["max_seed"]) == (90.0, 12.0, 101)
    assert (g0["open"]["instances"], g0["open"]["mean"], g0["open"]["max_seed"]) == (3, pytest.approx(2 / 3), 101)
    # one instance: a value and no deviation; no instance: nothing
    g1 = rows[1]
    assert g1["latency_mean"] == {"instances": 1, "mean": 20.0, "std": None, "stderr": None, "min": 20.0, "max": 20.0, "min_seed": 102, "max_seed": 102}
    assert rows[2]["open"]["mean"] == 5.0 and rows[2]["recovery"]["max"] == 0.0 and rows[2]["commits"]["min_seed"] == 105
    for name in metrics:
        assert rows[3][name] == {"instances": 0, "mean": None, "std": None, "stderr": None, "min": None, "max": None, "min_seed": None, "max_seed": None}
    # a plain batch: one group of every instance
    class Plain(Stub):
        num_instances = 6
    Plain.seeds = seeds
    (row,) = BatchResult(Plain()).seed_spread()
    assert (row["set"], row["instances"], row["faulted"]) == (0, 6, 1) and row["commits"]["instances"] == 5 and row["longest_stall"]["max_seed"] == 106
    assert row["commits"]["min_seed"] == 106 and row["latency_mean"]["instances"] == 4 and row["open"]["max_seed"] == 105
