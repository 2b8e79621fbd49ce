"""CPU-side checks of the commit timelines (lbft_batch_commit_series / lbft_batch_commit_stalls): the entry points are declared, exported
and bound, their launcher lives in liblbft_commit_times.so, NULL and zero arguments are refused before any HIP call, the Python methods
check their arguments before any library call, the new kernel is in the side library's code object without scratch, and the grid tool
parses its new options and leaves its output alone without them."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

from support import Stub, hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lbft_batch_commit_series", "lbft_batch_commit_stalls")


def test_timeline_symbols_are_declared_and_exported(hiplib):
    from librabft_simulator_amd import build
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    raw = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in hiplib.ABI_SYMBOLS, name
        assert hasattr(raw, name), name
    assert re.search(r"#define LBFT_STALL_STATS 16\b", header) and hiplib.STALL_STATS == 16
    side = ctypes.CDLL(build.CT_OUT)
    assert hasattr(side, "lbft_ct_launch_timeline")
    for other in (hiplib.LIB_PATH, *other_libs("commit_times")):
        assert not hasattr(ctypes.CDLL(other), "lbft_ct_launch_timeline"), other
    assert "lbft_ct_timeline_fn" in open(os.path.join(ROOT, "librabft_simulator_amd", "csrc", "lbft_commit_times.h")).read()


def test_arguments_are_refused_without_a_gpu(hiplib):
    L = hiplib.lib()
    hist = np.zeros(16, dtype=np.uint64)
    stats = np.zeros(16, dtype=np.uint64)
    since = np.zeros(1, dtype=np.int64)
    for width, bins in ((1, 16), (0, 16), (1, 0), (0, 0)):
        assert L.lbft_batch_commit_series(None, width, bins, hist.ctypes.data) == hiplib.LBFT_ERR_INVALID
        assert L.lbft_batch_commit_series(None, width, bins, None) == hiplib.LBFT_ERR_INVALID
        for s in (None, since.ctypes.data):
            assert L.lbft_batch_commit_stalls(None, s, width, bins, hist.ctypes.data, stats.ctypes.data) == hiplib.LBFT_ERR_INVALID
            assert L.lbft_batch_commit_stalls(None, s, width, bins, None, None) == hiplib.LBFT_ERR_INVALID
    assert not hist.any() and not stats.any()


def test_python_methods_refuse_bad_arguments_before_the_device():
    from librabft_simulator_amd.simulator import BatchResult
    res = BatchResult(Stub())
    for kw in ({"bins": 0}, {"bin_width": 0}, {"bin_width": 0, "bins": 0}, {"bins": -3}):
        with pytest.raises(ValueError):
            res.commit_series(**kw)
        with pytest.raises(ValueError):
            res.stall_histogram(**kw)
    for since in (-1, 1001, [0, 0], [], "partition_start", [1001]):
        with pytest.raises(ValueError):
            res.stall_histogram(since=since)
        with pytest.raises(ValueError):
            res.stalls_by_param_set(since=since)


def test_since_forms():
    from librabft_simulator_amd.simulator import BatchResult, ParamSet

    class Sets(Stub):
        param_sets = [ParamSet(), ParamSet(partition=(2, 300, 600)), ParamSet(partition=(1, 100, 5000)), ParamSet(partition=(0, 10, 20))]
    res = BatchResult(Sets())
    assert res._since(None) is None
    assert res._since(7).tolist() == [7, 7, 7, 7]
    assert res._since([0, 1, 2, 1000]).tolist() == [0, 1, 2, 1000]
    assert res._since("partition_end").tolist() == [0, 600, 1000, 0]  # clipped to max_clock; 0 without a partition
    assert res._since("partition_end").dtype == np.int64
    with pytest.raises(ValueError):
        res._since([0, 1, 2])

    class Plain(Stub):
        partition = (2, 300, 600)
    assert BatchResult(Plain())._since("partition_end").tolist() == [600]
    assert BatchResult(Stub())._since("partition_end").tolist() == [0]
    assert BatchResult(Stub())._binning(None, None) == (1, 1001)
    assert BatchResult(Stub())._binning(None, 10) == (101, 10)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_timeline_kernel_is_in_the_side_library_without_scratch(hiplib):
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    ct = _kernel_metadata(build.CT_OUT)
    mine = [v for k, v in ct.items() if re.search(r"\d+lbft_k_ct_timelineN", k)]
    assert len(mine) == 1, sorted(ct)
    assert mine[0]["private_segment_fixed_size"] == 0, mine[0]
    assert not any("run0" in k or "run1" in k for k in ct if "timeline" in k)
    for other in other_libs("commit_times"):
        assert not any("timeline" in k for k in _kernel_metadata(other)), other


def test_grid_options():
    from librabft_simulator_amd import grid
    assert grid._partitions("2:300:600") == [(2, 300, 600)]
    assert grid._partitions("none,2:300:600, 1:0:50") == [None, (2, 300, 600), (1, 0, 50)]
    assert grid._partitions("NONE") == [None]
    for bad in ("", "2:300", "2:300:600:7", "a:b:c", "2-300-600"):
        with pytest.raises(argparse.ArgumentTypeError):
            grid._partitions(bad)

    class Args:
        mean, variance, delta, gamma, lambda_, target_commit_interval, drop_per_million = [10.0], [4.0], [10, 20], [2.0], [0.5], [100000], [0]
        partition = None
    plain = grid.grid_points(Args())
    assert len(plain) == 2 and all("partition" not in pt for pt in plain)
    assert list(plain[0]) == ["mean", "variance", "delta", "gamma", "lambda", "target_commit_interval", "drop_per_million"]
    Args.partition = [None, (2, 300, 600)]
    pts = grid.grid_points(Args())
    assert [(pt["delta"], pt["partition"]) for pt in pts] == [(10, None), (10, (2, 300, 600)), (20, None), (20, (2, 300, 600))]
    # a bad option ends the tool before it creates a batch
    for argv in (["--series", "0"], ["--partition", "2:300"]):
        with pytest.raises(SystemExit):
            grid.main(argv)
