"""CPU-side checks of the round statistics (lbft_batch_round_stats / lbft_batch_round_switches_all): the entry points are declared,
exported and bound, the launcher lives in liblbft_round_stats.so alone, NULL and zero arguments are refused before any HIP call, the
Python methods check their arguments before any library call, the new kernel is in the side library's code object exactly once and
without scratch, and liblbft_hip.so's machine code is still the committed manifest's."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from support import Stub, hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lbft_batch_round_stats", "lbft_batch_round_switches_all")


def test_round_stats_symbols_are_declared_and_exported(hiplib):
    from librabft_simulator_amd import build
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    raw = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in hiplib.ABI_SYMBOLS, name
        assert hasattr(raw, name), name
        assert getattr(hiplib.lib(), name).argtypes is not None, name
    assert re.search(r"#define LBFT_ROUND_STATS 16\b", header) and hiplib.ROUND_STATS == 16
    assert (build.RS_SRC, build.RS_OUT, build.RS_DEPS) in build.LIBS and os.path.basename(build.RS_OUT) == "liblbft_round_stats.so"
    assert hasattr(ctypes.CDLL(build.RS_OUT), "lbft_rs_launch_rounds")
    for other in (hiplib.LIB_PATH, *other_libs("round_stats")):
        assert not hasattr(ctypes.CDLL(other), "lbft_rs_launch_rounds"), other
    csrc = os.path.join(ROOT, "librabft_simulator_amd", "csrc")
    assert "lbft_rs_rounds_fn" in open(os.path.join(csrc, "lbft_round_stats.h")).read()
    # the reference's pass size is the kernel's
    import round_stats_reference as ref
    assert re.search(r"#define LBFT_RS_LDS_BINS %d\b" % ref.LDS_BINS, open(os.path.join(csrc, "lbft_round_stats.hip")).read())


def test_arguments_are_refused_without_a_gpu(hiplib):
    L = hiplib.lib()
    stay = np.zeros(16, dtype=np.uint64)
    skew = np.zeros(16, dtype=np.uint64)
    stats = np.zeros(16, dtype=np.uint64)
    p = [a.ctypes.data for a in (stay, skew, stats)]
    for width, bins in ((1, 16), (0, 16), (1, 0), (0, 0)):
        assert L.lbft_batch_round_stats(None, width, bins, *p) == hiplib.LBFT_ERR_INVALID
        assert L.lbft_batch_round_stats(None, width, bins, None, None, None) == hiplib.LBFT_ERR_INVALID
    out = np.zeros(16, dtype=np.int64)
    mr = np.zeros(4, dtype=np.uint64)
    assert L.lbft_batch_round_switches_all(None, out.ctypes.data, 4, mr.ctypes.data, None) == hiplib.LBFT_ERR_INVALID
    assert L.lbft_batch_round_switches_all(None, None, 4, None, None) == hiplib.LBFT_ERR_INVALID
    assert not stay.any() and not skew.any() and not stats.any() and not out.any()


def test_python_methods_refuse_bad_arguments_before_the_device():
    from librabft_simulator_amd.simulator import BatchResult
    res = BatchResult(Stub())
    for kw in ({"bins": 0}, {"bin_width": 0}, {"bin_width": 0, "bins": 0}, {"bins": -3}):
        with pytest.raises(ValueError):
            res.round_histogram(**kw)
    with pytest.raises(ValueError):
        res.round_tables(cap_rounds=-1)


def test_grid_rounds_option_is_parsed():
    from librabft_simulator_amd import grid
    for argv in (["--rounds", "--round-trace", "0"], ["--round-trace", "-5"]):  # a bad option ends the tool before it creates a batch
        with pytest.raises(SystemExit):
            grid.main(argv)
    assert grid.round_trace_capacity(1000, None) == 264 and grid.round_trace_capacity(1000, 77) == 77
    assert grid.round_trace_capacity(10 ** 6, None) == 1 << 16


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_round_stats_kernel_is_in_its_own_library_without_scratch(hiplib):
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    assert os.path.exists(build.RS_OUT)
    rs = _kernel_metadata(build.RS_OUT)
    mine = [v for k, v in rs.items() if re.search(r"\d+lbft_k_rs_roundsN", k)]
    assert len(mine) == 1 and len([k for k in rs if "lbft_k_rs_" in k]) == 1, sorted(rs)
    assert mine[0]["private_segment_fixed_size"] == 0 and mine[0]["vgpr_spill_count"] == 0, mine[0]
    assert not any("lbft_k_run" in k or "lbft_k_ct_" in k or "lbft_k_ps_" in k for k in rs), sorted(rs)
    for other in other_libs("round_stats"):
        assert not any("lbft_k_rs_" in k for k in _kernel_metadata(other)), other


def test_the_main_library_keeps_its_machine_code(hiplib):
    from librabft_simulator_amd import build
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.json")))
    assert build.kernel_hash(build.OUT) == committed["kernel_hash"]
    assert build.kernel_hash(build.RS_OUT) != committed["kernel_hash"]
