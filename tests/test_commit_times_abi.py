"""CPU-side checks of commit-time recording (lbft_batch_record_commit_times): the entry points are declared and exported, NULL and
zero-bin arguments are refused before any HIP call, the run kernels and the histogram kernel are built into a code object of their own
(liblbft_commit_times.so) with no more scratch than the kernels they twin, and liblbft_hip.so's machine code is still the one the
committed codegen manifest pins."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from support import Stub, hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lbft_batch_record_commit_times", "lbft_batch_commit_times", "lbft_batch_commit_latency_histogram")


def test_commit_time_symbols_are_declared_and_exported(hiplib):
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    raw = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in hiplib.ABI_SYMBOLS, name
        assert hasattr(raw, name), name
    # the launchers live in the side library, not in liblbft_hip.so
    from librabft_simulator_amd import build
    side = ctypes.CDLL(build.CT_OUT)
    assert hasattr(side, "lbft_ct_launch_run") and hasattr(side, "lbft_ct_launch_histogram")
    for other in (hiplib.LIB_PATH, *other_libs("commit_times")):
        assert not hasattr(ctypes.CDLL(other), "lbft_ct_launch_run"), other


def test_arguments_are_refused_without_a_gpu(hiplib):
    L = hiplib.lib()
    hist = np.zeros(16, dtype=np.uint64)
    stats = np.zeros(4, dtype=np.uint64)
    out = np.zeros(16, dtype=np.int64)
    assert L.lbft_batch_record_commit_times(None, 1) == hiplib.LBFT_ERR_INVALID
    assert L.lbft_batch_commit_times(None, out.ctypes.data, 4) == hiplib.LBFT_ERR_INVALID
    for width, bins in ((1, 16), (0, 16), (1, 0), (0, 0)):
        assert L.lbft_batch_commit_latency_histogram(None, width, bins, hist.ctypes.data, stats.ctypes.data) == hiplib.LBFT_ERR_INVALID
        assert L.lbft_batch_commit_latency_histogram(None, width, bins, None, None) == hiplib.LBFT_ERR_INVALID


def test_python_histogram_refuses_zero_bins_before_the_device():
    from librabft_simulator_amd.simulator import BatchResult
    res = BatchResult(Stub())
    for kw in ({"bins": 0}, {"bin_width": 0}, {"bin_width": 0, "bins": 0}, {"bins": -3}):
        with pytest.raises(ValueError):
            res.latency_histogram(**kw)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_commit_time_kernels_are_a_separate_code_object_without_extra_scratch(hiplib):
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    assert os.path.exists(build.CT_OUT)
    ct = _kernel_metadata(build.CT_OUT)
    names = sorted(ct)
    want = ("lbft_k_ct_run0", "lbft_k_ct_run1", "lbft_k_ct_ps_run0", "lbft_k_ct_ps_run1", "lbft_k_ct_latency_hist")
    for w in want:
        assert sum(1 for k in names if re.search(r"\d%sN" % w, k)) == 1, (w, names)
    base = _kernel_metadata(build.OUT)
    run0 = [v for k, v in base.items() if re.search(r"lbft_k_run0N", k)]
    run1 = [v for k, v in base.items() if "lbft_k_runILi1E" in k]
    assert len(run0) == 1 and len(run1) == 1, sorted(base)
    for k, v in ct.items():
        cap = run0[0] if "run0" in k else run1[0] if "run1" in k else {"private_segment_fixed_size": 0}
        assert v["private_segment_fixed_size"] <= cap["private_segment_fixed_size"], (k, v, cap)
    # none of them went into liblbft_hip.so or into another side library
    for other in other_libs("commit_times"):
        assert not any("lbft_k_ct_" in k for k in _kernel_metadata(other)), other


def test_main_library_machine_code_is_unchanged(hiplib):
    from librabft_simulator_amd import build
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.json")))
    assert build.kernel_hash(build.OUT) == committed["kernel_hash"]
    assert build.kernel_hash(build.CT_OUT) != committed["kernel_hash"]
