"""CPU-side checks of commit finality (lbft_batch_commit_finality): the entry point is declared, exported and bound, the launcher lives
in liblbft_commit_times.so alone, NULL and zero arguments are refused before any HIP call, the Python methods check their arguments
before any library call, the grid tool knows the option, the new kernel is in the side library's code object exactly once, without
scratch and with an LDS footprint that lets two workgroups share a compute unit, and liblbft_hip.so's machine code is still the
committed manifest's."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from support import Stub, hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "librabft_simulator_amd", "csrc")
NAME = "lbft_batch_commit_finality"


def test_finality_symbol_is_declared_exported_and_bound(hiplib):
    from librabft_simulator_amd import build
    import commit_finality_reference as ref
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    assert NAME in declared and NAME in hiplib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(hiplib.LIB_PATH), NAME)
    assert len(getattr(hiplib.lib(), NAME).argtypes) == 7
    assert re.search(r"#define LBFT_FINALITY_STATS 24\b", header) and hiplib.FINALITY_STATS == 24 == ref.FINALITY_STATS == 4 * ref.FAMILIES
    # the launcher: in the commit-time library, in no other, in the table and in the typedefs
    assert "lbft_ct_launch_finality" in build.TABLE[2].launchers and build.TABLE[2].tag == "commit_times"
    assert hasattr(ctypes.CDLL(build.CT_OUT), "lbft_ct_launch_finality")
    for other in (hiplib.LIB_PATH, *other_libs("commit_times")):
        assert not hasattr(ctypes.CDLL(other), "lbft_ct_launch_finality"), other
    assert "lbft_ct_finality_fn" in open(os.path.join(CSRC, "lbft_commit_times.h")).read()
    rules = os.path.join(CSRC, "lbft_commit_finality.h")
    assert rules in build.CT_DEPS and rules not in build.DEPS  # liblbft_hip.so includes nothing of it: its device code stays as it is
    # the reference's pass size is the kernel's, the rules need nothing of the device
    assert re.search(r"#define LBFT_FN_LDS_BINS %d\b" % ref.LDS_BINS, open(os.path.join(CSRC, "lbft_commit_times.hip")).read())
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", open(rules).read())
    assert sorted(includes) == ["lbft_group_stats.h", "stdint.h"]
    enum = re.search(r"enum \{ FIN_FIRST = 0, FIN_VALID = 1, FIN_QUORUM = 2, FIN_ALL = 3, FIN_SPREAD = 4, FIN_OPEN = 5, FIN_FAMILIES = 6 \}", open(rules).read())
    assert enum and (ref.FIRST, ref.VALID, ref.QUORUM, ref.ALL, ref.SPREAD, ref.OPEN) == (0, 1, 2, 3, 4, 5)


def test_arguments_are_refused_without_a_gpu(hiplib):
    L = hiplib.lib()
    fin, spread = np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    first, stats = np.zeros(4, dtype=np.uint64), np.zeros(24, dtype=np.uint64)
    p = [a.ctypes.data for a in (fin, spread, first, stats)]
    for width, bins in ((1, 16), (0, 16), (1, 0), (0, 0)):
        assert getattr(L, NAME)(None, width, bins, *p) == hiplib.LBFT_ERR_INVALID
        assert getattr(L, NAME)(None, width, bins, None, None, None, None) == hiplib.LBFT_ERR_INVALID
    assert not fin.any() and not spread.any() and not first.any() and not stats.any()


def test_python_methods_refuse_bad_arguments_before_the_device():
    from librabft_simulator_amd.simulator import BatchResult
    res = BatchResult(Stub())
    for kw in ({"bins": 0}, {"bin_width": 0}, {"bin_width": 0, "bins": 0}, {"bins": -3}, {"bin_width": -1}):
        with pytest.raises(ValueError):
            res.finality_histogram(**kw)
    assert callable(res.finality_by_param_set)


def test_grid_finality_option_is_parsed():
    from librabft_simulator_amd import grid
    with pytest.raises(SystemExit):  # a bad option ends the tool before it creates a batch
        grid.main(["--finality", "--seeds-per-point", "0"])
    with pytest.raises(SystemExit):
        grid.main(["--finality=yes"])
    assert "--finality" in grid.__doc__


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_finality_kernel_is_in_the_commit_time_library_without_scratch(hiplib):
    """LDS: a compute unit has 160 KiB, so two workgroups share it when each takes at most 80 KiB.  The kernel's own sum: the tile of 4
    wavefronts x 32 nodes x 64 entries x 4 B = 32 KiB, two histograms of 4096 u32 bins = 32 KiB, 32 first-committer bins and 32 rights =
    256 B, 24 statistics words = 192 B: 65 984 B."""
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    ct = _kernel_metadata(build.CT_OUT)
    mine = [(k, v) for k, v in ct.items() if re.search(r"\d+lbft_k_ct_finalityN", k)]
    assert len(mine) == 1 and len([k for k in ct if "finality" in k]) == 1, sorted(ct)
    name, meta = mine[0]
    assert "_run" not in name and "run0" not in name and "run1" not in name
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
    assert meta["group_segment_fixed_size"] == 4 * 32 * 64 * 4 + 2 * 4096 * 4 + 2 * 32 * 4 + 24 * 8 <= 80 * 1024, meta
    assert meta["vgpr_count"] <= 256, meta  # two wavefronts per SIMD, what the LDS admits
    for other in other_libs("commit_times"):
        assert not any("finality" in k for k in _kernel_metadata(other)), other


def test_the_main_library_keeps_its_machine_code(hiplib):
    from librabft_simulator_amd import build
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.json")))
    assert build.kernel_hash(build.OUT) == committed["kernel_hash"]
    assert build.kernel_hash(build.CT_OUT) != committed["kernel_hash"]
