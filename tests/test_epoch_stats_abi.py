"""CPU-side checks of the epoch statistics (lbft_batch_epoch_stats): the entry point is declared, exported and bound, the launcher lives in
liblbft_paramsets.so alone and is in build.TABLE's row, NULL arguments, a zero binning and epoch_bins of 0 or above 512 are refused before
any HIP call with the outputs untouched, the Python methods check their arguments before any library call, the grid tool parses --epochs,
the kernel is in the parameter-set library's code object exactly once and within its budget, the rule header needs <stdint.h> and
lbft_group_stats.h alone, and liblbft_hip.so's machine code is still the committed manifest's."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from support import Stub, hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "librabft_simulator_amd", "csrc")
NAME, KERNEL, LAUNCHER = "lbft_batch_epoch_stats", "lbft_k_ps_epochs", "lbft_ps_launch_epochs"


def test_symbol_is_declared_exported_and_bound(hiplib):
    import epoch_stats_reference as ref
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    assert NAME in declared and NAME in hiplib.ABI_SYMBOLS and hasattr(ctypes.CDLL(hiplib.LIB_PATH), NAME)
    assert len(hiplib.lib().lbft_batch_epoch_stats.argtypes) == 7
    for macro, value in (("LBFT_EPOCH_FAMILIES", 10), ("LBFT_EPOCH_STATS", 40), ("LBFT_EPOCH_COLUMNS", 7), ("LBFT_EPOCH_MAX_BINS", 512)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert hiplib.EPOCH_STATS == 40 == ref.EPOCH_STATS == 4 * len(hiplib.EPOCH_FAMILIES) and hiplib.EPOCH_FAMILIES == ref.FAMILIES
    assert hiplib.EPOCH_COLUMNS == ref.COLUMNS and len(hiplib.EPOCH_COLUMNS) == 7 and hiplib.EPOCH_MAX_BINS == ref.MAX_BINS == 512
    # the rule header's enums are the macros' (a static_assert beside the kernel holds them together at build time)
    rules = open(os.path.join(CSRC, "lbft_epoch_rules.h")).read()
    assert "EP_FAMILIES = 10" in rules and "EP_COLUMNS = 7" in rules and re.search(r"#define EP_MAX_BINS 512u\b", rules)
    assert "static_assert(LBFT_EPOCH_STATS == EP_FAMILIES * 4" in open(os.path.join(CSRC, "lbft_paramsets.hip")).read()


def test_launcher_is_in_the_table_and_exported_by_the_paramsets_library_alone(hiplib):
    from librabft_simulator_amd import build
    assert LAUNCHER in dict((lib.tag, lib.launchers) for lib in build.TABLE)["paramsets"]
    assert hasattr(ctypes.CDLL(build.PS_OUT), LAUNCHER)
    for other in other_libs("paramsets"):
        assert not hasattr(ctypes.CDLL(other), LAUNCHER), other
    assert "lbft_ps_epochs_fn" in open(os.path.join(CSRC, "lbft_paramsets.h")).read()
    # the launcher is looked up with the library's others: a file without it is refused as a whole
    text = open(os.path.join(CSRC, "lbft_hip.hip")).read()
    call = text[text.index("static int load_paramsets_lib()"):]
    assert '"%s"' % LAUNCHER in call[:call.index("\n}\n")]
    # the rule header is the parameter-set library's alone and needs nothing of the device
    header = os.path.join(CSRC, "lbft_epoch_rules.h")
    assert header in build.PS_DEPS
    for deps in (build.DEPS, build.CT_DEPS, build.RS_DEPS, build.CS_DEPS, build.RH_DEPS):
        assert header not in deps
    rules = open(header).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", rules)) == ["lbft_group_stats.h", "stdint.h"]
    assert "__shfl" not in rules and "__ballot" not in rules and "threadIdx" not in rules and "atomic" not in rules
    # the main library gets host code only
    assert not re.search(r"__global__[^;{]*\b%s\b" % KERNEL, text) and "<<<" not in text[text.index("int %s(" % NAME):][:2500].split("\n}\n")[0]


def test_refusals_come_before_any_hip_call_with_the_outputs_untouched(hiplib):
    L = hiplib.lib()
    outs = [np.full(k, 77, np.uint64) for k in (16, 7 * 8, 40)]
    p = [a.ctypes.data for a in outs]
    fake = ctypes.c_void_p(outs[0].ctypes.data)  # never dereferenced: these refusals come before the handle is looked at
    for width, bins, epoch_bins in ((1, 16, 8), (0, 16, 8), (1, 0, 8), (1, 16, 0), (0, 0, 0), (1, 16, 513)):
        assert L.lbft_batch_epoch_stats(None, width, bins, epoch_bins, *p) == hiplib.LBFT_ERR_INVALID
        for k in range(3):
            args = list(p)
            args[k] = None
            assert L.lbft_batch_epoch_stats(fake, width, bins, epoch_bins, *args) == hiplib.LBFT_ERR_INVALID, k
    for width, bins, epoch_bins in ((0, 16, 8), (1, 0, 8), (1, 16, 0), (1, 16, 513), (1, 16, 2 ** 32 - 1)):
        assert L.lbft_batch_epoch_stats(fake, width, bins, epoch_bins, *p) == hiplib.LBFT_ERR_INVALID
    assert all((a == 77).all() for a in outs)


def test_refusals_are_ordered_in_the_source():
    """lbft_batch_vote_stats' order: the arguments, the binning and epoch_bins, then the state, all before the library is opened and the
    device is set (a batch that has run needs a device: tests/test_epoch_stats_gpu.py observes the order there)."""
    text = open(os.path.join(CSRC, "lbft_hip.hip")).read()
    fn = text[text.index("int %s(" % NAME):]
    fn = fn[:fn.index("\n}\n")]
    order = [fn.index(s) for s in ("handover_hist && epoch_table && stats && epoch_bins != 0", "epoch_bins > LBFT_EPOCH_MAX_BINS", "refuse_grouped(b, args_ok, bin_width, bins, false)",
                                   "load_paramsets_lib()", "hipSetDevice", "GroupedCall gc(b)", "g_ps_epochs(")]
    assert order == sorted(order)
    votes = text[text.index("int lbft_batch_vote_stats("):]
    assert "refuse_grouped(b, margin_hist && votes_hist && node_table && stats, bin_width, bins, false)" in votes[:votes.index("\n}\n")]


def test_python_methods_refuse_bad_arguments_before_the_device():
    from librabft_simulator_amd.simulator import BatchResult
    res = BatchResult(Stub())
    for kw in ({"bins": 0}, {"bin_width": 0}, {"bins": -3}, {"bin_width": -1}, {"bin_width": 0, "bins": 4}, {"epoch_bins": 0}, {"epoch_bins": 513},
               {"epoch_bins": -1}):
        with pytest.raises(ValueError):
            res.epoch_stats(**kw)
    for kw in ({"epoch_bins": 0}, {"epoch_bins": 513}):
        with pytest.raises(ValueError):
            res.epochs_by_param_set(**kw)
    # the default binning covers [0, max_clock] in at most 4 096 bins
    assert res._epoch_binning(None, None) == (1, 1001)
    stub = Stub()
    stub._max_clock = 5000
    assert BatchResult(stub)._epoch_binning(None, None) == (2, 2501) and BatchResult(stub)._epoch_binning(1, None) == (1, 5001)
    stub._max_clock = 4095
    assert BatchResult(stub)._epoch_binning(None, None) == (1, 4096)


def test_grid_epochs_option_is_parsed():
    from librabft_simulator_amd import grid
    with pytest.raises(SystemExit):  # a bad option ends the tool before it creates a batch
        grid.main(["--epochs", "--commands-per-epoch", "5", "--seeds-per-point", "0"])
    with pytest.raises(SystemExit):
        grid.main(["--epochs=yes"])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_kernel_is_in_the_paramsets_library_alone_and_within_its_budget(hiplib):
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    ps = _kernel_metadata(build.PS_OUT)
    mine = [v for k, v in ps.items() if re.search(r"\d+%sN" % KERNEL, k)]
    assert len(mine) == 1, sorted(ps)
    print(mine[0])
    assert mine[0]["private_segment_fixed_size"] == 0 and mine[0]["vgpr_spill_count"] == 0, mine[0]
    # 256 lanes per workgroup: 128 registers keep four wavefronts per SIMD.  LDS: the handover histogram (16 KiB), 512 x 7 x 4 B for the
    # epoch table and the statistics' 40 x 8 B
    assert mine[0]["vgpr_count"] <= 128 and mine[0]["group_segment_fixed_size"] <= 16 * 1024 + 512 * 7 * 4 + 40 * 8, mine[0]
    assert not any("_run" in k for k in ps if KERNEL in k)
    for other in other_libs("paramsets"):
        assert not any(KERNEL in k for k in _kernel_metadata(other)), other


def test_the_main_library_keeps_its_machine_code(hiplib):
    from librabft_simulator_amd import build
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.json")))
    assert build.kernel_hash(build.OUT) == committed["kernel_hash"]
