"""CPU-side checks of the vote statistics (lbft_batch_vote_stats): the entry point is declared, exported and bound, the launcher lives in
liblbft_paramsets.so alone and is in build.TABLE's row, NULL arguments and a zero binning are refused before any HIP call with the outputs
untouched, the Python methods check their arguments before any library call, the grid tool parses --votes, the kernel is in the
parameter-set library's code object exactly once and without scratch, the rule header needs <stdint.h> and lbft_group_stats.h alone, and
liblbft_hip.so's machine code is still the committed manifest's."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from support import Stub, hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "librabft_simulator_amd", "csrc")
NAME, KERNEL, LAUNCHER = "lbft_batch_vote_stats", "lbft_k_ps_votes", "lbft_ps_launch_votes"


def test_symbol_is_declared_exported_and_bound(hiplib):
    import vote_stats_reference as ref
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    assert NAME in declared and NAME in hiplib.ABI_SYMBOLS and hasattr(ctypes.CDLL(hiplib.LIB_PATH), NAME)
    assert len(hiplib.lib().lbft_batch_vote_stats.argtypes) == 7
    for macro, value in (("LBFT_VOTE_FAMILIES", 8), ("LBFT_VOTE_STATS", 32), ("LBFT_VOTE_NODE_COLUMNS", 3)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert hiplib.VOTE_STATS == 32 == ref.VOTE_STATS == 4 * len(hiplib.VOTE_FAMILIES) and hiplib.VOTE_FAMILIES == ref.FAMILIES
    assert hiplib.VOTE_NODE_COLUMNS == ("proposed", "orphaned", "voted") and len(hiplib.VOTE_NODE_COLUMNS) == ref.NODE_COLUMNS


def test_launcher_is_in_the_table_and_exported_by_the_paramsets_library_alone(hiplib):
    from librabft_simulator_amd import build
    assert LAUNCHER in dict((lib.tag, lib.launchers) for lib in build.TABLE)["paramsets"]
    assert hasattr(ctypes.CDLL(build.PS_OUT), LAUNCHER)
    for other in other_libs("paramsets"):
        assert not hasattr(ctypes.CDLL(other), LAUNCHER), other
    assert "lbft_ps_votes_fn" in open(os.path.join(CSRC, "lbft_paramsets.h")).read()
    # the launcher is looked up with the library's others: a file without it is refused as a whole
    text = open(os.path.join(CSRC, "lbft_hip.hip")).read()
    call = text[text.index("static int load_paramsets_lib()"):]
    assert '"%s"' % LAUNCHER in call[:call.index("\n}\n")]
    # the rule header is the parameter-set library's alone and needs nothing of the device
    header = os.path.join(CSRC, "lbft_vote_rules.h")
    assert header in build.PS_DEPS
    for deps in (build.DEPS, build.CT_DEPS, build.RS_DEPS, build.CS_DEPS, build.RH_DEPS):
        assert header not in deps
    rules = open(header).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", rules)) == ["lbft_group_stats.h", "stdint.h"]
    assert "__shfl" not in rules and "__ballot" not in rules and "threadIdx" not in rules
    # the main library gets host code only
    assert not re.search(r"__global__[^;{]*\b%s\b" % KERNEL, text) and "<<<" not in text[text.index("int %s(" % NAME):][:2000].split("\n}\n")[0]


def test_refusals_come_before_any_hip_call_with_the_outputs_untouched(hiplib):
    L = hiplib.lib()
    outs = [np.full(k, 77, np.uint64) for k in (16, 5, 12, 32)]
    p = [a.ctypes.data for a in outs]
    fake = ctypes.c_void_p(outs[0].ctypes.data)  # never dereferenced: these refusals come before the handle is looked at
    for width, bins in ((1, 16), (0, 16), (1, 0), (0, 0)):
        assert L.lbft_batch_vote_stats(None, width, bins, *p) == hiplib.LBFT_ERR_INVALID
        for k in range(4):
            args = list(p)
            args[k] = None
            assert L.lbft_batch_vote_stats(fake, width, bins, *args) == hiplib.LBFT_ERR_INVALID, k
    for width, bins in ((0, 16), (1, 0)):
        assert L.lbft_batch_vote_stats(fake, width, bins, *p) == hiplib.LBFT_ERR_INVALID
    assert all((a == 77).all() for a in outs)


def test_refusals_are_ordered_in_the_source():
    """lbft_batch_chain_stats' order: the arguments and the binning, then the state, all before the library is opened and the device is
    set (a batch that has run needs a device: tests/test_vote_stats_gpu.py observes the order there)."""
    text = open(os.path.join(CSRC, "lbft_hip.hip")).read()
    fn = text[text.index("int %s(" % NAME):]
    fn = fn[:fn.index("\n}\n")]
    order = [fn.index(s) for s in ("refuse_grouped(b, margin_hist && votes_hist && node_table && stats, bin_width, bins, false)", "load_paramsets_lib()",
                                   "hipSetDevice", "GroupedCall gc(b)", "g_ps_votes(")]
    assert order == sorted(order)
    chain = text[text.index("int lbft_batch_chain_stats("):]
    assert "refuse_grouped(b, interval_hist && author_blocks && stats, bin_width, bins, false)" in chain[:chain.index("\n}\n")]


def test_python_methods_refuse_bad_binning_before_the_device():
    from librabft_simulator_amd.simulator import BatchResult
    res = BatchResult(Stub())
    for kw in ({"bins": 0}, {"bin_width": 0}, {"bins": -3}, {"bin_width": -1}, {"bin_width": 0, "bins": 4}):
        with pytest.raises(ValueError):
            res.vote_stats(**kw)
    assert callable(res.votes_by_param_set)


def test_grid_votes_option_is_parsed():
    from librabft_simulator_amd import grid
    with pytest.raises(SystemExit):  # a bad option ends the tool before it creates a batch
        grid.main(["--votes", "--seeds-per-point", "0"])
    with pytest.raises(SystemExit):
        grid.main(["--votes=yes"])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_kernel_is_in_the_paramsets_library_alone_and_uses_no_scratch(hiplib):
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    ps = _kernel_metadata(build.PS_OUT)
    mine = [v for k, v in ps.items() if re.search(r"\d+%sN" % KERNEL, k)]
    assert len(mine) == 1, sorted(ps)
    print(mine[0])
    assert mine[0]["private_segment_fixed_size"] == 0 and mine[0]["vgpr_spill_count"] == 0, mine[0]
    # (256 lanes per workgroup: 128 registers keep four wavefronts per SIMD; the margin histogram and the small tables fit 24 KiB of LDS)
    assert mine[0]["vgpr_count"] <= 128 and mine[0]["group_segment_fixed_size"] <= 24 * 1024, mine[0]
    assert not any("_run" in k for k in ps if KERNEL in k)
    for other in other_libs("paramsets"):
        assert not any(KERNEL in k for k in _kernel_metadata(other)), other


def test_the_main_library_keeps_its_machine_code(hiplib):
    from librabft_simulator_amd import build
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.json")))
    assert build.kernel_hash(build.OUT) == committed["kernel_hash"]
