"""CPU-side checks of the chain statistics (lbft_batch_chain_stats): the entry point is declared, exported and bound, the launcher lives
in liblbft_chain_stats.so alone, NULL and zero arguments are refused before any HIP call, the Python methods check their arguments before
any library call, the new kernel is in the side library's code object exactly once and without scratch, and liblbft_hip.so's machine
code is still the committed manifest's."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

from support import Stub, hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lbft_batch_chain_stats"


def test_chain_stats_symbol_is_declared_exported_and_bound(hiplib):
    from librabft_simulator_amd import build
    import chain_stats_reference as ref
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    assert NAME in declared and NAME in hiplib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(hiplib.LIB_PATH), NAME)
    assert len(getattr(hiplib.lib(), NAME).argtypes) == 6
    assert re.search(r"#define LBFT_CHAIN_STATS 24\b", header) and hiplib.CHAIN_STATS == 24 == ref.CHAIN_STATS == 4 * ref.FAMILIES
    assert (build.CS_SRC, build.CS_OUT, build.CS_DEPS) in build.LIBS and os.path.basename(build.CS_OUT) == "liblbft_chain_stats.so"
    assert hasattr(ctypes.CDLL(build.CS_OUT), "lbft_cs_launch_chain")
    for other in (hiplib.LIB_PATH, *other_libs("chain_stats")):
        assert not hasattr(ctypes.CDLL(other), "lbft_cs_launch_chain"), other
    csrc = os.path.join(ROOT, "librabft_simulator_amd", "csrc")
    assert "lbft_cs_chain_fn" in open(os.path.join(csrc, "lbft_chain_stats.h")).read()
    assert os.path.join(csrc, "lbft_chain_stats.h") in build.DEPS and os.path.join(csrc, "lbft_chain_rules.h") in build.CS_DEPS
    # the reference's pass size is the kernel's, the rules need nothing of the device
    assert re.search(r"#define LBFT_CS_LDS_BINS %d\b" % ref.LDS_BINS, open(os.path.join(csrc, "lbft_chain_stats.hip")).read())
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", open(os.path.join(csrc, "lbft_chain_rules.h")).read())
    assert sorted(includes) == ["lbft_group_stats.h", "stdint.h"]


def test_arguments_are_refused_without_a_gpu(hiplib):
    L = hiplib.lib()
    hist = np.zeros(16, dtype=np.uint64)
    authors = np.zeros(4, dtype=np.uint64)
    stats = np.zeros(24, dtype=np.uint64)
    p = [a.ctypes.data for a in (hist, authors, stats)]
    for width, bins in ((1, 16), (0, 16), (1, 0), (0, 0)):
        assert L.lbft_batch_chain_stats(None, width, bins, *p) == hiplib.LBFT_ERR_INVALID
        assert L.lbft_batch_chain_stats(None, width, bins, None, None, None) == hiplib.LBFT_ERR_INVALID
    assert not hist.any() and not authors.any() and not stats.any()


def test_python_methods_refuse_bad_arguments_before_the_device():
    from librabft_simulator_amd.simulator import BatchResult
    res = BatchResult(Stub())
    for kw in ({"bins": 0}, {"bin_width": 0}, {"bin_width": 0, "bins": 0}, {"bins": -3}, {"bin_width": -1}):
        with pytest.raises(ValueError):
            res.chain_stats(**kw)


def test_grid_chain_option_is_parsed():
    from librabft_simulator_amd import grid
    with pytest.raises(SystemExit):  # a bad option ends the tool before it creates a batch
        grid.main(["--chain", "--seeds-per-point", "0"])
    with pytest.raises(SystemExit):
        grid.main(["--chain=yes"])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_chain_stats_kernel_is_in_its_own_library_without_scratch(hiplib, capsys):
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    assert os.path.exists(build.CS_OUT)
    cs = _kernel_metadata(build.CS_OUT)
    mine = [v for k, v in cs.items() if re.search(r"\d+lbft_k_cs_chainN", k)]
    assert len(mine) == 1 and len([k for k in cs if "lbft_k_cs_" in k]) == 1, sorted(cs)
    assert mine[0]["private_segment_fixed_size"] == 0 and mine[0]["vgpr_spill_count"] == 0, mine[0]
    assert mine[0]["vgpr_count"] <= 128 and mine[0]["group_segment_fixed_size"] <= 32 * 1024, mine[0]  # four wavefronts per SIMD, four workgroups per CU
    assert not any("lbft_k_run" in k or "lbft_k_ct_" in k or "lbft_k_ps_" in k or "lbft_k_rs_" in k for k in cs), sorted(cs)
    for other in other_libs("chain_stats"):
        assert not any("lbft_k_cs_" in k for k in _kernel_metadata(other)), other
    # the register tool lists it
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    argv = sys.argv
    sys.argv = ["kernel_regs.py", build.CS_OUT]
    try:
        kernel_regs.main()
    finally:
        sys.argv = argv
    out = capsys.readouterr().out
    assert out.count("lbft_k_cs_chain") == 1 and "scratch    0 B" in out, out


def test_the_main_library_keeps_its_machine_code(hiplib):
    from librabft_simulator_amd import build
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.json")))
    assert build.kernel_hash(build.OUT) == committed["kernel_hash"]
    assert build.kernel_hash(build.CS_OUT) != committed["kernel_hash"]
