"""CPU-side checks of the run load (lbft_batch_load_stats, lbft_batch_instance_load): the entry points are declared, exported and bound,
the launcher lives in liblbft_paramsets.so alone and is in build.TABLE's row, NULL arguments are refused first and before any HIP call
(whatever the other arguments are), the Python methods check their arguments before any library call, the kernel is in the
parameter-set library's code object exactly once and without scratch, the rule header's first part needs <stdint.h> alone, and
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
NAMES = ("lbft_batch_load_stats", "lbft_batch_instance_load")
KERNEL, LAUNCHER = "lbft_k_ps_load", "lbft_ps_launch_load"


def test_load_symbols_are_declared_exported_and_bound(hiplib):
    import load_stats_reference as ref
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    raw = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in hiplib.ABI_SYMBOLS and hasattr(raw, name), name
    assert len(hiplib.lib().lbft_batch_load_stats.argtypes) == 8 and len(hiplib.lib().lbft_batch_instance_load.argtypes) == 2
    for macro, value in (("LBFT_LOAD_FAMILIES", 16), ("LBFT_LOAD_STATS", 64), ("LBFT_LOAD_CAPS", 5)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert hiplib.LOAD_STATS == 64 == ref.LOAD_STATS == 4 * len(hiplib.LOAD_FAMILIES) and hiplib.LOAD_FAMILIES == ref.FAMILIES
    assert hiplib.LOAD_CAPS == ("queue", "chunks", "snapshots", "blocks", "log")
    assert [hiplib.LOAD_FAMILIES.index(name) for name in hiplib.LOAD_CAPS] == [9, 10, 11, 12, 13]


def test_launcher_is_in_the_table_and_exported_by_the_paramsets_library_alone(hiplib):
    from librabft_simulator_amd import build
    assert LAUNCHER in dict((lib.tag, lib.launchers) for lib in build.TABLE)["paramsets"]
    assert hasattr(ctypes.CDLL(build.PS_OUT), LAUNCHER)
    for other in other_libs("paramsets"):
        assert not hasattr(ctypes.CDLL(other), LAUNCHER), other
    assert "lbft_ps_load_fn" in open(os.path.join(CSRC, "lbft_paramsets.h")).read()
    # the rule header is the parameter-set library's alone, and its first part needs nothing of the device
    header = os.path.join(CSRC, "lbft_load_stats.h")
    assert header in build.PS_DEPS
    for deps in (build.DEPS, build.CT_DEPS, build.RS_DEPS, build.CS_DEPS, build.RH_DEPS):
        assert header not in deps
    text = open(header).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text)) == ["lbft_group_stats.h", "stdint.h"]
    assert "__shfl" not in text.split("#if defined(__HIPCC__)")[0] and "ld_reduce_to_lds" not in open(os.path.join(CSRC, "lbft_group_stats.h")).read()


def test_null_arguments_are_refused_first_and_without_a_gpu(hiplib):
    L = hiplib.lib()
    hist, faults, stats = np.zeros(16, np.uint64), np.zeros(32, np.uint64), np.zeros(64, np.uint64)
    caps, rows = np.full(5, 77, np.uint32), np.full(16, 77, np.uint32)
    p = [a.ctypes.data for a in (hist, faults, stats)]
    fake = ctypes.c_void_p(hist.ctypes.data)  # never dereferenced: a NULL argument is refused before the handle is looked at
    for family, width, bins in ((9, 1, 16), (16, 1, 16), (0, 0, 16), (0, 1, 0), (99, 0, 0)):
        assert L.lbft_batch_load_stats(None, family, width, bins, *p, caps.ctypes.data) == hiplib.LBFT_ERR_INVALID
        assert L.lbft_batch_load_stats(None, family, width, bins, *p, None) == hiplib.LBFT_ERR_INVALID
        for k in range(3):
            args = list(p)
            args[k] = None
            assert L.lbft_batch_load_stats(fake, family, width, bins, *args, caps.ctypes.data) == hiplib.LBFT_ERR_INVALID, k
    assert L.lbft_batch_instance_load(None, rows.ctypes.data) == hiplib.LBFT_ERR_INVALID
    assert L.lbft_batch_instance_load(fake, None) == hiplib.LBFT_ERR_INVALID and L.lbft_batch_instance_load(None, None) == hiplib.LBFT_ERR_INVALID
    assert not hist.any() and not faults.any() and not stats.any() and (caps == 77).all() and (rows == 77).all()


def test_refusals_are_ordered_in_the_source():
    """State before the family and the binning, all before the library is opened and the device is set (a batch that has run needs
    a device: tests/test_load_stats_gpu.py observes the order there)."""
    text = open(os.path.join(CSRC, "lbft_hip.hip")).read()
    body = text[text.index("static int refuse_load("):text.index("int lbft_batch_load_stats(")]
    order = [body.index(s) for s in ("refuse_grouped(b, args_ok, 1, 1, false)", "hist_family >= LBFT_LOAD_FAMILIES", "refuse_grouped(b, true, bin_width, bins, false)",
                                     "load_paramsets_lib()")]
    assert order == sorted(order) and "hip" not in body.replace("lbft_hip", "")
    for name in NAMES:
        fn = text[text.index("int %s(" % name):]
        fn = fn[:fn.index("\n}\n")]
        assert fn.index("refuse_load(") < fn.index("hipSetDevice") < fn.index("GroupedCall gc(b)") < fn.index("g_ps_load("), name


def test_python_methods_refuse_bad_arguments_before_the_device():
    from librabft_simulator_amd.simulator import BatchResult
    res = BatchResult(Stub())
    for kw in ({"bins": 0}, {"bin_width": 0}, {"bins": -3}, {"bin_width": -1}, {"family": "latency"}, {"family": 16}, {"family": -1}, {"family": None},
               {"family": 1.5}, {"family": True}):
        with pytest.raises(ValueError):
            res.load_stats(**kw)


def test_grid_load_option_is_parsed():
    from librabft_simulator_amd import grid
    with pytest.raises(SystemExit):  # a bad option ends the tool before it creates a batch
        grid.main(["--load", "--seeds-per-point", "0"])
    with pytest.raises(SystemExit):
        grid.main(["--load=yes"])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_load_kernel_is_in_the_paramsets_library_alone_and_uses_no_scratch(hiplib):
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    ps = _kernel_metadata(build.PS_OUT)
    mine = [v for k, v in ps.items() if re.search(r"\d+%sN" % KERNEL, k)]
    assert len(mine) == 1, sorted(ps)
    print(mine[0])
    assert mine[0]["private_segment_fixed_size"] == 0 and mine[0]["vgpr_spill_count"] == 0, mine[0]
    # (the 32 KiB histogram lets four workgroups share a CU's LDS: four wavefronts per SIMD, which 128 registers allow)
    assert mine[0]["vgpr_count"] <= 128 and mine[0]["group_segment_fixed_size"] <= 40 * 1024, mine[0]
    assert not any("_run" in k for k in ps if KERNEL in k)
    for other in other_libs("paramsets"):
        assert not any(KERNEL in k for k in _kernel_metadata(other)), other


def test_the_main_library_keeps_its_machine_code(hiplib):
    from librabft_simulator_amd import build
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.json")))
    assert build.kernel_hash(build.OUT) == committed["kernel_hash"]
