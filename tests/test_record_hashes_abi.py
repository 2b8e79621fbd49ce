"""CPU-side checks of the record hashes of whole batches (lbft_batch_chain_record_hashes): the entry point is declared, exported and bound,
the launcher lives in liblbft_record_hashes.so alone, NULL and zero arguments are refused before any HIP call, the Python methods check
their arguments before any library call, the new kernel is in the side library's code object exactly once and without scratch, and
liblbft_hip.so's machine code is still the committed manifest's."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

from support import Stub, hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lbft_batch_chain_record_hashes"


def test_symbol_is_declared_exported_and_bound(hiplib):
    from librabft_simulator_amd import build
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    assert NAME in declared and NAME in hiplib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(hiplib.LIB_PATH), NAME)
    assert len(getattr(hiplib.lib(), NAME).argtypes) == 5
    # the structs: 32 and 40 bytes, field for field
    assert hiplib.RECORD_HASH_DTYPE.itemsize == 32 and hiplib.CHAIN_HEAD_DTYPE.itemsize == 40
    head = re.search(r"typedef struct lbft_chain_head \{(.*?)\} lbft_chain_head;", header, re.S).group(1)
    fields = [f.strip() for part in re.findall(r"uint(?:64|32)_t ([^;]+);", head) for f in part.split(",")]
    assert fields == list(hiplib.CHAIN_HEAD_DTYPE.names)
    assert (build.RH_SRC, build.RH_OUT, build.RH_DEPS) in build.LIBS and os.path.basename(build.RH_OUT) == "liblbft_record_hashes.so"
    assert hasattr(ctypes.CDLL(build.RH_OUT), "lbft_rh_launch_chain")
    for other in (hiplib.LIB_PATH, *other_libs("record_hashes")):
        assert not hasattr(ctypes.CDLL(other), "lbft_rh_launch_chain"), other
    csrc = os.path.join(ROOT, "librabft_simulator_amd", "csrc")
    iface = open(os.path.join(csrc, "lbft_record_hashes.h")).read()
    assert "lbft_rh_chain_fn" in iface and re.search(r"#define LBFT_RH_TEMP_BYTES \(256ull << 20\)", iface)
    assert os.path.join(csrc, "lbft_record_hashes.h") in build.DEPS and os.path.join(csrc, "lbft_record_hash_rules.h") in build.RH_DEPS
    # the rules need nothing of the device beyond what lbft_core.h offers
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", open(os.path.join(csrc, "lbft_record_hash_rules.h")).read())
    assert sorted(includes) == ["lbft_core.h", "stdint.h"]
    assert "fn " + NAME in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()


def test_arguments_are_refused_without_a_gpu(hiplib):
    L = hiplib.lib()
    out = np.full(4, 7, dtype=hiplib.RECORD_HASH_DTYPE)
    heads = np.full(1, 7, dtype=hiplib.CHAIN_HEAD_DTYPE)
    prefix = np.full(4, 7, dtype=np.uint32)
    o, h, p = out.ctypes.data, heads.ctypes.data, prefix.ctypes.data
    for args in ((o, 4, h, p), (None, 0, h, None), (o, 0, h, p), (o, 4, None, p), (None, 0, None, None)):
        assert L.lbft_batch_chain_record_hashes(None, *args) == hiplib.LBFT_ERR_INVALID
    assert out.tobytes() == np.full(4, 7, dtype=hiplib.RECORD_HASH_DTYPE).tobytes() and (prefix == 7).all()
    assert heads.tobytes() == np.full(1, 7, dtype=hiplib.CHAIN_HEAD_DTYPE).tobytes()


def test_python_methods_refuse_bad_arguments_before_the_device():
    from librabft_simulator_amd.simulator import BatchResult
    res = BatchResult(Stub())
    for cap in (0, -1):
        with pytest.raises(ValueError):
            res.chain_record_hashes(cap)
    assert callable(res.chain_heads)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_kernel_is_in_its_own_library_without_scratch(hiplib, capsys):
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    assert os.path.exists(build.RH_OUT)
    rh = _kernel_metadata(build.RH_OUT)
    mine = [v for k, v in rh.items() if re.search(r"\d+lbft_k_rh_chainN", k)]
    assert len(mine) == 1 and len([k for k in rh if "lbft_k_" in k]) == 1, sorted(rh)
    assert mine[0]["private_segment_fixed_size"] == 0 and mine[0]["vgpr_spill_count"] == 0, mine[0]
    assert mine[0]["vgpr_count"] <= 128 and mine[0]["group_segment_fixed_size"] == 0, mine[0]  # four wavefronts per SIMD, no LDS
    for other in other_libs("record_hashes"):
        assert not any("lbft_k_rh_" in k for k in _kernel_metadata(other)), other
    # the register tool lists it
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    argv = sys.argv
    sys.argv = ["kernel_regs.py", build.RH_OUT]
    try:
        kernel_regs.main()
    finally:
        sys.argv = argv
    out = capsys.readouterr().out
    assert out.count("lbft_k_rh_chain") == 1 and "scratch    0 B" in out, out


def test_the_main_library_keeps_its_machine_code(hiplib):
    from librabft_simulator_amd import build
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.json")))
    assert build.kernel_hash(build.OUT) == committed["kernel_hash"]
    assert build.kernel_hash(build.RH_OUT) != committed["kernel_hash"]
