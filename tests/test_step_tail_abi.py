"""CPU-side checks of the step tail (State hashes on demand): the counters kernel behind every finished run, lbft_k_ps_counters, is built
into liblbft_paramsets.so alone, its launcher is exported there alone, it uses no scratch, and the machine code of liblbft_hip.so --
lbft_k_finalize included, which now runs only when the hashes are asked for -- is still the one the committed codegen manifest pins."""
import ctypes
import json
import os

import pytest

from support import hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL, LAUNCHER = "lbft_k_ps_counters", "lbft_ps_launch_counters"


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_counters_kernel_is_in_the_paramsets_library_alone_and_uses_no_scratch(hiplib):
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    mine = {k: v for k, v in _kernel_metadata(build.PS_OUT).items() if KERNEL in k}
    assert len(mine) == 1, sorted(_kernel_metadata(build.PS_OUT))
    meta = next(iter(mine.values()))
    print(meta)
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
    for other in other_libs("paramsets"):
        assert not any(KERNEL in k for k in _kernel_metadata(other)), other


def test_counters_launcher_is_exported_by_the_paramsets_library_alone(hiplib):
    from librabft_simulator_amd import build
    assert LAUNCHER in dict((lib.tag, lib.launchers) for lib in build.TABLE)["paramsets"]
    assert hasattr(ctypes.CDLL(build.PS_OUT), LAUNCHER)
    for other in other_libs("paramsets"):
        assert not hasattr(ctypes.CDLL(other), LAUNCHER), other


def test_main_library_machine_code_is_unchanged(hiplib):
    from librabft_simulator_amd import build
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.json")))
    assert build.kernel_hash(build.OUT) == committed["kernel_hash"]
