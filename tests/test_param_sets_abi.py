"""CPU-side checks of parameter-set batches (lbft_batch_create_param_sets): the entry point is declared and exported, every argument is
validated before any HIP call, the kernels are built into a code object of their own (liblbft_paramsets.so) without scratch, and the
machine code of liblbft_hip.so is still the one the committed codegen manifest pins."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from support import hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_param_set_symbols_are_declared_and_exported(hiplib):
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    assert "lbft_batch_create_param_sets" in re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header)
    assert "typedef struct lbft_param_set" in header and re.search(r"#define LBFT_MAX_PARAM_SETS 256\b", header)
    assert "lbft_batch_create_param_sets" in hiplib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(hiplib.LIB_PATH), "lbft_batch_create_param_sets")
    # lbft_param_set: 2 f64, 4 i64, 2 f64, 2 u32, 2 i64
    assert ctypes.sizeof(hiplib.LbftParamSet) == 16 + 32 + 16 + 8 + 16


def _base(hiplib, n=4):
    cfg = hiplib.LbftConfig()
    cfg.num_nodes = n
    cfg.mean, cfg.variance, cfg.commands_per_epoch = 10.0, 4.0, 30000
    cfg.target_commit_interval, cfg.delta, cfg.gamma, cfg.lambda_ = 100000, 20, 2.0, 0.5
    return cfg


def _set(hiplib, **kw):
    s = hiplib.LbftParamSet()
    s.mean, s.variance, s.target_commit_interval, s.delta, s.gamma, s.lambda_ = 10.0, 4.0, 100000, 20, 2.0, 0.5
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _create(hiplib, cfg, sets, set_of, n_sets=None):
    L = hiplib.lib()
    arr = (hiplib.LbftParamSet * max(len(sets), 1))(*sets)
    idx = np.ascontiguousarray(set_of, dtype=np.uint32)
    seeds = np.arange(1, len(idx) + 1, dtype=np.uint64)
    h = ctypes.c_void_p()
    return L.lbft_batch_create_param_sets(ctypes.byref(cfg), arr, len(sets) if n_sets is None else n_sets, idx.ctypes.data, seeds.ctypes.data,
                                          len(idx), 0, ctypes.byref(h))


def test_argument_validation_needs_no_gpu(hiplib):
    ok = _set(hiplib)
    assert _create(hiplib, _base(hiplib), [], [0, 0], n_sets=0) == hiplib.LBFT_ERR_INVALID
    assert _create(hiplib, _base(hiplib), [ok] * 257, [0, 0]) == hiplib.LBFT_ERR_INVALID
    assert _create(hiplib, _base(hiplib), [ok, ok], [0, 2, 1]) == hiplib.LBFT_ERR_INVALID  # index out of range
    assert _create(hiplib, _base(hiplib), [ok, _set(hiplib, variance=-1.0)], [0, 1]) == hiplib.LBFT_ERR_INVALID
    assert _create(hiplib, _base(hiplib), [_set(hiplib, gamma=float("nan")), ok], [0, 1]) == hiplib.LBFT_ERR_INVALID
    assert _create(hiplib, _base(hiplib), [ok, _set(hiplib, delta=-5)], [0, 1]) == hiplib.LBFT_ERR_INVALID
    assert _create(hiplib, _base(hiplib, 33), [ok], [0, 0]) == hiplib.LBFT_ERR_UNSUPPORTED  # the large-network kernels are out of scope
    bad_quirks = _base(hiplib)
    bad_quirks.quirks = 4
    assert _create(hiplib, bad_quirks, [ok], [0]) == hiplib.LBFT_ERR_UNSUPPORTED


def test_python_api_validates_before_the_device():
    from librabft_simulator_amd import BatchSimulator, LbftError, NodeConfig, ParamSet, RandomDelay
    seeds = np.arange(1, 5, dtype=np.uint64)
    with pytest.raises(ValueError):
        BatchSimulator.with_param_sets(seeds, 4, [ParamSet(RandomDelay.new(10, 4)), ParamSet(RandomDelay.uniform(5, 15))], [0, 1, 0, 1])
    with pytest.raises(ValueError):
        BatchSimulator.with_param_sets(seeds, 4, [ParamSet()], [0, 0, 0])
    with pytest.raises(TypeError):
        BatchSimulator.with_param_sets(seeds, 4, [ParamSet()], [0, 0, 0, 0], drop_per_million=5)
    with pytest.raises(LbftError) as e:
        BatchSimulator.with_param_sets(seeds, 4, [ParamSet(node_config=NodeConfig(gamma=-1.0))], [0, 0, 0, 0])
    assert e.value.code == -1


def test_grid_assignments():
    from librabft_simulator_amd import grid
    set_of, seed_index = grid.set_assignment(3, 4, "blocked")
    assert list(set_of) == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2] and list(seed_index) == [0, 1, 2, 3] * 3
    set_of, seed_index = grid.set_assignment(3, 4, "interleaved")
    assert list(set_of) == [0, 1, 2] * 4 and list(seed_index) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]


def test_grid_cli_does_not_import_the_oracle():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import librabft_simulator_amd.grid\n"
            "print(sorted(m for m in sys.modules if 'oracle' in m))\n") % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip() == "[]"


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_param_set_kernels_are_a_separate_code_object_without_scratch(hiplib):
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    assert os.path.exists(build.PS_OUT)
    ps = _kernel_metadata(build.PS_OUT)
    names = sorted(ps)
    assert any("lbft_k_ps_init" in k for k in names) and any("lbft_k_ps_run0" in k for k in names) and any("lbft_k_ps_run1" in k for k in names), names
    base = _kernel_metadata(build.OUT)
    run0 = [v for k, v in base.items() if re.search(r"lbft_k_run0N", k)]
    run1 = [v for k, v in base.items() if "lbft_k_runILi1E" in k]
    assert len(run0) == 1 and len(run1) == 1, sorted(base)
    for k, v in ps.items():
        cap = run0[0] if "ps_run0" in k else run1[0] if "ps_run1" in k else {"private_segment_fixed_size": 0}
        assert v["private_segment_fixed_size"] <= cap["private_segment_fixed_size"], (k, v, cap)
    # none of them went into liblbft_hip.so or into another side library
    for other in other_libs("paramsets"):
        assert not any("lbft_k_ps_" in k for k in _kernel_metadata(other)), other


def test_main_library_machine_code_is_unchanged(hiplib):
    from librabft_simulator_amd import build
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_manifest.json")))
    assert build.kernel_hash(build.OUT) == committed["kernel_hash"]
    assert build.kernel_hash(build.PS_OUT) != committed["kernel_hash"]
