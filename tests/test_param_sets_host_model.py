"""Host build of the parameter-set classes against the oracle: mixed-set batches run through lbft_core.h on the CPU
(tests/param_sets_host_model.cpp, compiled here with g++), each instance equal to the oracle run of its own set's configuration and seed --
commit counts, active rounds, last states, histories.  Drawn: network sizes, both delay models, delta / gamma / lambda /
target_commit_interval, loss and partitions (the mid class), equivocators, blocked and interleaved assignment."""
import ctypes as C

import numpy as np
import pytest

from support import build_shim, set_oracle_cfg

SIZES = (3, 4, 7, 16, 20, 32)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return load_harness(tmp_path_factory.mktemp("ps_host"))


def load_harness(directory):
    """Compiles the host model into `directory` and binds it."""
    L = build_shim(directory, "param_sets_host_model.cpp", "libps_hostmodel.so", "-ffp-contract=off", "-pthread", "-w")
    vp = C.c_void_p
    L.ps_hostmodel_run.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_size_t, C.c_int64, C.c_uint32, vp, vp, vp, vp, C.c_size_t, vp, C.c_uint32]
    L.ps_hostmodel_run.restype = C.c_int
    return L


def run_host(L, base, sets, set_of, seeds, max_clock, history_cap, state_fill=0):
    from librabft_simulator_amd import _lib
    m, n = len(seeds), base.num_nodes
    arr = (_lib.LbftParamSet * len(sets))(*sets)
    set_of = np.ascontiguousarray(set_of, dtype=np.uint32)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    cc = np.zeros((m, n), dtype=np.uint32)
    ar = np.zeros((m, n), dtype=np.uint64)
    ls = np.zeros((m, n), dtype=np.uint64)
    hist = np.zeros((m, n, history_cap), dtype=_lib.COMMIT_DTYPE)
    faults = np.zeros(m, dtype=np.uint32)
    cls = L.ps_hostmodel_run(C.byref(base), arr, len(sets), set_of.ctypes.data, seeds.ctypes.data, m, max_clock, 8, cc.ctypes.data,
                             ar.ctypes.data, ls.ctypes.data, hist.ctypes.data, history_cap, faults.ctypes.data, state_fill)
    assert cls >= 0, cls
    return cls, {"commit_counts": cc, "active_rounds": ar, "last_states": ls, "histories": hist, "faults": faults}


def draw_batch(rng, n):
    """A base config and 3-8 sets for a network of n nodes."""
    from librabft_simulator_amd import _lib
    base = _lib.LbftConfig()
    base.num_nodes = n
    base.delay_model = int(rng.random() < 0.35)
    base.commands_per_epoch = 30000
    lossy = rng.random() < 0.5
    base.equivocate_every = int(rng.choice([0, 0, 0, 3])) if n >= 4 else 0
    base.quirks = int(rng.choice([0, 2]))
    sets = []
    for _ in range(int(rng.integers(3, 9))):
        s = _lib.LbftParamSet()
        s.mean = float(rng.choice([3.0, 5.0, 10.0, 20.0]))
        s.variance = float(rng.choice([0.0, 1.0, 4.0, 25.0]))
        s.uniform_lo = int(rng.integers(1, 8))
        s.uniform_hi = s.uniform_lo + int(rng.integers(0, 20))
        s.delta = int(rng.choice([5, 10, 20, 40]))
        s.gamma = float(rng.choice([1.0, 1.5, 2.0]))
        s.lambda_ = float(rng.choice([0.25, 0.5, 0.75, 1.0]))
        s.target_commit_interval = int(rng.choice([100000, 100000, 50, 200]))
        if lossy and rng.random() < 0.7:
            s.drop_per_million = int(rng.choice([0, 10000, 50000]))
            if rng.random() < 0.5:
                s.partition_size = int(rng.integers(1, n))
                s.partition_start = int(rng.integers(0, 200))
                s.partition_end = s.partition_start + int(rng.integers(50, 300))
        sets.append(s)
    return base, sets


def test_mixed_set_batches_equal_the_oracle_per_instance(harness, oracle):
    rng = np.random.default_rng(20261015)
    configs = compared = 0
    classes = set()
    batch = 0
    while configs < 300:
        n = SIZES[batch % len(SIZES)]
        how = "blocked" if batch % 2 == 0 else "interleaved"
        batch += 1
        base, sets = draw_batch(rng, n)
        per = 2
        k = np.arange(len(sets) * per)
        set_of = (k // per if how == "blocked" else k % len(sets)).astype(np.uint32)
        seeds = rng.integers(1, 1 << 40, size=len(set_of)).astype(np.uint64)
        max_clock = 400 if n <= 16 else 250
        cls, got = run_host(harness, base, sets, set_of, seeds, max_clock, 32)
        classes.add(cls)
        for j, s in enumerate(sets):
            idx = np.nonzero(set_of == j)[0]
            ref = oracle.run_batch(set_oracle_cfg(oracle, base, s), seeds[idx], max_clock, history_cap=32)
            ok = got["faults"][idx] == 0  # (capacity faults are the device's, not the protocol's: compared where none was raised)
            for key in ("commit_counts", "active_rounds", "last_states", "histories"):
                assert (got[key][idx][ok] == ref[key][ok]).all(), (batch, n, how, j, key)
            compared += int(ok.sum())
            configs += 1
    assert classes == {0, 1}, classes  # both the small and the mid class ran
    assert compared >= 500, compared


@pytest.mark.parametrize("equivocate_every", [0, 3], ids=["class0", "class1"])
def test_returned_class_is_the_one_from_before_the_table_of_run_kernels(harness, equivocate_every):
    from test_host_dispatch import TWIN_CLASS, twin_batch
    assert run_host(harness, *twin_batch(equivocate_every, 2), 0, 4)[0] == TWIN_CLASS[equivocate_every, 2]
