"""Host build of the commit-time classes against the oracle: batches run through lbft_core.h's K_SMALL_TIMED / K_MID_TIMED /
K_SMALL_SETS_TIMED / K_MID_SETS_TIMED steps on the CPU (tests/commit_times_host_model.cpp, compiled here with g++) record, entry for entry,
the commit times derived from fresh oracle runs (tests/commit_times_oracle.py), and their histories equal the oracle's.  Drawn: 3 to 32
nodes, both delay models, equivocators, loss and partitions, quirks 0 and 3 with a small commands_per_epoch (epoch changes), weighted
rights, and parameter-set batches with mixed sets."""
import ctypes as C
import os

import numpy as np
import pytest

import commit_times_oracle as cto
from support import build_shim, set_oracle_cfg

THREADS = min(os.cpu_count() or 8, 16)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return load_harness(tmp_path_factory.mktemp("ct_host"))


def load_harness(directory):
    """Compiles the host model into `directory` and binds it."""
    L = build_shim(directory, "commit_times_host_model.cpp", "libct_hostmodel.so", "-ffp-contract=off", "-pthread", "-w")
    vp = C.c_void_p
    L.ct_hostmodel_run.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_size_t, C.c_int64, C.c_uint32, vp, vp, vp, vp, C.c_size_t, vp, C.c_uint32]
    L.ct_hostmodel_run.restype = C.c_int
    return L


def run_host(L, base, sets, set_of, seeds, max_clock, cap, state_fill=0):
    from librabft_simulator_amd import _lib
    m, n = len(seeds), base.num_nodes
    arr = (_lib.LbftParamSet * max(len(sets), 1))(*sets)
    set_of = np.ascontiguousarray(set_of if sets else np.zeros(m), dtype=np.uint32)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    cc = np.zeros((m, n), dtype=np.uint32)
    ct = np.zeros((m, n, cap), dtype=np.int64)
    hist = np.zeros((m, n, cap), dtype=_lib.COMMIT_DTYPE)
    st = np.zeros((m, n), dtype=np.int64)
    faults = np.zeros(m, dtype=np.uint32)
    cls = L.ct_hostmodel_run(C.byref(base), arr, len(sets), set_of.ctypes.data, seeds.ctypes.data, m, max_clock, THREADS, cc.ctypes.data,
                             ct.ctypes.data, hist.ctypes.data, st.ctypes.data, cap, faults.ctypes.data, state_fill)
    assert cls >= 0, cls
    return cls, {"commit_counts": cc, "commit_times": ct, "histories": hist, "startup_times": st, "faults": faults}


def draw(rng, n, n_sets, small=False):
    """A base config for n nodes and n_sets sets (the base's own fields are set 0's for a plain batch); `small`: an honest, lossless
    network without the record exchange (kernel class 0 for <= 4 nodes)."""
    from librabft_simulator_amd import _lib
    base = _lib.LbftConfig()
    base.num_nodes = n
    base.delay_model = int(rng.random() < 0.35)
    base.quirks = 0 if small else int(rng.choice([0, 0, 3]))
    base.commands_per_epoch = int(rng.choice([30000, 3, 5]))
    base.equivocate_every = int(rng.choice([0, 0, 3])) if n >= 4 and not small else 0
    lossy = rng.random() < 0.5 and not small
    sets = []
    for _ in range(max(n_sets, 1)):
        s = _lib.LbftParamSet()
        s.mean = float(rng.choice([4.0, 8.0, 12.0]))
        s.variance = float(rng.choice([0.0, 2.0, 9.0]))
        s.uniform_lo = int(rng.integers(1, 6))
        s.uniform_hi = s.uniform_lo + int(rng.integers(0, 15))
        s.delta = int(rng.choice([10, 20, 40]))
        s.gamma = float(rng.choice([1.5, 2.0]))
        s.lambda_ = float(rng.choice([0.25, 0.5, 0.75]))
        s.target_commit_interval = int(rng.choice([100000, 100000, 60]))
        if lossy:
            s.drop_per_million = int(rng.choice([0, 10000, 40000]))
            if rng.random() < 0.5:
                s.partition_size = int(rng.integers(1, n))
                s.partition_start = int(rng.integers(0, 100))
                s.partition_end = s.partition_start + int(rng.integers(30, 150))
        sets.append(s)
    rights = None
    if rng.random() < 0.3:
        rights = rng.integers(1, 4, size=n).astype(np.uint64)
    if not n_sets:
        s = sets[0]
        for f in ("mean", "variance", "uniform_lo", "uniform_hi", "delta", "gamma", "lambda_", "target_commit_interval", "drop_per_million",
                  "partition_size", "partition_start", "partition_end"):
            setattr(base, f, getattr(s, f))
    if rights is not None:
        base._rights = np.ascontiguousarray(rights)  # (kept alive with the struct)
        base.voting_rights = base._rights.ctypes.data_as(C.POINTER(C.c_uint64))
    return base, (sets if n_sets else []), sets, rights


# (nodes, parameter sets -- 0 = a plain batch, class 0 forced)
CASES = [(3, 0, False), (4, 0, False), (4, 3, False), (5, 0, False), (7, 0, False), (10, 4, False), (16, 0, False), (20, 0, False), (32, 0, False),
         (4, 0, True), (6, 2, False), (13, 0, False), (4, 5, True), (24, 3, False), (8, 0, False), (3, 2, False), (3, 0, True), (4, 4, True)]


def test_commit_times_equal_the_oracle(harness, oracle):
    rng = np.random.default_rng(20261015)
    classes, flags, compared, epochs_changed, samples, big_commits = set(), set(), 0, False, 0, False
    for case, (n, n_sets, small) in enumerate(CASES):
        base, sets, all_sets, rights = draw(rng, n, n_sets, small)
        m = 8 if n <= 10 else 4
        set_of = (np.arange(m) % max(n_sets, 1)).astype(np.uint32)
        seeds = rng.integers(1, 1 << 40, size=m).astype(np.uint64)
        max_clock = 300 if n <= 10 else 240
        cap = max_clock // 2 + 64
        cls, got = run_host(harness, base, sets, set_of, seeds, max_clock, cap)
        classes.add((cls, bool(n_sets)))
        configs = [set_oracle_cfg(oracle, base, s, rights) for s in all_sets]
        ref_ct = cto.param_set_commit_times(oracle, configs, set_of, seeds, max_clock, cap, THREADS)
        ok = got["faults"] == 0  # (capacity faults are the host build's, not the protocol's: compared where none was raised)
        assert ok.sum() >= m // 2, (case, got["faults"])
        assert (got["commit_times"][ok] == ref_ct[ok]).all(), (case, n, n_sets)
        for k, cfg in enumerate(configs):
            idx = np.nonzero(set_of == k)[0]
            ref = oracle.run_batch(cfg, seeds[idx], max_clock, history_cap=cap)
            sel = ok[idx]
            assert (got["commit_counts"][idx][sel] == ref["commit_counts"][sel]).all(), (case, k)
            assert (got["histories"][idx][sel] == ref["histories"][sel]).all(), (case, k)
        assert ((got["commit_times"] >= 0).sum(axis=2)[ok] == got["commit_counts"][ok]).all()
        lat, _ = cto.latencies(got["commit_times"], got["histories"], got["startup_times"], got["faults"])
        assert (lat >= 0).all() and (lat <= max_clock).all(), case
        samples += len(lat)
        big_commits |= n > 16 and len(lat) > 0
        compared += int(ok.sum())
        flags.add((base.quirks, base.equivocate_every > 0, rights is not None, any(s.drop_per_million or s.partition_size for s in all_sets),
                   base.delay_model))
        epochs_changed |= base.commands_per_epoch < 100 and int(got["commit_counts"].max()) > base.commands_per_epoch
    assert classes >= {(0, False), (1, False), (0, True), (1, True)}, classes  # the four commit-time classes ran
    assert any(f[0] == 3 for f in flags) and any(f[1] for f in flags) and any(f[2] for f in flags) and any(f[3] for f in flags)
    assert {f[4] for f in flags} == {0, 1}
    assert epochs_changed
    assert compared >= 60 and samples >= 1000 and big_commits, (compared, samples)


def test_quantile_rule_is_numpy_inverted_cdf():
    from librabft_simulator_amd.simulator import histogram_quantile
    rng = np.random.default_rng(3)
    for trial in range(200):
        x = rng.integers(0, int(rng.integers(1, 60)), size=int(rng.integers(1, 300)))
        hist = np.bincount(x, minlength=int(x.max()) + 1 + int(rng.integers(0, 5)))
        for q in (0.0, 0.01, 0.25, 0.5, 0.9, 0.99, 1.0, float(rng.random())):
            assert histogram_quantile(hist, 1, q) == int(np.quantile(x, q, method="inverted_cdf")), (trial, q)
    assert histogram_quantile(np.zeros(4, dtype=np.uint64), 1, 0.5) is None
    assert histogram_quantile(np.array([0, 3, 1]), 5, 0.9) == 10  # (bin k starts at k * width)


@pytest.mark.parametrize("equivocate_every,n_sets", [(0, 0), (0, 2), (3, 0), (3, 2)], ids=["class0", "class0-sets", "class1", "class1-sets"])
def test_returned_class_is_the_one_from_before_the_table_of_run_kernels(harness, equivocate_every, n_sets):
    from test_host_dispatch import TWIN_CLASS, twin_batch
    assert run_host(harness, *twin_batch(equivocate_every, n_sets), 0, 4)[0] == TWIN_CLASS[equivocate_every, n_sets]
