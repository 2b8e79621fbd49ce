"""The step tail on the device: a finished run reduces its fourteen batch counters with lbft_k_ps_counters (liblbft_paramsets.so) and
computes the State hashes only when they are asked for (lbft_k_finalize, once per finished run).

Every case compares the counters, commit counts, active rounds and State hashes with the oracle, and derives `rounds`, `commits` and
`faulted_instances` from the per-node / per-instance arrays of the same run.  The counters are read BEFORE the hashes: they are the lean
kernel's.  The request for the hashes then launches lbft_k_finalize, whose own fourteen words are compared with them inside the library
(a difference is an error that names the counter), so every hash read below is also that cross-check.

The lifecycle cases pin which state the hashes belong to: the last finished run's, whatever was accepted in between."""
import os
import subprocess
import sys

import numpy as np
import pytest

from support import amd, oracle_cfg, run_to_end  # noqa: F401
from test_gpu_parity import HOST_THREADS, run_gpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_COUNTERS = ("events", "rng_draws", "rounds", "commits", "events_scheduled")

# name -> (oracle / device configuration, instances, max_clock, run kernel or kernel class the batch must take, or None)
BATCHES = {
    "headline_1056x4_run0q": (dict(num_nodes=4), 1056, 200, "lbft_k_run0q"),         # 16.5 wavefronts of 64 instances: a partial last one
    "headline_130x4_run0u": (dict(num_nodes=4), 130, 1000, "lbft_k_run0u"),           # one full and one partial 64-block
    "golden_5x3": (dict(num_nodes=3), 5, 1000, None),
    "weighted_70x7": (dict(num_nodes=7, voting_rights=[2, 1, 1, 3, 1, 2, 1]), 70, 1000, None),  # node count no multiple of 4
    "equivocator_65x8": (dict(num_nodes=8, equivocate_every=8), 65, 1000, 1),         # class 1; crosses a 64-instance tile
    "large_3x40": (dict(num_nodes=40), 3, 100, 2),                                    # large network, large class
}


def seeds_of(m):
    return np.arange(1, m + 1, dtype=np.uint64) * 104729 + 17


def kernel_name(sim):
    sys.path.insert(0, ROOT)
    import bench
    return bench.run_kernel_name(sim.layout()["kernel_class"])


def check_counters(res, ref_counters):
    """The lean kernel's counters: equal to the oracle's (where one oracle run gives them) and to what the run's own arrays say."""
    c = res.counters
    print("counters", c)
    if ref_counters is not None:
        for key in ORACLE_COUNTERS:
            assert c[key] == ref_counters[key], (key, c[key], ref_counters[key])
    assert c["rounds"] == int(res.active_rounds.min(axis=1).sum())
    assert c["commits"] == int(res.commit_counts.min(axis=1).sum())
    assert c["faulted_instances"] == int(np.count_nonzero(res.faults))
    return c


def check_against(res, ref, rows=slice(None)):
    """Counters first (no State hash has been asked for yet), then the arrays, the hashes last."""
    first = dict(check_counters(res, ref.get("counters")))
    assert (res.commit_counts[rows] == ref["commit_counts"][rows]).all()
    assert (res.active_rounds[rows] == ref["active_rounds"][rows]).all()
    assert (res.last_committed_states[rows] == ref["last_states"][rows]).all()  # (launches lbft_k_finalize: the cross-check of all fourteen words)
    assert type(res)(res._sim).counters == first  # read again from the library: the hash request changed no counter


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_batch_counters_and_hashes_equal_the_oracle(amd, oracle, name):
    kw, m, max_clock, kernel = BATCHES[name]
    seeds = seeds_of(m)
    sim, res = run_gpu(amd, kw, seeds, max_clock)
    if isinstance(kernel, str):
        assert kernel_name(sim) == kernel, sim.layout()
    elif kernel is not None:
        assert sim.layout()["kernel_class"] & 255 == kernel, sim.layout()
    ref = oracle.run_batch(oracle.make_config(math_mode=1, **kw), seeds, max_clock, threads=HOST_THREADS, history_cap=8)
    assert not res.faults.any()
    check_against(res, ref)
    sim.close()


def two_sets(amd):
    return [amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, 20, 2.0, 0.5)),
            amd.ParamSet(amd.RandomDelay.new(5.0, 2.5), amd.NodeConfig(40, 40, 1.75, 0.25))]


@pytest.mark.parametrize("timed", [False, True], ids=["param_sets_66", "param_sets_66_commit_times"])
def test_parameter_set_batch_counters_and_hashes_equal_the_oracle(amd, oracle, timed):
    sets, m, max_clock = two_sets(amd), 66, 1000
    set_of = (np.arange(m) % 2).astype(np.uint32)
    seeds = seeds_of(m)
    sim = amd.BatchSimulator.with_param_sets(seeds, 4, sets, set_of, **(dict(commit_times=True) if timed else {}))
    res = sim.loop_until(max_clock)
    assert sim.layout()["kernel_class"] & 65536 and bool(sim.layout()["kernel_class"] & 131072) == timed, sim.layout()
    ref = {"commit_counts": np.zeros((m, 4), np.uint32), "active_rounds": np.zeros((m, 4), np.uint64), "last_states": np.zeros((m, 4), np.uint64),
           "counters": {"events": [0, 0, 0, 0], "rng_draws": 0, "rounds": 0, "commits": 0, "events_scheduled": 0}}
    for k, ps in enumerate(sets):
        idx = np.nonzero(set_of == k)[0]
        part = oracle.run_batch(oracle_cfg(oracle, 4, ps), seeds[idx], max_clock, threads=HOST_THREADS, history_cap=8)
        for key in ("commit_counts", "active_rounds", "last_states"):
            ref[key][idx] = part[key]
        for key in ORACLE_COUNTERS:  # the batch's counters are the sums over its sets' runs
            if key == "events":
                ref["counters"][key] = [a + b for a, b in zip(ref["counters"][key], part["counters"][key])]
            else:
                ref["counters"][key] += part["counters"][key]
    assert not res.faults.any()
    check_against(res, ref)
    sim.close()


# ---- lifecycle: the 130 x 4 batch, one oracle run for all cases ----
KW, M, MAX_CLOCK = BATCHES["headline_130x4_run0u"][:3]


@pytest.fixture(scope="module")
def ref130(oracle):
    return oracle.run_batch(oracle.make_config(math_mode=1, **KW), seeds_of(M), MAX_CLOCK, threads=HOST_THREADS, history_cap=8)


def new130(amd, **kw):
    return amd.BatchSimulator.new(seeds_of(M), 4, amd.RandomDelay.new(10.0, 4.0), **kw)


def raw_states(sim):
    from librabft_simulator_amd import _lib
    out = np.zeros((sim.num_instances, sim.num_nodes), dtype=np.uint64)
    _lib.check(_lib.lib().lbft_batch_last_committed_states(sim._h, out.ctypes.data))
    return out


def test_hashes_after_reset_and_a_second_run_are_the_second_runs(amd, ref130):
    sim = new130(amd)
    first = sim.loop_until(300)  # its hashes are never asked for
    assert first.counters["commits"] < ref130["counters"]["commits"]
    sim.reset()
    check_against(sim.loop_until(MAX_CLOCK), ref130)
    sim.close()


def test_hashes_asked_for_twice_are_identical_and_leave_the_counters(amd, ref130):
    import ctypes
    from librabft_simulator_amd import _lib
    sim = new130(amd)
    res = sim.loop_until(MAX_CLOCK)
    before = dict(res.counters)
    assert any("liblbft_paramsets.so" in line for line in open("/proc/self/maps"))  # a plain batch, and the counters kernel's library is open
    a, b = raw_states(sim), raw_states(sim)
    assert (a == b).all() and (a == ref130["last_states"]).all()
    one = ctypes.c_uint64()
    _lib.check(_lib.lib().lbft_batch_last_committed_state(sim._h, M - 1, 3, ctypes.byref(one)))
    assert one.value == int(a[M - 1, 3])
    assert amd.BatchResult(sim).counters == before
    # the single-node call as the FIRST request of a run
    sim.reset()
    sim.loop_until(MAX_CLOCK)
    _lib.check(_lib.lib().lbft_batch_last_committed_state(sim._h, 64, 1, ctypes.byref(one)))
    assert one.value == int(ref130["last_states"][64, 1])
    sim.close()


def test_hashes_after_a_stepped_run_that_finishes(amd, ref130):
    sim = new130(amd)
    res = run_to_end(sim, MAX_CLOCK, 97)
    assert res.counters["launches"] > 3
    check_against(res, ref130)
    sim.close()


def test_hashes_after_checkpoint_load_and_resume(amd, ref130, tmp_path):
    path = str(tmp_path / "mid.ckp")
    sim = new130(amd)
    for _ in range(3):
        left, _res = sim.run_steps(MAX_CLOCK, 97)
        assert left > 0
    sim.save_checkpoint(path)
    sim.close()
    resumed = new130(amd)
    resumed.loop_until(300)  # a finished run whose hashes stay pending ...
    resumed.reset()           # ... and are dropped here: the checkpoint's run is another state
    resumed.load_checkpoint(path)
    check_against(run_to_end(resumed, MAX_CLOCK, 97), ref130)
    resumed.close()


def test_a_faulted_instance_is_counted_raises_and_leaves_its_neighbours_hashes(amd, ref130):
    """queue_capacity one below the batch's own high-water mark: the instances that reach it (at least one, far from all) raise
    LBFT_FAULT_QUEUE_OVERFLOW; the run still raises LBFT_ERR_FAULT, the counter is the number of non-zero fault words, and every other
    instance's results and hashes are the oracle's."""
    probe = new130(amd)
    high = probe.loop_until(MAX_CLOCK).counters["max_queue"]
    probe.close()
    sim = new130(amd, queue_capacity=high - 1)
    with pytest.raises(amd.LbftError) as e:
        sim.loop_until(MAX_CLOCK)
    assert e.value.code == -5
    sim.reset()
    res = sim.loop_until(MAX_CLOCK, allow_faults=True)
    faulted = res.faults != 0
    print("max_queue %d, faulted instances %s" % (high, np.nonzero(faulted)[0].tolist()))
    assert 1 <= faulted.sum() < M // 2 and (res.faults[faulted] & 1).all()
    c = check_counters(res, None)
    assert c["faulted_instances"] == int(faulted.sum())
    clean = ~faulted
    assert (res.commit_counts[clean] == ref130["commit_counts"][clean]).all() and (res.active_rounds[clean] == ref130["active_rounds"][clean]).all()
    assert (res.last_committed_states[clean] == ref130["last_states"][clean]).all()
    sim.close()


def test_node_calls_after_manual_finalize_leave_the_hashes_of_the_finalize(amd, oracle):
    """lbft_batch_manual_finalize, more node-level calls, then the hashes.  The expectation is read from the parent's code: d_states_out is
    written by lbft_k_finalize inside lbft_batch_manual_finalize and by nothing else, and the node-level calls stay accepted after it --
    so the hashes read after further calls are those of the state AT the finalize, although the nodes have committed more since.  Session
    A reads them right after its finalize; session B makes the same calls, finalizes, goes on, and only then asks."""
    from test_node_level import DeviceDriver, full_exchange

    def rounds(d, clocks):
        for clock in clocks:
            full_exchange(d, clock, [])

    a = DeviceDriver(amd, 4)
    rounds(a, range(0, 12))
    res_a = a.sim.manual_finalize()
    at_finalize, commits_a = raw_states(a.sim), res_a.commit_counts.copy()
    assert commits_a[1].min() > 0 and commits_a[0].sum() == 0

    b = DeviceDriver(amd, 4)
    rounds(b, range(0, 12))
    res_b = b.sim.manual_finalize()
    check_counters(res_b, None)
    rounds(b, range(12, 24))  # accepted after the finalize; the first of these calls computes the pending hashes
    assert (raw_states(b.sim) == at_finalize).all()
    later = b.sim.manual_finalize()
    assert (later.commit_counts[1] > commits_a[1]).all()  # the state did move on ...
    check_counters(later, None)
    moved = raw_states(b.sim)
    assert (moved[1] != at_finalize[1]).all() and (moved[0] == at_finalize[0]).all()  # ... and the second finalize's hashes follow it
    a.sim.close()
    b.sim.close()


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import librabft_simulator_amd as amd
from librabft_simulator_amd import _lib
assert os.path.dirname(_lib.LIB_PATH) == %(lib_dir)r, _lib.LIB_PATH
seeds = np.arange(1, %(m)d + 1, dtype=np.uint64) * 104729 + 17
sim = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0))
res = sim.loop_until(%(max_clock)d)
c = res.counters
mapped = sorted(set(l.split()[-1] for l in open("/proc/self/maps") if "liblbft_" in l))
assert [os.path.basename(p) for p in mapped] == ["liblbft_hip.so"], mapped
np.savez(%(out)r, commit_counts=res.commit_counts, active_rounds=res.active_rounds, last_states=res.last_committed_states, faults=res.faults,
         counters=np.array(c["events"] + [c["rng_draws"], c["rounds"], c["commits"], c["events_scheduled"], c["faulted_instances"]], dtype=np.uint64))
"""


def test_a_plain_batch_without_the_side_library_falls_back_and_equals_the_oracle(ref130, tmp_path):
    """liblbft_hip.so alone in a directory (LBFT_HIP_LIB), in a fresh process: no liblbft_paramsets.so beside it, so every run takes
    lbft_k_finalize as it always did -- silently, with the same results."""
    import shutil
    from librabft_simulator_amd import build
    lib_dir = str(tmp_path / "alone")
    os.mkdir(lib_dir)
    shutil.copy(build.OUT, lib_dir)
    out = str(tmp_path / "child.npz")
    code = CHILD % dict(root=ROOT, lib_dir=lib_dir, m=M, max_clock=MAX_CLOCK, out=out)
    run = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LBFT_HIP_LIB=os.path.join(lib_dir, "liblbft_hip.so")),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.load(out)
    assert not got["faults"].any()
    for key in ("commit_counts", "active_rounds", "last_states"):
        assert (got[key] == ref130[key]).all(), key
    rc = ref130["counters"]
    assert got["counters"].tolist() == list(rc["events"]) + [rc["rng_draws"], rc["rounds"], rc["commits"], rc["events_scheduled"], 0]
