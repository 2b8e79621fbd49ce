"""The calendar queue's exhausted chunk pool on the device: the two mixed batches of tests/queue_exhaustion.py -- 8 seeds of which the host model
faults some for want of chunks (tests/test_queue_exhaustion_host.py holds the host model to the fence and the oracle on them) -- through
BatchSimulator at the same capacities.  The faulted instances are the host model's, with F_QUEUE_OVERFLOW; every other instance equals the oracle;
the handle survives the fault; the same batch on the binary heap and on a generous calendar is clean on all 8."""
import numpy as np
import pytest

import queue_exhaustion as qx
from support import amd  # noqa: F401  (fixture)

CALENDAR = 1 << 9  # lbft_batch_layout's flag word (include/lbft.h)
HISTORY = 104      # the automatic log capacity of a 400-tick run


def assert_equals_oracle(res, want, rows, what):
    got = dict(commit_counts=res.commit_counts, active_rounds=res.active_rounds, last_states=res.last_committed_states,
               histories=res.committed_histories(HISTORY))
    for key in qx.RESULT_KEYS:
        assert (got[key][rows] == want[key][rows]).all(), (what, key)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(qx.MIXED))
def test_exhausted_pool_faults_cleanly_on_the_device(amd, oracle, name):  # noqa: F811
    from librabft_simulator_amd import _lib
    kw, max_clock, queue_capacity, words = qx.MIXED[name]
    n, words = kw["num_nodes"], np.asarray(words, dtype=np.uint32)
    seeds = np.asarray(qx.MIXED_SEEDS, dtype=np.uint64)
    delay = amd.RandomDelay.uniform(kw["uniform_lo"], kw["uniform_hi"])
    want = qx.oracle_run(oracle, kw, seeds, max_clock, HISTORY)
    everyone = np.ones(len(seeds), dtype=bool)

    sim = amd.BatchSimulator.new(seeds, n, delay, queue_capacity=queue_capacity)
    res = sim.loop_until(max_clock, allow_faults=True)
    assert sim.layout()["kernel_class"] & CALENDAR
    faults = res.faults.copy()
    print(name, "faults", faults.tolist(), "host model", words.tolist())
    assert ((faults != 0) == (words != 0)).all() and ((faults & qx.F_QUEUE) == (words & qx.F_QUEUE)).all(), (faults, words)
    assert not (faults & ~np.uint32(qx.CAPACITY_BITS)).any(), faults
    assert (res.commit_counts <= HISTORY).all()
    assert_equals_oracle(res, want, faults == 0, name)

    sim.reset()  # the same run without allow_faults raises, and the handle stays usable
    with pytest.raises(amd.LbftError) as e:
        sim.loop_until(max_clock)
    assert e.value.code == -5
    sim.reset()
    _lib.check(_lib.lib().lbft_batch_set_calendar_queue(sim._h, 0))  # ... for the same batch on the binary heap, which holds every event
    res = sim.loop_until(max_clock)
    assert not sim.layout()["kernel_class"] & CALENDAR and not res.faults.any()
    assert_equals_oracle(res, want, everyone, name + " on the heap")
    sim.close()

    # the path that does not run out: the same delays on a calendar with room
    sim = amd.BatchSimulator.new(seeds, n, delay, queue_capacity=max(4096, 64 * n * n))
    res = sim.loop_until(max_clock)
    assert sim.layout()["kernel_class"] & CALENDAR and not res.faults.any()
    assert_equals_oracle(res, want, everyone, name + " with room")
    sim.close()
