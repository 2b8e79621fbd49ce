"""An exhausted chunk pool of the calendar queue faults cleanly (CPU only).  tests/queue_exhaustion_host.cpp -- the host build of the kernel logic as
a stand-alone program with a fence around every instance -- runs the cases of tests/queue_exhaustion.py twice: built plain (-O2), and under the
address and undefined-behaviour sanitizers.  The fence sees an access that leaves the instance's rows (the host model keeps all instances in one
vector, where a sanitizer sees nothing), the sanitizers one that leaves the vector.  A crash of the program is an exit status.  Every assertion is
exact and the oracle is oracle.run_batch with the same configuration.

Before push_event / bulk_append dropped the event of an exhausted pool (they handed out chunk cal_chunks - 1, "in bounds", live or not), the first,
third and fourth regression case ended in a segmentation fault of the plain build, the second in the fault words [1, 1, 577], and every one left
cal_free and cal_bump above cal_chunks (532 / 526 / 508 of 360 in the second)."""
import subprocess

import numpy as np
import pytest

import queue_exhaustion as qx


@pytest.fixture(scope="module", params=["plain", "sanitizers"])
def program(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("qex_" + request.param)
    if request.param == "sanitizers":
        probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input="int main(){}",
                               capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip("the sanitizer runtimes are not installed")
    return qx.compile_program(str(tmp / "queue_exhaustion_host"), request.param == "sanitizers")


def run(program, cases):
    status, out, err = qx.run_program(program, cases)
    assert status == 0 and len(out) == len(cases), ("exit status %d after %d of %d cases" % (status, len(out), len(cases)), err)
    assert all(d["rc"] >= 0 for d in out), [d["rc"] for d in out]
    return out


_STATS = {}


def count(program, d):
    for k, v in d["stats"].items():
        _STATS.setdefault(program, dict.fromkeys(qx.STATS, 0))[k] += v


# ---- (a) the cases that crashed ----
@pytest.mark.parametrize("name", sorted(qx.REGRESSION))
def test_regression_cases_fault_cleanly(program, oracle, name):
    kw, max_clock, caps = qx.REGRESSION[name]
    d, = run(program, [(kw, max_clock, caps, qx.REGRESSION_SEEDS, caps["lcap"])])
    print(name, "faults", d["faults"], "maxq", d["maxq"], "pool", d["cal_bump"], d["cal_chunks"], d["stats"])
    count(program, d)
    qx.assert_faulted_cleanly(d, caps, name)
    assert ((d["faults"] == 0) | (d["faults"] & qx.F_QUEUE != 0)).all()
    assert d["faults"].any(), name  # (these are the cases that exhaust the pool)
    assert (d["maxq"][d["faults"] != 0] < caps["qcap"]).all(), name  # ... and not the queue
    qx.assert_clean_equal(qx.oracle_run(oracle, kw, qx.REGRESSION_SEEDS, max_clock, caps["lcap"]), d, d["faults"], name)


def test_the_sizing_gap_remains(oracle):
    """The capacity regression against the heap that is still open: 20 nodes, uniform [20, 120], queue_capacity 3200 --
    the binary heap holds every event (clean, equal to the oracle), the calendar's pool runs out below 3200 entries."""
    kw, max_clock, caps = qx.REGRESSION["n20_u20_120_heap_is_clean"]
    seeds = np.asarray(qx.REGRESSION_SEEDS, dtype=np.uint64)
    cfg = oracle.make_config(math_mode=1, **kw)
    want = oracle.run_batch(cfg, seeds, max_clock, threads=4, history_cap=64)
    heap = oracle.hostmodel_run_batch(cfg, seeds, max_clock, threads=3, history_cap=64, **dict(caps, qcal=0))
    assert not heap["faults"].any() and (heap["maxq"] < caps["qcap"]).all()
    qx.assert_clean_equal(want, heap, heap["faults"], "heap")
    cal = oracle.hostmodel_run_batch(cfg, seeds, max_clock, threads=3, history_cap=64, **caps)
    assert (cal["faults"] == qx.F_QUEUE).all() and (cal["maxq"] < caps["qcap"]).all()


# ---- (b) batches where some instances exhaust the pool and their neighbours do not ----
@pytest.mark.parametrize("name", sorted(qx.MIXED))
def test_mixed_batches_leave_the_neighbours_exact(program, oracle, name):
    kw, max_clock, queue_capacity, words = qx.MIXED[name]
    caps = qx.planned_caps(oracle, kw, len(qx.MIXED_SEEDS), max_clock, queue_capacity)
    assert caps["qcal"] == 1 and (caps["ring"], caps["tw"]) == ((512, 1) if kw["num_nodes"] > 32 else (0, 64)), caps
    d, = run(program, [(kw, max_clock, caps, qx.MIXED_SEEDS, caps["lcap"])])
    print(name, caps, "faults", d["faults"], "maxq", d["maxq"], d["stats"])
    count(program, d)
    qx.assert_faulted_cleanly(d, caps, name, allowed=qx.F_QUEUE)
    assert d["faults"].tolist() == list(words), name
    faulted = int((d["faults"] != 0).sum())
    assert 1 <= faulted <= len(words) // 2
    assert (d["maxq"][d["faults"] != 0] < caps["qcap"]).all()  # the pool ran out, not the queue
    clean = qx.assert_clean_equal(qx.oracle_run(oracle, kw, qx.MIXED_SEEDS, max_clock, caps["lcap"]), d, d["faults"], name)
    assert clean.sum() == len(words) - faulted
    # the tiled class takes push_event's branches, the cooperative loop bulk_append's as well
    assert d["stats"]["empty_bucket"] > 0 if kw["num_nodes"] <= 32 else d["stats"]["bulk_1"] > 0


# ---- (c) every branch of the exhausted pool ----
@pytest.mark.parametrize("name", sorted(qx.BRANCHES))
def test_branch_cases_fault_cleanly(program, oracle, name):
    kw, max_clock, caps, seeds, must = qx.BRANCHES[name]
    d, = run(program, [(kw, max_clock, caps, seeds, caps["lcap"])])
    print(name, "faults", d["faults"], "maxq", d["maxq"], d["stats"])
    count(program, d)
    qx.assert_faulted_cleanly(d, caps, name, allowed=qx.F_QUEUE)
    assert d["faults"].any() and (d["maxq"][d["faults"] != 0] < caps["qcap"]).all()
    assert all(d["stats"][k] > 0 for k in must), (name, d["stats"])
    qx.assert_clean_equal(qx.oracle_run(oracle, kw, seeds, max_clock, caps["lcap"]), d, d["faults"], name)


def test_every_branch_was_reached(program, oracle):
    """Exhaustion on an empty bucket, on a full tail chunk, in bulk_append for a group that needed 1, 2 and 3 new chunks, and with a stack of freed
    chunks that is not empty but too short: each at least once over the cases above (selected alone, this test runs the branch cases itself)."""
    if not all(_STATS.get(program, {}).get(k) for k in qx.STATS):
        for name in sorted(qx.BRANCHES):
            kw, max_clock, caps, seeds, _ = qx.BRANCHES[name]
            count(program, run(program, [(kw, max_clock, caps, seeds, 0)])[0])
    print(_STATS[program])
    assert all(_STATS[program][k] > 0 for k in qx.STATS), _STATS[program]


# ---- (d) on used memory ----
def test_exhaustion_on_dirty_state(program, oracle):
    """A regression case started on rows that hold 0xDEADBEEF (tests/test_dirty_state_host.py's used batch): the same fault words, pool words and
    results as on fresh pages -- the chunk links, the free stack and the entries the dropped events never wrote are not read either."""
    for name in ("n20_u0_250", "n40_u0_300_coop512"):
        kw, max_clock, caps = qx.REGRESSION[name]
        fresh, dirty = run(program, [(kw, max_clock, dict(caps, state_fill=fill), qx.REGRESSION_SEEDS, caps["lcap"]) for fill in (0, 0xDEADBEEF)])
        qx.assert_faulted_cleanly(dirty, caps, name)
        for key in ("faults", "maxq", "maxsnap", "cal_free", "cal_bump") + qx.RESULT_KEYS:
            assert (fresh[key] == dirty[key]).all(), (name, key)
        assert fresh["stats"] == dirty["stats"]


# ---- (e) small capacities, drawn ----
def test_drawn_small_capacities_fault_cleanly(program, oracle):
    draws = qx.fuzz_draws(oracle)
    out = run(program, [(kw, max_clock, caps, seeds, caps["lcap"]) for kw, max_clock, caps, seeds, _ in draws])
    ended_clean = ended_faulted = 0
    for (kw, max_clock, caps, seeds, allowed), d in zip(draws, out):
        what = (kw, max_clock, caps)
        qx.assert_faulted_cleanly(d, caps, what, allowed=allowed)
        qx.assert_clean_equal(qx.oracle_run(oracle, kw, seeds, max_clock, caps["lcap"]), d, d["faults"], what)
        ended_clean += not d["faults"].any()
        ended_faulted += bool(d["faults"].any())
    print("draws", len(draws), "clean", ended_clean, "faulted", ended_faulted)
    assert 3 * ended_clean >= len(draws) and 3 * ended_faulted >= len(draws), (len(draws), ended_clean, ended_faulted)
