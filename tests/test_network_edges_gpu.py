"""Device tier of the network edge-case table (tests/network_edge_cases.py): BatchSimulator on the MI355X against the oracle on every
accepted case -- commit counts, active rounds, last states, startup times, histories per instance, the summed events / rng_draws /
events_scheduled counters, the fault words -- and the kernel family each case pins.  Every case of at most 32 nodes again on the
commit-time twins: the untimed results, commit times equal to the oracle-derived ones, the default latency histogram.  The parameter-set
batches plain and timed, per set against the oracle.  The weighted cases through finality_histogram() and chain_stats(): zero and 24-bit
rights in the thresholds.  The refused configurations through the Python API.  The CPU tier is tests/test_network_edges_host.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chain_stats_reference as chain_ref  # noqa: E402
import commit_times_oracle as cto  # noqa: E402
import network_edge_cases as nec  # noqa: E402
import support  # noqa: E402
from test_edge_cases_gpu import assert_instances_equal, oracle_runs, sum_counters  # noqa: E402

pytestmark = pytest.mark.gpu
HOST_THREADS = min(os.cpu_count() or 8, 16)
TIMED = [c for c in nec.CASES if c["n"] <= 32]
WEIGHTED = [c for c in nec.CASES if c.get("weighted")]


def amd():
    import librabft_simulator_amd as m
    return m


def timed_clock(case):
    return case.get("timed_max_clock", case["max_clock"])


@pytest.mark.parametrize("case", nec.CASES, ids=lambda c: c["name"])
def test_network_edge_case_device(oracle, case):
    kind, arg = nec.expected(case)
    sim = nec.make_sim(amd(), case)
    res = sim.loop_until(case["max_clock"], allow_faults=True)
    nec.check_layout_flags(case, sim.layout()["kernel_class"])
    if kind == "fault":
        assert (res.faults == arg).all(), (case["name"], res.faults)
        sim.close()
        return
    assert (res.faults == 0).all(), (case["name"], res.faults)
    refs = oracle_runs(oracle, case, case["seeds"])
    assert_instances_equal(res, range(len(refs)), refs, case["name"])
    ctr, want = res.counters, sum_counters(refs)
    assert list(ctr["events"]) == want["events"], (case["name"], ctr["events"], want["events"])
    assert ctr["rng_draws"] == want["rng_draws"] and ctr["events_scheduled"] == want["events_scheduled"], (case["name"], ctr, want)
    sim.close()


def test_the_table_reaches_every_kernel_family_on_the_device():
    """What the cases pin, taken together: class 1 on the array and on the calendar, the lean class 2, the exchange kernel, class 0."""
    pins = [nec.layout_flags(c) for c in nec.CASES]
    assert any(p.get("kernel_class") == 1 and p.get("calendar") is False for p in pins)
    assert any(p.get("kernel_class") == 1 and p.get("calendar") is True for p in pins)
    assert any(p.get("kernel_class") == 2 and p.get("lean") is True and p.get("exchange") is False for p in pins)
    assert any(p.get("kernel_class") == 2 and p.get("exchange") is True for p in pins)
    assert any(p.get("kernel_class") == 0 for p in pins)


@pytest.mark.parametrize("case", TIMED, ids=lambda c: c["name"])
def test_network_edge_case_with_commit_times(oracle, case):
    """The case again on a batch that records commit times (at the case's timed_max_clock where the table gives one: the oracle derives
    commit times by bisection over fresh runs, one per clock tick with a commit)."""
    kind, arg = nec.expected(case)
    mc = timed_clock(case)
    plain = nec.make_sim(amd(), case)
    rp = plain.loop_until(mc, allow_faults=True)
    timed = nec.make_sim(amd(), case, commit_times=True)
    rt = timed.loop_until(mc, allow_faults=True)
    flags = timed.layout()["kernel_class"]
    assert flags & (1 << 17) and flags & 0xff == plain.layout()["kernel_class"] & 0xff, (case["name"], hex(flags))
    assert (rt.faults == (arg if kind == "fault" else 0)).all(), (case["name"], rt.faults)
    cto.same_results(rt, rp)
    ct = rt.commit_times()
    assert ((ct >= 0).sum(axis=2) == rt.commit_counts).all()
    if kind == "equal":
        ref = cto.commit_times(oracle, nec.oracle_config(oracle, case), np.array(case["seeds"], dtype=np.uint64), mc, ct.shape[2], HOST_THREADS)
        assert (ct == ref).all(), case["name"]
    cto.check_default_latency(rt, mc)
    plain.close()
    timed.close()


# ---- parameter-set batches ---------------------------------------------------------------------------------------------------------------------
def make_param_set_sim(case, commit_times=False):
    m = amd()
    set_of, seeds = nec.set_layout(case)
    set_of, seeds = np.array(set_of, dtype=np.uint32), np.array(seeds, dtype=np.uint64)
    sim = m.BatchSimulator.with_param_sets(seeds, case["n"], nec.param_sets(m, case), set_of, commit_times=commit_times, **nec.base_kwargs(case))
    return sim, set_of, seeds


@pytest.mark.parametrize("case", nec.PARAM_SET_CASES, ids=lambda c: c["name"])
def test_network_param_set_batch_device(oracle, case):
    """Per set equal to the oracle; the ordinary set 0 is the loss-free plain run, untouched by its neighbours' loss and partition words."""
    sim, set_of, seeds = make_param_set_sim(case)
    res = sim.loop_until(case["max_clock"], allow_faults=True)
    flags = sim.layout()["kernel_class"]
    assert flags & (1 << 16) and flags & 0xff == case["kernel_class"], hex(flags)
    assert (res.faults == 0).all(), res.faults
    for k in range(len(case["sets"])):
        idx = np.nonzero(set_of == k)[0]
        sub = nec.set_as_case(case, k)
        assert_instances_equal(res, idx, oracle_runs(oracle, sub, seeds[idx]), sub["name"])
    sim.close()


@pytest.mark.parametrize("case", nec.PARAM_SET_CASES, ids=lambda c: c["name"])
def test_network_param_set_batch_with_commit_times(oracle, case):
    mc = case["max_clock"]
    plain, set_of, seeds = make_param_set_sim(case)
    rp = plain.loop_until(mc, allow_faults=True)
    timed, _, _ = make_param_set_sim(case, commit_times=True)
    rt = timed.loop_until(mc, allow_faults=True)
    flags = timed.layout()["kernel_class"]
    assert flags & (1 << 16) and flags & (1 << 17) and flags & 0xff == case["kernel_class"], hex(flags)
    assert (rt.faults == 0).all(), rt.faults
    cto.same_results(rt, rp)
    ct = rt.commit_times()
    assert ((ct >= 0).sum(axis=2) == rt.commit_counts).all()
    for k in range(len(case["sets"])):
        idx = np.nonzero(set_of == k)[0]
        sub = nec.set_as_case(case, k)
        ref = cto.commit_times(oracle, nec.oracle_config(oracle, sub), seeds[idx], mc, ct.shape[2], HOST_THREADS)
        assert (ct[idx] == ref).all(), sub["name"]
    cto.check_default_latency(rt, mc, set_of, len(case["sets"]))
    plain.close()
    timed.close()


# ---- zero and 24-bit rights in the thresholds of the device statistics ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", WEIGHTED, ids=lambda c: c["name"])
def test_weighted_case_finality_and_chain_statistics(oracle, case):
    cfg, mc = case["cfg"], timed_clock(case)
    seeds = np.array(case["seeds"], dtype=np.uint64)
    sim = nec.make_sim(amd(), case, commit_times=True)
    res = sim.loop_until(mc)
    assert res.commit_counts.max() > 0, case["name"]
    support.check_finality(res, mc, [(None, None), (5, 20)], rights=cfg["voting_rights"], rotation=cfg.get("rights_rotation", 0),
                           commands_per_epoch=cfg.get("commands_per_epoch", 30000))
    want = chain_ref.oracle_batch(oracle, nec.oracle_config(oracle, case), seeds, mc)
    support.check_chain_stats(res, want, mc, [(None, None), (5, 20)])
    sim.close()


# ---- refused -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nec.REFUSED, ids=lambda c: c["name"])
def test_refused_network_configuration_on_the_device(case):
    m = amd()
    cfg = dict(case["cfg"])
    delay = m.RandomDelay(model=cfg.pop("delay_model", 0))
    with pytest.raises(m.LbftError) as e:
        m.BatchSimulator.new(np.array([1, 2], dtype=np.uint64), case["n"], delay, m.NodeConfig(),
                             voting_rights=cfg.pop("voting_rights", None) if case["n"] else None, **cfg)
    assert e.value.code == case["code"]


@pytest.mark.parametrize("case", nec.REFUSED_PARAM_SETS, ids=lambda c: c["name"])
def test_refused_param_set_arguments_on_the_device(case):
    m = amd()
    sets = [m.ParamSet() for _ in range(case["n_sets"])]
    set_of = np.array(case["set_of"], dtype=np.uint32)
    seeds = np.arange(1, len(set_of) + 1, dtype=np.uint64)
    if not sets:  # Python refuses an empty list itself; the C ABI's answer is the CPU tier's
        with pytest.raises(ValueError):
            m.BatchSimulator.with_param_sets(seeds, case["n"], sets, set_of)
        return
    with pytest.raises(m.LbftError) as e:
        m.BatchSimulator.with_param_sets(seeds, case["n"], sets, set_of)
    assert e.value.code == case["code"]
