"""Device tier of the edge-case table (tests/edge_cases.py): BatchSimulator / with_param_sets on the MI355X against the oracle on every case
-- commit counts, last states, histories, active rounds, startup times, fault words and the events / rng_draws / events_scheduled counters --
the kernel class and queue discipline each boundary case must select, and the refused horizons.  Every case of at most 32 nodes and every
parameter-set batch again with commit times recorded (the twins of liblbft_commit_times.so): the untimed outcome and results, commit times
equal to the oracle-derived ones, the default latency histogram equal to numpy.  Plus SimT::trunc_exp at its decision
boundary through lbft_device_sample_delays: the device's single-precision exp2 estimate and the 2e-6 margin that decides when it is trusted
are code the host build never runs."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import commit_times_oracle as cto  # noqa: E402
import edge_cases as ec  # noqa: E402
import plan_batches as pb  # noqa: E402

pytestmark = pytest.mark.gpu


def amd():
    import librabft_simulator_amd as m
    return m


def make_sim(case, commit_times=False):
    return pb.make_sim(amd(), pb.edge_batch(case, commit_times=commit_times))


def oracle_runs(oracle, case, seeds):
    cfg = ec.oracle_config(oracle, case)
    out = []
    for s in seeds:
        o = oracle.OracleSim(cfg, int(s)).run_until(case["max_clock"])
        out.append({"commit_counts": o.commit_counts(), "active_rounds": o.active_rounds(), "last_states": o.last_committed_states(),
                    "startup_times": o.startup_times(), "histories": [o.committed_history(k) for k in range(case["n"])],
                    "counters": o.counters()})
        o.close()
    return out


def assert_instances_equal(res, idx, refs, name):
    hist = res.committed_histories(max(1, int(res.commit_counts.max())))
    for i, r in zip(idx, refs):
        assert list(res.commit_counts[i]) == r["commit_counts"], (name, i)
        assert list(res.active_rounds[i]) == r["active_rounds"], (name, i)
        assert list(res.last_committed_states[i]) == r["last_states"], (name, i)
        assert list(res.startup_times[i]) == r["startup_times"], (name, i)
        for k, h in enumerate(r["histories"]):
            assert (hist[i, k, :len(h)] == h).all(), (name, i, k)


def sum_counters(refs):
    return {k: (np.sum([r["counters"][k] for r in refs], axis=0).tolist() if k == "events" else sum(r["counters"][k] for r in refs))
            for k in ec.COMPARED_COUNTERS}


@pytest.mark.parametrize("case", [c for c in ec.CASES if ec.expected(c)[0] != "refused" and not c.get("host_only")], ids=lambda c: c["name"])
def test_edge_case_device(oracle, case):
    kind, arg = ec.expected(case)
    sim = make_sim(case)
    res = sim.loop_until(case["max_clock"], allow_faults=True)
    flags = sim.layout()["kernel_class"]
    if "kernel_class" in case:
        assert flags & 0xff == case["kernel_class"], (case["name"], hex(flags))
    if "calendar" in case:
        assert bool(flags & ec.LAYOUT_CALENDAR) == case["calendar"], (case["name"], hex(flags))
    # the table's own statement of the class and queue discipline (the CPU tier runs the host build with the planner's)
    assert (flags & 0xff, (flags >> 8) & 1, (flags >> 9) & 1, (flags >> 11) & 1) == ec.expected_layout(case), (case["name"], hex(flags))
    if kind == "fault":
        assert (res.faults == arg).all(), (case["name"], res.faults)
        return
    assert (res.faults == 0).all(), (case["name"], res.faults)
    refs = oracle_runs(oracle, case, case["seeds"])
    assert_instances_equal(res, range(len(refs)), refs, case["name"])
    ctr, want = res.counters, sum_counters(refs)
    assert list(ctr["events"]) == want["events"], (case["name"], ctr["events"], want["events"])
    assert ctr["rng_draws"] == want["rng_draws"] and ctr["events_scheduled"] == want["events_scheduled"], (case["name"], ctr, want)


@pytest.mark.parametrize("entry", pb.recorded(), ids=lambda e: e["name"])
def test_recorded_layout_on_the_device(entry):
    """The library still reports, for every batch of tests/plan_batches.py, what it reported before the planner moved into
    csrc/lbft_plan.h (tests/golden/plan_layouts.json)."""
    spec = pb.BATCHES[entry["name"]]
    sim = pb.make_sim(amd(), spec)
    sim.loop_until(pb.max_clock_of(spec), allow_faults=True)
    got = list(sim.layout().values())
    assert got == entry["layout"], (entry["name"], got, hex(got[7]), hex(entry["layout"][7]))
    assert sim.device_bytes() == entry["device_bytes"], entry["name"]
    sim.close()


def test_calendar_limit_on_the_device(oracle):
    """16 383 on the calendar and 16 383 with the calendar switched off give the same results instance by instance (the table runs each of
    them, and 16 384 on the heap, against the oracle)."""
    runs = []
    for name in ("calendar_last_horizon", "calendar_last_horizon_heap"):
        case = ec.by_name(name)
        sim = make_sim(case)
        res = sim.loop_until(case["max_clock"])
        runs.append((res.commit_counts.copy(), res.last_committed_states.copy(), res.active_rounds.copy()))
    for a, b in zip(*runs):
        assert (a == b).all()


@pytest.mark.parametrize("case", [c for c in ec.CASES if ec.expected(c)[0] == "refused"], ids=lambda c: c["name"])
def test_refused_on_the_device(case):
    m = amd()
    _, code = ec.expected(case)
    if not case["name"].startswith("max_clock"):
        with pytest.raises(m.LbftError) as e:
            make_sim(case)
        assert e.value.code == code
        return
    sim = make_sim(case)
    assert m._lib.lib().lbft_batch_run_until(sim._h, case["max_clock"]) == code
    assert m._lib.lib().lbft_batch_run_steps(sim._h, case["max_clock"], 0, ctypes.byref(ctypes.c_uint64())) == code
    res = sim.loop_until(ec.MAX_CLOCK_LIMIT)  # the same batch takes the largest accepted horizon
    assert (res.faults == 0).all()


def make_param_set_sim(case, commit_times=False):
    set_of, seeds = ec.set_layout(case)
    sim = pb.make_sim(amd(), dict(sets=case["name"], commit_times=commit_times))
    return sim, np.array(set_of, dtype=np.uint32), np.array(seeds, dtype=np.uint64)


@pytest.mark.parametrize("case", ec.PARAM_SET_CASES, ids=lambda c: c["name"])
def test_param_set_edge_batch_device(oracle, case):
    sim, set_of, seeds = make_param_set_sim(case)
    res = sim.loop_until(case["max_clock"], allow_faults=True)
    flags = sim.layout()["kernel_class"]
    assert flags & (1 << 16) and flags & 0xff == case["kernel_class"], hex(flags)
    for k in range(len(case["sets"])):
        idx = np.nonzero(set_of == k)[0]
        sub = ec.set_as_case(case, k)
        kind, arg = ec.expected(sub)
        if kind == "fault":
            assert (res.faults[idx] == arg).all(), (k, res.faults[idx])
            continue
        assert (res.faults[idx] == 0).all(), (k, res.faults[idx])
        assert_instances_equal(res, idx, oracle_runs(oracle, sub, seeds[idx]), sub["name"])


# ---- the same cases on the commit-time twins (lbft_k_ct_*) -------------------------------------------------------------------------------
HOST_THREADS = min(os.cpu_count() or 8, 16)


@pytest.mark.parametrize("case", [c for c in ec.CASES if ec.expected(c)[0] != "refused" and not c.get("host_only") and c["n"] <= 32],
                         ids=lambda c: c["name"])
def test_edge_case_with_commit_times(oracle, case):
    """Every case again on a batch that records commit times: the untimed outcome and results, commit times equal to the ones derived
    from fresh oracle runs, and the default latency histogram (at the largest horizon: width 32 768, 65 536 bins, 8 passes) equal to numpy."""
    kind, arg = ec.expected(case)
    mc = case["max_clock"]
    plain = make_sim(case)
    rp = plain.loop_until(mc, allow_faults=True)
    timed = make_sim(case, commit_times=True)
    rt = timed.loop_until(mc, allow_faults=True)
    flags = timed.layout()["kernel_class"]
    assert flags & (1 << 17) and flags & 0xff == ec.expected_layout(case)[0], (case["name"], hex(flags))
    assert (rt.faults == (arg if kind == "fault" else 0)).all(), (case["name"], rt.faults)
    cto.same_results(rt, rp)
    ct = rt.commit_times()
    assert ((ct >= 0).sum(axis=2) == rt.commit_counts).all()
    if kind == "equal":
        ref = cto.commit_times(oracle, ec.oracle_config(oracle, case), np.array(case["seeds"], dtype=np.uint64), mc, ct.shape[2], HOST_THREADS)
        assert (ct == ref).all(), case["name"]
    cto.check_default_latency(rt, mc)
    plain.close()
    timed.close()


@pytest.mark.parametrize("case", ec.PARAM_SET_CASES, ids=lambda c: c["name"])
def test_param_set_edge_batch_with_commit_times(oracle, case):
    mc = case["max_clock"]
    plain, set_of, seeds = make_param_set_sim(case)
    rp = plain.loop_until(mc, allow_faults=True)
    timed, _, _ = make_param_set_sim(case, commit_times=True)
    rt = timed.loop_until(mc, allow_faults=True)
    flags = timed.layout()["kernel_class"]
    assert flags & (1 << 16) and flags & (1 << 17) and flags & 0xff == case["kernel_class"], hex(flags)
    cto.same_results(rt, rp)
    ct = rt.commit_times()
    assert ((ct >= 0).sum(axis=2) == rt.commit_counts).all()
    for k in range(len(case["sets"])):
        idx = np.nonzero(set_of == k)[0]
        sub = ec.set_as_case(case, k)
        kind, arg = ec.expected(sub)
        assert (rt.faults[idx] == (arg if kind == "fault" else 0)).all(), (k, rt.faults[idx])
        if kind == "equal":
            ref = cto.commit_times(oracle, ec.oracle_config(oracle, sub), seeds[idx], mc, ct.shape[2], HOST_THREADS)
            assert (ct[idx] == ref).all(), sub["name"]
    cto.check_default_latency(rt, mc, set_of, len(case["sets"]))
    plain.close()
    timed.close()


# ---- SimT::trunc_exp at its decision boundary --------------------------------------------------------------------------------------------
def _boundary_means():
    """Means for variance-0 samples (every sample is trunc_exp(ln(mean))): integers of every octave up to 2^20 and their float neighbours,
    means that put exp(y) just inside / just outside the 2e-6 a margin, means in (0, 1), means where |y log2 e| is close to 20."""
    rng = np.random.default_rng(20261015)
    ks = set()
    for e in range(21):
        lo, hi = 1 << e, 1 << (e + 1)
        ks.update(int(v) for v in rng.integers(lo, min(hi, (1 << 20) + 2), size=24))
        ks.update((lo, lo + 1, hi - 1))
    means = []
    for k in sorted(ks):
        means += [float(k), math.nextafter(float(k), 0.0), math.nextafter(float(k), math.inf)]
    for k in (3, 17, 1000, 4097, 65537, 300001, 1000003):
        for r in (1.5e-6, 1.9e-6, 2.1e-6, 2.5e-6, 8e-7, 1e-7):
            means += [k * (1 + r), k * (1 - r), (k + 1) - k * r, k + k * r]
    means += [float(v) for v in np.concatenate([rng.uniform(1e-7, 1.0, 64), np.geomspace(1e-7, 1.0, 64)])]
    for t in (20.0, 19.9999999, 19.999999, 20.000001, -20.0, -19.999999, -20.000001):
        means += [2.0 ** t, math.nextafter(2.0 ** t, 0.0), math.nextafter(2.0 ** t, math.inf)]
    return [v for v in means if v > 0.0]


def test_trunc_exp_decision_boundary_on_the_device(oracle):
    m = amd()
    L, OL = m._lib.lib(), oracle.lib()
    from librabft_simulator_amd.simulator import make_config
    means = _boundary_means()
    got = np.zeros(len(means), dtype=np.int64)
    one = np.zeros(1, dtype=np.int64)
    for j, mean in enumerate(means):
        cfg = make_config(4, m.RandomDelay.new(mean, 0.0), m.NodeConfig())
        m._lib.check(L.lbft_device_sample_delays(0, ctypes.byref(cfg), 7, one.ctypes.data, 1))
        got[j] = one[0]
    want = np.array([int(math.exp(math.log(v))) for v in means], dtype=np.int64)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(means[i], int(got[i]), int(want[i])) for i in bad[:10]]
    for mode in (0, 1):
        for j, mean in enumerate(means):
            OL.lbft_oracle_sample_delays(ctypes.byref(oracle.make_config(mean=mean, variance=0.0, math_mode=mode)), 7, one.ctypes.data, 1)
            assert one[0] == got[j], (mode, mean, int(one[0]), int(got[j]))
    # the sweep does reach the slow path: integers whose float estimate sits inside the margin
    assert sum(1 for v in means if v >= 1.0 and abs(v - round(v)) < 2e-6 * v) > 500
    # dense sprays around integers of every octave: y = mu + sigma * N(0, 1) with sigma ~ 1e-6, so exp(y) falls within a few 1e-6 of k,
    # on both sides of the margin
    n = 20000
    a, b = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for e in range(1, 21):
        for k in ((1 << e) - 1, (3 << e) // 2 + 1):
            if k > 1 << 20:
                continue
            for rel in (4e-7, 1.5e-6):
                cfg = make_config(4, m.RandomDelay.new(float(k), (k * rel) ** 2), m.NodeConfig())
                m._lib.check(L.lbft_device_sample_delays(0, ctypes.byref(cfg), 1000 + e, b.ctypes.data, n))
                for mode in (0, 1):
                    OL.lbft_oracle_sample_delays(ctypes.byref(oracle.make_config(mean=float(k), variance=(k * rel) ** 2, math_mode=mode)),
                                                 1000 + e, a.ctypes.data, n)
                    assert (a == b).all(), (k, rel, mode, int((a != b).sum()))


def test_headline_kernel_takes_the_samplers_decision(oracle):
    """A full run on the headline kernel (4 nodes, log-normal delays, > 8 networks per wavefront) with a fixed delay at a mean where
    exp(ln(mean)) < mean, so every delay is mean - 1 -- decided by the same trunc_exp as the sampler entry point."""
    m = amd()
    k = next(k for k in range(9, 100) if math.exp(math.log(k)) < k)
    seeds = np.arange(1, 32769, dtype=np.uint64)
    sim = m.BatchSimulator.new(seeds, 4, m.RandomDelay.new(float(k), 0.0))
    res = sim.loop_until(1000)
    assert sim.layout()["kernel_class"] & (1 << 14), sim.layout()
    assert (res.faults == 0).all()
    idx = np.arange(0, len(seeds), 2048)
    ref = oracle.run_batch(oracle.make_config(num_nodes=4, mean=float(k), variance=0.0, math_mode=1), seeds[idx], 1000, history_cap=64)
    assert (res.commit_counts[idx] == ref["commit_counts"]).all()
    assert (res.last_committed_states[idx] == ref["last_states"]).all()
    assert (res.committed_histories(64)[idx] == ref["histories"]).all()
    assert (res.startup_times[idx] == k).all()  # 0 + (k - 1) + 1
