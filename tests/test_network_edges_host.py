"""CPU tier of the network edge-case table (tests/network_edge_cases.py): the host build of the kernel logic (oracle/host_model.cpp) against
the oracle on every accepted case with the capacities and queue discipline the planner chooses -- the four result arrays, the three
counters, the fault word --; the identities the oracle itself must satisfy (a loss of 2^32 - 1 is a loss of 1 000 000, a partition that
holds everybody or whose window is empty, reversed or outside the horizon cuts nothing, rotations are taken modulo num_nodes ...); the
parameter-set batches through the host build of the parameter-set classes; the refused configurations through the C ABI, which decides
them before any HIP call; and every accepted case once through the fenced stand-alone program (tests/queue_exhaustion_host.cpp), built
plain and under the address and undefined-behaviour sanitizers.  The device tier is tests/test_network_edges_gpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import network_edge_cases as nec  # noqa: E402
import queue_exhaustion as qx  # noqa: E402
import test_param_sets_host_model as psh  # noqa: E402  (run_host: the host build of the parameter-set classes)
from test_param_sets_host_model import harness  # noqa: E402,F401  (the fixture that compiles it)

ACCEPTED = nec.CASES
_ORACLE = {}


def seeds_of(case):
    return np.array(case["seeds"], dtype=np.uint64)


def oracle_run(oracle, case):
    """The oracle's run of a case: computed once, shared by the tests of this module, never modified."""
    if case["name"] not in _ORACLE:
        _ORACLE[case["name"]] = oracle.run_batch(nec.oracle_config(oracle, case), seeds_of(case), case["max_clock"], threads=8,
                                                 history_cap=nec.HISTORY_CAP)
    return _ORACLE[case["name"]]


def planned_flags(oracle, case):
    return oracle.plan(nec.oracle_config(oracle, case), len(case["seeds"]), case["max_clock"], block_capacity=case.get("block_capacity", 0))["layout"][7]


@pytest.mark.parametrize("case", ACCEPTED, ids=lambda c: c["name"])
def test_network_edge_case_host_model(oracle, case):
    kind, arg = nec.expected(case)
    got = oracle.hostmodel_run_batch(nec.oracle_config(oracle, case), seeds_of(case), case["max_clock"], threads=8, history_cap=nec.HISTORY_CAP,
                                     **nec.host_caps(case))
    nec.check_layout_flags(case, planned_flags(oracle, case))
    if kind == "fault":
        assert (got["faults"] == arg).all(), (case["name"], got["faults"], arg)
        return
    ref = oracle_run(oracle, case)
    assert (got["faults"] == 0).all(), (case["name"], got["faults"])
    for key in nec.COMPARED:
        assert (got[key] == ref[key]).all(), (case["name"], key)
    for key in nec.COMPARED_COUNTERS:
        assert got["counters"][key] == ref["counters"][key], (case["name"], key, got["counters"][key], ref["counters"][key])


def test_the_table_reaches_every_kernel_family(oracle):
    """Class 1 on the array and on the calendar, the lean class 2, the exchange kernel, the full class 2, class 0."""
    reached = set()
    for case in ACCEPTED:
        f = planned_flags(oracle, case)
        reached.add((f & 0xff, bool(f & nec.LAYOUT_CALENDAR), bool(f & nec.LAYOUT_LEAN), bool(f & nec.LAYOUT_EXCHANGE)))
    for family in ((1, False, False, False), (1, True, False, False), (1, True, True, False), (2, True, True, False), (2, True, True, True),
                   (2, True, False, False), (0, False, False, False)):
        assert family in reached, (family, sorted(reached))


def test_class_0_takes_neither_loss_nor_cut_nor_equivocators(oracle):
    for case in ACCEPTED:
        if planned_flags(oracle, case) & 0xff == 0:
            assert not set(case["cfg"]) & {"drop_per_million", "partition_size", "equivocate_every"}, case["name"]


# ---- what the oracle itself says at these values -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(nec.SAME_AS))
def test_oracle_identities(oracle, name):
    case = nec.by_name(name)
    a = oracle_run(oracle, case)
    twin = dict(case, cfg=dict(case["cfg"], **nec.SAME_AS[name]))
    b = oracle.run_batch(nec.oracle_config(oracle, twin), seeds_of(case), case["max_clock"], threads=8, history_cap=nec.HISTORY_CAP)
    for key in nec.COMPARED:
        assert (a[key] == b[key]).all(), (name, key)
    assert a["counters"] == b["counters"], name


def test_oracle_facts_of_the_loss_and_partition_ends(oracle):
    for name, events in nec.ORACLE_EVENTS.items():
        assert oracle_run(oracle, nec.by_name(name))["counters"]["events"] == events, name
    one = oracle_run(oracle, nec.by_name("loss_1_per_million"))["commit_counts"]
    assert one.min() == 30 and one.max() == 35, (one.min(), one.max())
    # a rotation that is no multiple of num_nodes does change the run (the identities above are not vacuous)
    case = nec.by_name("rotation_13_on_5_nodes")
    still = oracle.run_batch(nec.oracle_config(oracle, dict(case, cfg=dict(case["cfg"], rights_rotation=0))), seeds_of(case), case["max_clock"],
                             history_cap=nec.HISTORY_CAP)
    assert (still["last_states"] != oracle_run(oracle, case)["last_states"]).any()
    # ... and so does the cut the partition cases vary
    cut = oracle.run_batch(oracle.make_config(num_nodes=4, math_mode=1, **nec.CUT), np.array([1, 2, 3], dtype=np.uint64), 1000, history_cap=nec.HISTORY_CAP)
    assert (cut["last_states"] != oracle_run(oracle, nec.by_name("partition_size_n"))["last_states"]).any()


def test_the_heavy_loss_rates_are_the_heaviest_live_ones(oracle):
    """40 nodes to clock 300, seeds 1..3: none of 300 000 / 500 000 / 700 000 commits anything; on the ladder below them the heaviest rate at
    which every seed still commits is the table's -- every node with the record exchange, some node without it."""
    seeds = np.array([1, 2, 3], dtype=np.uint64)

    def counts(rate, quirks):
        return oracle.run_batch(oracle.make_config(num_nodes=40, math_mode=1, drop_per_million=rate, quirks=quirks), seeds, 300, threads=3)["commit_counts"]

    for quirks in (0, 1):
        for rate in (300000, 500000, 700000):
            assert counts(rate, quirks).max() == 0, (rate, quirks)
    live = [r for r in nec.LOSS_LADDER if (counts(r, 0).max(axis=1) > 0).all()]
    live_exchange = [r for r in nec.LOSS_LADDER if (counts(r, 1).min(axis=1) > 0).all()]
    assert max(live) == nec.HEAVY_LOSS and max(live_exchange) == nec.HEAVY_LOSS_EXCHANGE, (live, live_exchange)


def test_the_cases_keep_the_comparison_honest(oracle):
    """Two thirds of the `equal` cases have every node of every instance committing; the cases where nobody commits still process timers,
    draw random numbers and schedule events, so their counters compare something."""
    equal = [c for c in ACCEPTED if nec.expected(c)[0] == "equal"]
    everybody = [c["name"] for c in equal if oracle_run(oracle, c)["commit_counts"].min() >= 1]
    print("every node commits in %d of %d equal cases" % (len(everybody), len(equal)))
    assert 3 * len(everybody) >= 2 * len(equal), (len(everybody), len(equal))
    for name in nec.NO_COMMIT:
        ref = oracle_run(oracle, nec.by_name(name))
        assert ref["commit_counts"].max() == 0, name
        c = ref["counters"]
        assert c["events"][3] > 0 and c["rng_draws"] > 0 and c["events_scheduled"] > 0, (name, c)
    nobody = {c["name"] for c in equal if oracle_run(oracle, c)["commit_counts"].max() == 0}
    assert nobody == set(nec.NO_COMMIT), nobody ^ set(nec.NO_COMMIT)


# ---- the sizing gap of a node that is a quorum by itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quorum_holder_4_nodes", "quorum_holder_7_nodes_quirks1"])
def test_the_quorum_holder_gap_remains(oracle, name):
    """The automatic block capacity (max_clock / 10 + 64) does not hold the rounds of a node whose right alone is a quorum: the host build
    raises F_BLOCK_OVERFLOW and nothing else; the same run with block_capacity 2048 equals the oracle."""
    auto, explicit = nec.by_name(name + "_automatic"), nec.by_name(name + "_explicit")
    assert auto["cfg"] == explicit["cfg"] and auto["seeds"] == explicit["seeds"] and auto["max_clock"] == explicit["max_clock"]
    bcap = nec.host_caps(auto)["bcap"]
    assert bcap == auto["max_clock"] // 10 + 64
    ref = oracle_run(oracle, explicit)
    assert (ref["commit_counts"].max(axis=1) > bcap).all(), ref["commit_counts"].max(axis=1)  # more committed entries than automatic blocks
    got = oracle.hostmodel_run_batch(nec.oracle_config(oracle, auto), seeds_of(auto), auto["max_clock"], history_cap=nec.HISTORY_CAP, **nec.host_caps(auto))
    assert (got["faults"] == nec.F_BLOCK_OVERFLOW).all(), got["faults"]


# ---- parameter-set batches ---------------------------------------------------------------------------------------------------------------------
def param_set_structs(case):
    from librabft_simulator_amd import simulator
    import librabft_simulator_amd as m
    base = simulator.make_config(case["n"], m.RandomDelay.new(10.0, 4.0), m.NodeConfig(),
                                 **{k: v for k, v in case["base"].items() if k != "block_capacity"}, block_capacity=case["base"].get("block_capacity", 0))
    return base, [ps.to_struct() for ps in nec.param_sets(m, case)]


@pytest.mark.parametrize("case", nec.PARAM_SET_CASES, ids=lambda c: c["name"])
def test_network_param_set_batch_host_model(oracle, harness, case):
    """Each set of a batch gives what the oracle gives for it alone: the ends of the loss and partition words in one lane change nothing
    in the next, and the ordinary set 0 is the plain loss-free run."""
    base, sets = param_set_structs(case)
    set_of, seeds = nec.set_layout(case)
    set_of, seeds = np.array(set_of, dtype=np.uint32), np.array(seeds, dtype=np.uint64)
    cls, got = psh.run_host(harness, base, sets, set_of, seeds, case["max_clock"], nec.HISTORY_CAP)
    assert cls == case["kernel_class"], cls
    assert (got["faults"] == 0).all(), got["faults"]
    for k in range(len(sets)):
        idx = np.nonzero(set_of == k)[0]
        sub = nec.set_as_case(case, k)
        ref = oracle.run_batch(nec.oracle_config(oracle, sub), seeds[idx], case["max_clock"], history_cap=nec.HISTORY_CAP)
        for key in nec.COMPARED:
            assert (got[key][idx] == ref[key]).all(), (sub["name"], key)
    assert "drop_per_million" not in case["sets"][0] and "partition" not in case["sets"][0]


# ---- refused: decided before the first HIP call ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nec.REFUSED, ids=lambda c: c["name"])
def test_refused_network_configuration_needs_no_gpu(case):
    from librabft_simulator_amd import _lib, build
    build.build()
    cfg = nec.refused_config(case)
    seeds = np.array([1, 2], dtype=np.uint64)
    h = ctypes.c_void_p()
    assert _lib.lib().lbft_batch_create(ctypes.byref(cfg), seeds.ctypes.data, len(seeds), 0, ctypes.byref(h)) == case["code"]
    assert not h.value


@pytest.mark.parametrize("case", nec.REFUSED_PARAM_SETS, ids=lambda c: c["name"])
def test_refused_param_set_arguments_need_no_gpu(case):
    from librabft_simulator_amd import _lib, build
    build.build()
    cfg = nec.refused_config(dict(n=case["n"], cfg={}))
    one = _lib.LbftParamSet()
    for key, v in nec.ORDINARY.items():
        setattr(one, key, v)
    sets = (_lib.LbftParamSet * max(case["n_sets"], 1))(*([one] * max(case["n_sets"], 1)))
    set_of = np.array(case["set_of"], dtype=np.uint32)
    seeds = np.arange(1, len(set_of) + 1, dtype=np.uint64)
    h = ctypes.c_void_p()
    rc = _lib.lib().lbft_batch_create_param_sets(ctypes.byref(cfg), sets, case["n_sets"], set_of.ctypes.data, seeds.ctypes.data, len(seeds), 0, ctypes.byref(h))
    assert rc == case["code"] and not h.value, rc


# ---- the fenced stand-alone program, plain and under the sanitizers -----------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitizers"])
def program(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("net_" + request.param)
    if request.param == "sanitizers":
        probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input="int main(){}",
                               capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip("the sanitizer runtimes are not installed")
    return qx.compile_program(str(tmp / "queue_exhaustion_host"), request.param == "sanitizers")


def fenced_case(oracle, case):
    """The case as a line of the program: the configuration in oracle_ctypes.make_config's spelling, the planner's capacities."""
    kw = dict(case["cfg"], num_nodes=case["n"])
    p = oracle.plan(nec.oracle_config(oracle, case), len(case["seeds"]), case["max_clock"], block_capacity=case.get("block_capacity", 0))
    caps = {k: p[k] for k in ("qcap", "scap", "bcap", "lcap", "ql", "qheap", "qcal", "ring", "ring_topup", "tw")}
    return kw, case["max_clock"], caps, tuple(case["seeds"]), nec.HISTORY_CAP


def test_every_case_inside_the_fence(program, oracle):
    """One run of the program over the whole table: exit status 0 (under the sanitizers: no report), no load or store outside an
    instance's rows, and the results the oracle gives -- or, for the quorum holders at the automatic capacity, exactly F_BLOCK_OVERFLOW."""
    lines = [fenced_case(oracle, c) for c in ACCEPTED]
    status, out, err = qx.run_program(program, lines)
    assert status == 0 and len(out) == len(lines), ("exit status %d after %d of %d cases" % (status, len(out), len(lines)), err)
    for case, d in zip(ACCEPTED, out):
        kind, arg = nec.expected(case)
        assert d["rc"] >= 0, (case["name"], d["rc"])
        assert not d["violations"].any(), (case["name"], "the fence", [(i, v) for i, v in enumerate(d["first_violation"]) if v])
        if kind == "fault":
            assert (d["faults"] == arg).all(), (case["name"], d["faults"])
            continue
        assert (d["faults"] == 0).all(), (case["name"], d["faults"])
        ref = oracle_run(oracle, case)
        for key in qx.RESULT_KEYS:
            assert (d[key] == ref[key]).all(), (case["name"], key)


def test_lines_without_rights_keep_their_meaning(oracle):
    """The protocol's tail is optional: a case without voting rights and rotation gives the line it gave before the tail existed, and one
    with them appends rights_rotation and a right per node."""
    kw, max_clock, caps = qx.REGRESSION["n20_u0_250"]
    line = qx.case_line(kw, max_clock, caps, qx.REGRESSION_SEEDS, 64)
    assert len(line.split()) == len(qx.CONFIG_FIELDS) + 1 + len(qx.CAPS_FIELDS) + 2 + len(qx.REGRESSION_SEEDS)
    tail = qx.case_line(dict(kw, voting_rights=[2] * 20, rights_rotation=3), max_clock, caps, qx.REGRESSION_SEEDS, 64)
    assert tail == line + " 3" + " 2" * 20
