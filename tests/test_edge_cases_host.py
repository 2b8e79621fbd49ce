"""CPU tier of the edge-case table (tests/edge_cases.py): the host build of the kernel logic (oracle/host_model.cpp, lbft_core.h compiled with
g++) against the oracle on every case, with the capacities and queue discipline lbft_batch_run_until would choose; the parameter-set batches
through the host build of the parameter-set classes (tests/param_sets_host_model.cpp); the refused cases through the C ABI's argument
checks, which run before any HIP call.  The device tier is tests/test_edge_cases_gpu.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edge_cases as ec  # noqa: E402
import test_param_sets_host_model as psh  # noqa: E402  (run_host: the host build of the parameter-set classes)
from test_param_sets_host_model import harness  # noqa: E402,F401  (the fixture that compiles it)


def run_host(oracle, case, **over):
    caps = ec.host_caps(case)
    caps.update(over)
    seeds = np.array(case["seeds"], dtype=np.uint64)
    return oracle.hostmodel_run_batch(ec.oracle_config(oracle, case), seeds, case["max_clock"], threads=8, history_cap=ec.HISTORY_CAP, **caps)


def assert_equal_to_oracle(oracle, case, got):
    ref = oracle.run_batch(ec.oracle_config(oracle, case), np.array(case["seeds"], dtype=np.uint64), case["max_clock"], threads=8,
                           history_cap=ec.HISTORY_CAP)
    assert (got["faults"] == 0).all(), (case["name"], got["faults"])
    for key in ec.COMPARED:
        assert (got[key] == ref[key]).all(), (case["name"], key)
    for key in ec.COMPARED_COUNTERS:
        assert got["counters"][key] == ref["counters"][key], (case["name"], key, got["counters"][key], ref["counters"][key])
    return ref


@pytest.mark.parametrize("case", [c for c in ec.CASES if ec.expected(c)[0] != "refused"], ids=lambda c: c["name"])
def test_edge_case_host_model(oracle, case):
    kind, arg = ec.expected(case)
    got = run_host(oracle, case)
    if kind == "equal":
        ref = assert_equal_to_oracle(oracle, case, got)
        if case["name"] == "max_clock_largest_accepted":  # the network does run to the top of the clock range
            assert ref["histories"]["time"].max() > 2 ** 30 and ref["commit_counts"].min() >= 20
    else:
        assert (got["faults"] == arg).all(), (case["name"], got["faults"], arg)
    if "calendar" in case:
        assert ec.host_caps(case)["qcal"] == int(case["calendar"]), case["name"]
    if "kernel_class" in case:
        assert ec.expected_layout(case)[0] == case["kernel_class"], case["name"]


def test_hand_picked_seeds_keep_their_startups_representable(oracle):
    """uniform_span_2p32_startups_fit relies on its seeds' first delays: every startup time must be <= 2^30 - 1 (else the case is a fault)."""
    case = next(c for c in ec.CASES if c.get("startups_fit"))
    cfg = ec.oracle_config(oracle, case)
    for s in case["seeds"]:
        o = oracle.OracleSim(cfg, s)
        startups = o.run_until(0).startup_times()
        o.close()
        assert max(startups) <= 2 ** 30 - 1, (s, startups)


def test_calendar_limit_is_the_host_models(oracle):
    """The host build takes a calendar queue up to LBFT_CAL_MAX_CLOCK and refuses one above it (as prepare_run falls back to the heap)."""
    last, past = ec.by_name("calendar_last_horizon"), ec.by_name("calendar_first_horizon_past")
    heap = run_host(oracle, last, qcal=0, ql=16)
    cal = run_host(oracle, last, qcal=1, ql=0)
    for key in ec.COMPARED:
        assert (heap[key] == cal[key]).all(), key
    with pytest.raises(RuntimeError, match="-11"):
        run_host(oracle, past, qcal=1, ql=0)


def test_max_clock_contract_is_one_number(oracle):
    """include/lbft.h's LBFT_MAX_CLOCK is what the table, the header's prose and prepare_run use, and the host build refuses past it.
    (The binding pin is the device tier's test_refused_on_the_device: the C ABI reaches prepare_run's check only through a batch, which
    needs a GPU.  The source checks here only catch the header and the code drifting apart on a CPU-only machine.)"""
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    assert int(re.search(r"#define LBFT_MAX_CLOCK (0x[0-9a-f]+)", header).group(1), 16) == ec.MAX_CLOCK_LIMIT == 2 ** 31 - 3
    assert re.search(r"0\s*<=\s*max_clock\s*<=\s*LBFT_MAX_CLOCK", header)
    src = open(os.path.join(ROOT, "librabft_simulator_amd", "csrc", "lbft_hip.hip")).read()
    assert re.search(r"max_clock\s*<\s*0\s*\|\|\s*max_clock\s*>\s*LBFT_MAX_CLOCK\s*\)", src)
    for name in ("max_clock_one_above", "max_clock_2p31_minus_1", "max_clock_negative"):
        with pytest.raises(RuntimeError, match="-14"):
            run_host(oracle, ec.by_name(name))


@pytest.mark.parametrize("case", [c for c in ec.CASES if ec.expected(c)[0] == "refused" and not c["name"].startswith("max_clock")],
                         ids=lambda c: c["name"])
def test_refused_configuration_needs_no_gpu(case):
    from librabft_simulator_amd import _lib, build
    build.build()
    _, code = ec.expected(case)
    cfg = ec.lbft_config(case)
    seeds = np.array(case["seeds"], dtype=np.uint64)
    h = ctypes.c_void_p()
    assert _lib.lib().lbft_batch_create(ctypes.byref(cfg), seeds.ctypes.data, len(seeds), 0, ctypes.byref(h)) == code
    assert not h.value


@pytest.mark.parametrize("case", ec.PARAM_SET_CASES, ids=lambda c: c["name"])
def test_param_set_edge_batch_host_model(oracle, harness, case):
    """Each set of a batch gives what its own plain run gives: the extreme sets neither fault nor change their ordinary neighbours."""
    from librabft_simulator_amd import _lib
    base = _lib.LbftConfig()
    base.num_nodes, base.delay_model, base.commands_per_epoch = case["n"], case["delay_model"], 30000
    sets = []
    for k in range(len(case["sets"])):
        s = _lib.LbftParamSet()
        for key, v in ec.set_fields(case, k).items():
            setattr(s, key, v)
        sets.append(s)
    set_of, seeds = ec.set_layout(case)
    set_of, seeds = np.array(set_of, dtype=np.uint32), np.array(seeds, dtype=np.uint64)
    cls, got = psh.run_host(harness, base, sets, set_of, seeds, case["max_clock"], ec.HISTORY_CAP)
    assert cls == case["kernel_class"], cls
    for k in range(len(sets)):
        idx = np.nonzero(set_of == k)[0]
        kind, arg = ec.expected(ec.set_as_case(case, k))
        if kind == "fault":
            assert (got["faults"][idx] == arg).all(), (k, got["faults"][idx])
            continue
        assert (got["faults"][idx] == 0).all(), (k, got["faults"][idx])
        ref = oracle.run_batch(ec.oracle_config(oracle, ec.set_as_case(case, k)), seeds[idx], case["max_clock"], history_cap=ec.HISTORY_CAP)
        for key in ec.COMPARED:
            assert (got[key][idx] == ref[key]).all(), (k, key)
