"""The planner (csrc/lbft_plan.h) where the CPU tier can see it, through the host model's exported planner call (oracle_ctypes.plan: the
code the device library runs).  It reproduces what the device library reported on the MI355X for every recorded batch
(tests/golden/plan_layouts.json, tests/plan_batches.py: the eight words of lbft_batch_layout and lbft_batch_device_bytes), and for every
accepted edge case its class / heap / calendar / cooperative flags equal the edge-case table's own statement
(edge_cases.expected_layout)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edge_cases as ec  # noqa: E402
import plan_batches as pb  # noqa: E402


@pytest.mark.parametrize("entry", pb.recorded(), ids=lambda e: e["name"])
def test_planner_reproduces_the_recorded_layout(oracle, entry):
    got = pb.planned(oracle, pb.BATCHES[entry["name"]], entry["free_bytes"])
    assert got["layout"] == entry["layout"], (entry["name"], got["layout"], [hex(got["layout"][7]), hex(entry["layout"][7])])
    assert got["device_bytes"] == entry["device_bytes"], entry["name"]


def test_the_fixture_covers_the_table():
    """Every batch of the table is recorded but the ones tests/golden/plan_layouts.json lists as dropped for want of free memory, and
    every family of the table keeps at least one entry."""
    with_entry = {e["name"] for e in pb.recorded()}
    assert with_entry | set(pb.dropped()) == set(pb.BATCHES) and not with_entry & set(pb.dropped())
    for family in ("c2_", "c3_", "c3shard_", "c4_", "c5_", "256x4", "forced_lpw_", "lossy_32_nodes", "param_sets_small", "param_sets_mid",
                   "commit_times_class0", "commit_times_class1", "commit_times_param_sets_small", "commit_times_param_sets_mid"):
        assert any(n.startswith(family) for n in with_entry), family
    assert {"edge_" + c["name"] for c in ec.CASES if ec.expected(c)[0] != "refused" and not c.get("host_only")} <= with_entry


@pytest.mark.parametrize("case", [c for c in ec.CASES if ec.expected(c)[0] != "refused"], ids=lambda c: c["name"])
def test_planner_flags_equal_the_tables_statement(oracle, case):
    flags = oracle.plan(ec.oracle_config(oracle, case), len(case["seeds"]), case["max_clock"], block_capacity=case.get("block_capacity", 0),
                        calendar_queue=case.get("calendar_queue", True))["layout"][7]
    assert (flags & 0xff, (flags >> 8) & 1, (flags >> 9) & 1, (flags >> 11) & 1) == ec.expected_layout(case), (case["name"], hex(flags))
