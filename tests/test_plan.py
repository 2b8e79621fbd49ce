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


# ---- The planner under the tuning switches of the environment (oracle_ctypes.SWITCHES; lbft_hip.hip knobs_from_env reads them when a run is
# prepared, here they are arguments: oracle_ctypes.plan(knobs=...)).  One row per rule of pick_run_kernel and of the ring and window blocks of
# csrc/lbft_plan.h; the expected values are the rules' statements (their comments), not planner output.
import switch_batches as sb  # noqa: E402

NO_QUAD, NO_POPC, NO_UNI, NO_LEAN, LEAN2_OFF, both = sb.NO_QUAD, sb.NO_POPC, sb.NO_UNI, sb.NO_LEAN, sb.LEAN2_OFF, sb.both
EVERY_KERNEL_SWITCH = both(NO_QUAD, NO_POPC, NO_UNI, NO_LEAN, LEAN2_OFF)
C1_ARRAY, C1_CAL, C2_CAL, C2_HEAP = 1, 1 | sb.HEAP | sb.CALENDAR, 2 | sb.HEAP | sb.CALENDAR, 2 | sb.HEAP  # class | queue discipline

# (batch of switch_batches.BATCHES, networks, lanes_per_wavefront (0 = auto), switches, kernel, class | heap | calendar bits)
# Which line of pick_run_kernel a row reaches -- [T] commit_times, [P] param_sets, [L2] sim_lean && !no_lean && lean2, [L1] sim_lean1 &&
# !no_lean, [M] class 1, [G] class 2, [Q] the headline kernel's line with each of its five conditions failing once ([Q-quad] not the
# headline network, [Q-tiny], [Q-64] more than 32 lanes, [Q-no] no_quad), [S] the popc line (0u / 0s; failing by [S-lpw] lanes, [S-no]
# no_popc), [0] the last line:
KERNEL_ROWS = [
    ("headline", 130, 2, {}, "run0q", 0),                                  # [Q] taken
    ("headline", 130, 2, NO_POPC, "run0q", 0),                             # [Q] does not read no_popc ...
    ("headline", 130, 2, NO_UNI, "run0q", 0),                              # ... nor no_uni
    ("headline", 130, 2, NO_QUAD, "run0s", 0),                             # [Q-no] -> [S], more than one lane
    ("headline", 130, 2, both(NO_QUAD, NO_POPC), "run0", 0),               # [Q-no], [S-no] -> [0]
    ("headline", 1100, 1, {}, "run0q", 0),                                 # [Q] one lane but not tiny (>= 1 024 networks)
    ("headline", 1100, 1, NO_QUAD, "run0u", 0),                            # [Q-no] -> [S] one lane
    ("headline", 1100, 1, both(NO_QUAD, NO_UNI), "run0s", 0),              # [Q-no] -> [S] one lane, no_uni
    ("headline", 256, 0, {}, "run0u", 0),                                  # [Q-tiny] (auto lanes: one) -> [S]
    ("headline", 256, 0, NO_UNI, "run0s", 0),                              # [Q-tiny] -> [S] no_uni: NOT back to lbft_k_run0q (the rule that was once wrong)
    ("headline", 256, 0, both(NO_UNI, NO_POPC), "run0", 0),                # [Q-tiny], [S-no] -> [0]
    ("headline", 4096, 64, {}, "run0", 0),                                 # [Q-64], [S-lpw] -> [0]
    ("headline", 1100, 8, NO_QUAD, "run0s", 0),                            # [S] at LBFT_POPC_MAX_LPW = 8 lanes
    ("headline", 1100, 16, NO_QUAD, "run0", 0),                            # [S-lpw] past it
    ("c0_n7", 70, 1, {}, "run0u", 0),                                      # [Q-quad] -> [S] one lane
    ("c0_n7", 70, 1, NO_QUAD, "run0u", 0),                                 # (no_quad changes nothing off the headline network)
    ("c0_n7", 70, 1, NO_UNI, "run0s", 0),
    ("c0_n7", 70, 1, NO_POPC, "run0", 0),
    ("c0_n7", 70, 8, {}, "run0s", 0),
    ("c0_n7", 70, 8, NO_UNI, "run0s", 0),
    ("c0_n7", 70, 8, NO_POPC, "run0", 0),
    ("c0_n7", 70, 16, {}, "run0", 0),                                      # [S-lpw]
    ("c0_n7", 70, 16, NO_UNI, "run0", 0),
    ("c0_n7", 70, 16, NO_POPC, "run0", 0),
    ("c1_n4_equiv", 70, 0, {}, "run1l", C1_ARRAY),                         # [L1]
    ("c1_n4_equiv", 70, 0, LEAN2_OFF, "run1l", C1_ARRAY),                  # [L1] does not read lean2
    ("c1_n4_equiv", 70, 0, NO_LEAN, "run1", C1_ARRAY),                     # [M]
    ("c1_n20", 3, 0, {}, "run1l", C1_CAL),
    ("c1_n20", 3, 0, NO_LEAN, "run1", C1_CAL),
    ("c2_n40", 3, 0, {}, "run2l", C2_CAL | sb.RING),                       # [L2] without the record exchange
    ("c2_n40", 3, 0, NO_LEAN, "run2", C2_CAL | sb.RING),                   # [G] by no_lean
    ("c2_n40", 3, 0, LEAN2_OFF, "run2", C2_CAL | sb.RING),                 # [G] by lean2
    ("c2_n40_q1", 3, 0, {}, "run2q", C2_CAL | sb.RING),                    # [L2] with it
    ("c2_n40_q1", 3, 0, NO_LEAN, "run2", C2_CAL | sb.RING),
    ("c2_n40_q1", 3, 0, LEAN2_OFF, "run2", C2_CAL | sb.RING),
    ("c2_n40_lossy", 3, 0, {}, "run2", C2_CAL | sb.RING),                  # [G] not sim_lean, whatever the switches say
    ("c2_n40_lossy", 3, 0, EVERY_KERNEL_SWITCH, "run2", C2_CAL | sb.RING),
    ("c2_n40_heap", 3, 0, {}, "run2l", C2_HEAP),                           # [L2] on the heap
]
# the lane-private twins of the side libraries, [P] / [T]: class 0 -> ...0, class 1 -> ...1, whatever the switches say
TWIN_ROWS = [(batch, sets, timed, kernel, word) for batch, word, kernels in (
    ("headline", 0, ("ps_run0", "ct_run0", "ct_ps_run0")), ("c1_n4_equiv", C1_ARRAY, ("ps_run1", "ct_run1", "ct_ps_run1")))
    for (sets, timed), kernel in zip(((2, False), (0, True), (2, True)), kernels)]


@pytest.mark.parametrize("batch,m,lanes,switches,kernel,word", KERNEL_ROWS,
                         ids=["%s-%dx-lpw%d-%s->%s" % (r[0], r[1], r[2], "+".join(k[5:] + v for k, v in sorted(r[3].items())) or "default", r[4]) for r in KERNEL_ROWS])
def test_run_kernel_under_the_switches(oracle, batch, m, lanes, switches, kernel, word):
    got = sb.planned(oracle, batch, m, switches, lanes)
    assert sb.RUN_KERNELS[got["kernel"]] == kernel, (sb.RUN_KERNELS[got["kernel"]], got)
    ring = 512 if word & sb.RING else 0  # (the default ring and top-up of a large network on the calendar: 16 draws per step up to 64 nodes)
    assert (got["ring"], got["ring_topup"]) == (ring, 16 if ring else 0)
    assert got["blw"] == (32 if kernel == "run2q" else 0)  # the window is lbft_k_run2q's alone
    assert got["layout"][7] == word | sb.KERNEL_FLAGS[kernel], hex(got["layout"][7])
    assert lanes == 0 or got["lpw"] == lanes
    # two wavefronts per SIMD = 8-wavefront workgroups for every kernel but the full-register lbft_k_run<1> / <2>
    assert got["run_waves"] == (4 if kernel in ("run1", "run2") else 8)


@pytest.mark.parametrize("switches", [{}, EVERY_KERNEL_SWITCH, dict(LBFT_RING="128", LBFT_RING_TOPUP="4", LBFT_BLK_WINDOW="64")], ids=["default", "kernel-switches", "ring-window"])
@pytest.mark.parametrize("batch,sets,timed,kernel,word", TWIN_ROWS, ids=[r[3] for r in TWIN_ROWS])
def test_twin_kernels_whatever_the_switches_say(oracle, batch, sets, timed, kernel, word, switches):
    got = sb.planned(oracle, batch, 96, switches, param_sets=sets, commit_times=timed)
    assert sb.RUN_KERNELS[got["kernel"]] == kernel
    assert got["layout"][7] == word | sb.KERNEL_FLAGS[kernel], hex(got["layout"][7])
    assert (got["ring"], got["ring_topup"], got["blw"]) == (0, 0, 0)
    assert got["run_waves"] == (8 if kernel.endswith("0") else 4)  # lbft_k_run0's geometry / lbft_k_run<1>'s


# (batch, switches, ring, ring_topup).  The ring block of plan_capacities, line by line: [n] n > 32 && calendar, [d] the defaults 512 and
# 16 (up to 64 nodes) / 128, [r] ring_set, [t] ring_topup_set, [p] not a power of two -> 512, [m] below 128 -> 128, [z] no ring -> top-up 0.
RING_ROWS = [
    ("c2_n40", {}, 512, 16),                                               # [d]
    ("c2_n100", {}, 512, 128),                                             # [d] more than 64 nodes
    ("c2_n40", dict(LBFT_RING="100"), 512, 16),                            # [r] [p]
    ("c2_n40", dict(LBFT_RING="64"), 128, 16),                             # [r] [m]
    ("c2_n40", dict(LBFT_RING="1"), 128, 16),                              # [m] (1 is a power of two)
    ("c2_n40", dict(LBFT_RING="128"), 128, 16),
    ("c2_n40", dict(LBFT_RING="256"), 256, 16),
    ("c2_n40", dict(LBFT_RING="1024"), 1024, 16),                          # stays
    ("c2_n40", dict(LBFT_RING="0"), 0, 0),                                 # [z] no ring: lane-per-network execution
    ("c2_n40", dict(LBFT_RING="0", LBFT_RING_TOPUP="16"), 0, 0),           # [z] whatever the top-up says
    ("c2_n40", dict(LBFT_RING_TOPUP="0"), 512, 0),                         # [t] only on demand
    ("c2_n40", dict(LBFT_RING_TOPUP="4"), 512, 4),
    ("c2_n100", dict(LBFT_RING_TOPUP="16"), 512, 16),
    ("c2_n40", dict(LBFT_RING="128", LBFT_RING_TOPUP="2048"), 128, 2048),  # a top-up larger than the ring is kept (the kernel fills the room there is)
    ("c2_n40_q1", dict(LBFT_RING="256", LBFT_RING_TOPUP="4"), 256, 4),
    ("c2_n40_lossy", dict(LBFT_RING="256"), 256, 16),                      # (the ring is the calendar's, not the lean kernels')
    ("c2_n40_heap", {}, 0, 0),                                             # [n] on the heap: no ring ...
    ("c2_n40_heap", dict(LBFT_RING="256", LBFT_RING_TOPUP="4"), 0, 0),     # ... whatever LBFT_RING says
    ("c1_n20", dict(LBFT_RING="256", LBFT_RING_TOPUP="4"), 0, 0),          # [n] the calendar, but not a large network
    ("headline", dict(LBFT_RING="256", LBFT_RING_TOPUP="4"), 0, 0),
]


@pytest.mark.parametrize("batch,switches,ring,topup", RING_ROWS, ids=["%s-%s" % (r[0], "+".join(k[5:] + v for k, v in sorted(r[1].items())) or "default") for r in RING_ROWS])
def test_ring_under_the_switches(oracle, batch, switches, ring, topup):
    got, default = sb.planned(oracle, batch, 3, switches), sb.planned(oracle, batch, 3)
    assert (got["ring"], got["ring_topup"]) == (ring, topup)
    assert got["layout"][7] == (default["layout"][7] & ~sb.RING) | (sb.RING if ring else 0), hex(got["layout"][7])  # bit 11 and nothing else
    assert got["kernel"] == default["kernel"] and got["blw"] == default["blw"]
    # the ring is two rows of `ring` words per instance, and the only thing of the layout that LBFT_RING changes
    assert got["layout"][4] - default["layout"][4] == 4 * 2 * (ring - default["ring"])


def test_calendar_off_means_no_ring(oracle):
    got = sb.planned(oracle, "c2_n40", 3, dict(LBFT_RING="256"), calendar_queue=False)
    assert (got["ring"], got["ring_topup"], got["layout"][7]) == (0, 0, C2_HEAP | sb.KERNEL_FLAGS["run2l"])


# (batch, lanes, switches, blw).  The window block of plan_launch: [k] lbft_k_run2q only, [2] rounded down to a power of two, [c] at most
# 256, [f] halved until the kernel's LDS stays within 150 KiB, [0] off.  One entry is a tag and the ten words of a hot block record (44
# bytes) per network of the workgroup's eight wavefronts; beside the window the workgroup holds the tables (8 720 bytes), the phase words
# (8 x 32 x 8 + 8) and a 128-byte receiver list per network -- at 32 lanes 43 544 bytes + 11 264 per entry: 8 entries fit 150 KiB (133 656),
# 16 do not; at one lane 11 800 + 352 per entry: all 256 fit.  ([c] is reached by the rows that ask for 1 000, but no row can tell it from
# [f]: 512 entries are 180 224 bytes at one lane, more than 150 KiB on their own.)
WINDOW_ROWS = [
    ("c2_n40_q1", 1, {}, 32),                                              # the default
    ("c2_n40_q1", 1, dict(LBFT_BLK_WINDOW="32"), 32),
    ("c2_n40_q1", 1, dict(LBFT_BLK_WINDOW="48"), 32),                      # [2]
    ("c2_n40_q1", 1, dict(LBFT_BLK_WINDOW="8"), 8),
    ("c2_n40_q1", 1, dict(LBFT_BLK_WINDOW="256"), 256),
    ("c2_n40_q1", 1, dict(LBFT_BLK_WINDOW="1000"), 256),                   # [2] 512, [c] 256, which fits at one lane
    ("c2_n40_q1", 32, dict(LBFT_BLK_WINDOW="1000"), 8),                    # [c] [f] 256 -> 8 at 32 lanes
    ("c2_n40_q1", 32, dict(LBFT_BLK_WINDOW="256"), 8),                     # [f]
    ("c2_n40_q1", 32, {}, 8),                                              # [f] the default as well
    ("c2_n40_q1", 32, dict(LBFT_BLK_WINDOW="8"), 8),
    ("c2_n40_q1", 16, dict(LBFT_BLK_WINDOW="256"), 16),                    # [f] 8 720 + 2 056 + 16 384 + 5 632 per entry: 16 fit (117 272), 32 do not
    ("c2_n40_q1", 1, dict(LBFT_BLK_WINDOW="0"), 0),                        # [0]
    ("c2_n40_q1", 32, dict(LBFT_BLK_WINDOW="0"), 0),
    ("c2_n100_q1", 1, dict(LBFT_BLK_WINDOW="64"), 64),
    ("c2_n40_q1", 1, both(NO_LEAN, dict(LBFT_BLK_WINDOW="64")), 0),        # [k] lbft_k_run<2>
    ("c2_n40", 1, dict(LBFT_BLK_WINDOW="64"), 0),                          # [k] lbft_k_run2l
    ("c1_n20", 1, dict(LBFT_BLK_WINDOW="64"), 0),
    ("headline", 2, dict(LBFT_BLK_WINDOW="64"), 0),
]


@pytest.mark.parametrize("batch,lanes,switches,blw", WINDOW_ROWS, ids=["%s-lpw%d-%s" % (r[0], r[1], "+".join(k[5:] + v for k, v in sorted(r[2].items())) or "default") for r in WINDOW_ROWS])
def test_block_window_under_the_switches(oracle, batch, lanes, switches, blw):
    got = sb.planned(oracle, batch, 3, switches, lanes)
    off = sb.planned(oracle, batch, 3, both(switches, dict(LBFT_BLK_WINDOW="0")), lanes)
    assert got["blw"] == blw and off["blw"] == 0
    assert got["lds_bytes"] == off["lds_bytes"] + 8 * lanes * blw * 44 and got["lds_bytes"] <= 150 * 1024
    # nothing but the LDS bytes follows from the window: the kernel, the flag word and the state rows are the same
    assert {k: v for k, v in got.items() if k not in ("blw", "lds_bytes")} == {k: v for k, v in off.items() if k not in ("blw", "lds_bytes")}


def test_default_knobs_are_the_unset_environment(oracle):
    """plan() without knobs, with an empty dict and with every variable unset give the same plan, for one batch of every kernel."""
    for batch, m, lanes in (("headline", 130, 2), ("headline", 256, 0), ("c0_n7", 70, 16), ("c1_n4_equiv", 70, 0), ("c2_n40", 3, 0), ("c2_n40_q1", 3, 32),
                            ("c2_n100_q1", 1, 0), ("c2_n40_lossy", 3, 0)):
        b = sb.BATCHES[batch]
        plain = oracle.plan(oracle.make_config(**b["kw"]), m, b["max_clock"], lanes_per_wavefront=lanes, **b["caps"])
        assert plain == sb.planned(oracle, batch, m, {}, lanes) == sb.planned(oracle, batch, m, None, lanes)
    with pytest.raises(KeyError):
        oracle.knobs_of_switches(dict(LBFT_NO_SUCH="1"))
    with pytest.raises(KeyError):
        oracle.plan(oracle.make_config(num_nodes=4), 4, 100, knobs=dict(ring_set=1))
    # "0" leaves a NO_ switch off, as atoi does in the library
    assert sb.planned(oracle, "headline", 130, dict(LBFT_NO_QUAD="0"), 2)["kernel"] == sb.RK["run0q"]
    assert sb.planned(oracle, "c2_n40", 3, dict(LBFT_LEAN2="1"))["kernel"] == sb.RK["run2l"]


def test_the_class2_device_rows_cover_every_switch_value(oracle):
    """What the planner makes of the class-2 rows of tests/test_kernel_switches_gpu.py, per kernel: every ring of the grid, every top-up of
    the grid IN EFFECT (on a row with a ring: without one the planner drops it), one of them larger than its ring, lane-per-network
    execution on the 40- and on the 100-node network, and every window setting."""
    import test_kernel_switches_gpu as device_rows  # (the module needs the GPU only to run its tests)
    assert len(device_rows.CLASS2_ROWS) <= 24
    for kernel in ("run2l", "run2q", "run2"):
        plans = [(r, sb.planned(oracle, r[0], r[1], r[3], r[2])) for r in device_rows.CLASS2_ROWS if r[4] == kernel]
        assert {p["ring"] for _, p in plans} >= {0, 128, 256, 1024}, kernel
        assert {p["ring_topup"] for _, p in plans if p["ring"]} >= {0, 4, 16, 2048}, kernel
        assert all(p["ring_topup"] == 0 for _, p in plans if not p["ring"])
        assert any(p["ring_topup"] > p["ring"] > 0 for _, p in plans), kernel
        assert {r[3].get("LBFT_BLK_WINDOW") for r, _ in plans} >= {"0", "8", "256"}, kernel
    no_ring = {sb.BATCHES[r[0]]["kw"]["num_nodes"] for r in device_rows.CLASS2_ROWS if sb.planned(oracle, r[0], r[1], r[3], r[2])["ring"] == 0}
    assert no_ring == {40, 100}
    q = [(r[2], sb.planned(oracle, r[0], r[1], r[3], r[2])["blw"]) for r in device_rows.CLASS2_ROWS if r[4] == "run2q" and "LBFT_BLK_WINDOW" in r[3]]
    assert {lanes for lanes, _ in q} >= {1, 32} and {blw for _, blw in q} >= {0, 8, 256}
