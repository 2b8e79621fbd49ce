"""Every run kernel the tuning switches of the environment can select, on the batches the switches send it, against the oracle.

The planner reads eight variables when a run is prepared (oracle_ctypes.SWITCHES; lbft_hip.hip knobs_from_env, DESIGN.md section 4
"Knobs").  Every A/B figure of EXPERIMENTS.md was measured by flipping one, on the assumption that both sides compute the same thing; by
default the suite meets each kernel only on the batches the planner gives it unasked.  Here the switches are set in this process
(monkeypatch: the library reads them at every prepare_run), the flag word the batch reports must be the one the planner of
tests/test_plan.py's tables gives for the same batch and switches -- so the kernel under test is the one that ran -- and the results are
the oracle's bit for bit, as in tests/test_fuzz_model.py: commit counts, active rounds, last committed states, histories, no fault, and the
counters events, rng_draws, rounds, commits, events_scheduled.  Then the same batch across switches: reset under another switch, a switch
flipped in the middle of a stepped run, checkpoints across the kernels whose difference the checkpoint header does not record (the
class-0 kernels, the window of block records), and the refusal of a checkpoint across kernel families or ring sizes.

The batches are tests/switch_batches.py's, the smallest at which the paths in question run: odd sizes, a partly filled last wavefront."""
import os

import numpy as np
import pytest

import switch_batches as sb
from support import amd, run_to_end  # noqa: F401
from switch_batches import LEAN2_OFF, NO_LEAN, NO_POPC, NO_QUAD, NO_UNI, both

pytestmark = pytest.mark.gpu

RESULT_COUNTERS = ("events", "rng_draws", "rounds", "commits", "events_scheduled")
HISTORY_CAP = 96
INVALID = -1  # LBFT_ERR_INVALID


def seeds_of(m):
    return np.arange(1, m + 1, dtype=np.uint64) * 104729 + 17


_REFERENCES = {}


def reference(oracle, batch, m):
    """The oracle's run of ``m`` networks of a batch: computed once, shared by every row of the batch, read-only."""
    if (batch, m) not in _REFERENCES:
        b = sb.BATCHES[batch]
        ref = oracle.run_batch(oracle.make_config(math_mode=1, **b["kw"]), seeds_of(m), b["max_clock"], threads=8, history_cap=HISTORY_CAP)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFERENCES[(batch, m)] = ref
    return _REFERENCES[(batch, m)]


def set_switches(monkeypatch, oracle, switches):
    """Exactly ``switches`` of the eight variables in this process's environment (restored by monkeypatch when the test ends)."""
    for name in oracle.SWITCHES:
        if name in switches:
            monkeypatch.setenv(name, str(switches[name]))
        else:
            monkeypatch.delenv(name, raising=False)


def assert_equal_to_ref(res, ref):
    assert not res.faults.any(), sorted(set(int(f) for f in res.faults))
    assert (res.commit_counts == ref["commit_counts"]).all()
    assert (res.active_rounds == ref["active_rounds"]).all()
    assert (res.last_committed_states == ref["last_states"]).all()
    assert (res.committed_histories(HISTORY_CAP) == ref["histories"]).all()
    for key in RESULT_COUNTERS:
        assert res.counters[key] == ref["counters"][key], key


LAYOUT_WORDS = ("node_bytes", "event_bytes", "snapshot_bytes", "block_bytes", "instance_bytes", "lds_queue_slots", "lanes_per_wavefront", "kernel_class")


def assert_ran_on(oracle, sim, batch, m, lanes, switches, kernel=None):
    """The eight words of lbft_batch_layout are the planner's for this batch under these switches (and the flag word names ``kernel``):
    the kernel and the lanes, and with instance_bytes the ring the device laid out -- two rows of ``ring`` words per instance
    (tests/test_plan.py test_ring_under_the_switches), where the flag word's bit 11 only tells a ring from none.  The top-up and the
    window's size leave no trace in these words: for them the row rests on the planner's tables and on the environment being read at all
    (the refusals below)."""
    plan = sb.planned(oracle, batch, m, switches, lanes)
    lay = sim.layout()
    assert lay["kernel_class"] == plan["layout"][7], (hex(lay["kernel_class"]), hex(plan["layout"][7]))
    assert lay["lanes_per_wavefront"] == plan["lpw"]
    assert lay["instance_bytes"] == plan["layout"][4]
    assert [lay[k] for k in LAYOUT_WORDS] == plan["layout"]
    if kernel is not None:
        assert sb.RUN_KERNELS[plan["kernel"]] == kernel, sb.RUN_KERNELS[plan["kernel"]]
    return plan


def run_under(amd, oracle, monkeypatch, batch, m, lanes, switches, kernel=None, sim=None, **sim_kw):
    """A run to the end under ``switches`` (of a fresh batch, or of ``sim`` after a reset), checked against the oracle -> the batch, its result."""
    set_switches(monkeypatch, oracle, switches)
    if sim is None:
        sim = sb.make_sim(amd, batch, seeds_of(m), lanes, **sim_kw)
    else:
        sim.reset()
    res = sim.loop_until(sb.BATCHES[batch]["max_clock"], allow_faults=True)
    assert_ran_on(oracle, sim, batch, m, lanes, switches, kernel)
    assert_equal_to_ref(res, reference(oracle, batch, m))
    return sim, res


# steps per launch of the stepped runs: two launches before a flip or a checkpoint, then launches of `resume` steps to the end (the four
# nodes with two equivocators process 270 events per network in all: shorter launches)
CUTS = {"c1_n4_equiv": (40, 23)}


def cuts_of(batch, resume):
    return CUTS.get(batch, (150, 77)), (31 if batch in CUTS else resume)


def started(amd, batch, m, lanes):
    """A fresh batch, started with run_steps and not finished."""
    sim = sb.make_sim(amd, batch, seeds_of(m), lanes)
    for cut in cuts_of(batch, 0)[0]:
        left, _ = sim.run_steps(sb.BATCHES[batch]["max_clock"], cut)
        assert left > 0, "the run ended before the cut"
    return sim


def switch_id(switches):
    return "+".join("%s=%s" % (k[5:], v) for k, v in sorted(switches.items())) or "default"


def test_no_switch_is_set_when_the_module_starts():
    """(a test under a stray switch would check another kernel than it says)"""
    import oracle_ctypes
    assert [n for n in oracle_ctypes.SWITCHES if n in os.environ] == []


# ---- 1. every reachable kernel / batch pair

# (batch, networks, lanes per wavefront, switches, kernel).  131 = two networks past the 8 wavefronts x 8 (or 2) lanes of a workgroup's
# first round: a partly filled last wavefront; 1 100 at one lane: past the 1 024 below which lbft_k_run0u takes the headline network.
CLASS0_ROWS = [
    ("headline", 131, 2, {}, "run0q"),
    ("headline_cpe7", 131, 2, NO_QUAD, "run0s"),
    ("headline", 131, 2, both(NO_QUAD, NO_POPC), "run0"),
    ("headline_cpe7", 131, 8, {}, "run0q"),
    ("headline", 131, 8, NO_QUAD, "run0s"),
    ("headline_cpe7", 131, 8, both(NO_QUAD, NO_POPC), "run0"),
    ("headline", 1100, 1, {}, "run0q"),
    ("headline_cpe7", 1100, 1, NO_QUAD, "run0u"),
    ("headline", 1100, 1, both(NO_QUAD, NO_UNI), "run0s"),
    ("headline_cpe7", 1100, 1, both(NO_QUAD, NO_POPC), "run0"),
    # weighted rights, uniform delays: class 0 off the headline network
    ("c0_n7", 70, 1, {}, "run0u"),
    ("c0_n7", 70, 1, NO_UNI, "run0s"),
    ("c0_n7", 70, 1, NO_POPC, "run0"),
    ("c0_n7", 70, 8, {}, "run0s"),
    ("c0_n7", 70, 8, NO_UNI, "run0s"),
    ("c0_n7", 70, 8, NO_POPC, "run0"),
]
CLASS1_ROWS = [
    ("c1_n4_equiv", 70, 0, {}, "run1l"),
    ("c1_n4_equiv", 70, 0, NO_LEAN, "run1"),
    ("c1_n4_equiv4", 70, 0, {}, "run1l"),
    ("c1_n4_equiv4", 70, 0, NO_LEAN, "run1"),
    ("c1_n7_equiv", 70, 0, {}, "run1l"),
    ("c1_n7_equiv", 70, 0, NO_LEAN, "run1"),
    ("c1_n20", 3, 0, {}, "run1l"),
    ("c1_n20", 3, 0, NO_LEAN, "run1"),
]


def _ring(ring, topup, **more):
    return dict(dict(LBFT_RING=str(ring), LBFT_RING_TOPUP=str(topup)), **{k: str(v) for k, v in more.items()})


def _topup(topup, **more):
    return dict(dict(LBFT_RING_TOPUP=str(topup)), **{k: str(v) for k, v in more.items()})


# Class 2, 24 rows.  On each of lbft_k_run2l, lbft_k_run2q and lbft_k_run<2>: every LBFT_RING of {0, 128, 256, 1024} once, and every
# LBFT_RING_TOPUP of {0, 4, 16, 2048} (larger than every ring) on a row that HAS a ring -- without one the planner drops the top-up
# (tests/test_plan.py RING_ROWS [z]), so a LBFT_RING=0 row repeats the top-up of another row of its kernel, and the fourth top-up runs with
# the default ring of 512 entries (lbft_k_run2l, lbft_k_run<2>) or on the batch whose epochs change (lbft_k_run2q);
# tests/test_plan.py test_the_class2_device_rows_cover_every_switch_value counts what the planner makes of the rows, not what their names say.  LBFT_RING=0 runs the
# 100-node network, whose rights rotate, as well as the 40-node one.  NO_LEAN and LEAN2=0 on every base configuration, with a ring setting or
# without (c2_n40 under NO_LEAN alone is the reset chain's fourth run below).  Every LBFT_BLK_WINDOW of {0, 8, 256} at 1 and 32 lanes on
# lbft_k_run2q, whose window it sizes, and once on the two kernels that must not get one.
# (LBFT_RING=0 on a lean batch is neither refused nor routed elsewhere: tests/test_plan.py RING_ROWS -- the lean kernel, lane-per-network.)
CLASS2_ROWS = [
    ("c2_n40_q1", 3, 0, LEAN2_OFF, "run2"),
    ("c2_n100", 1, 0, LEAN2_OFF, "run2"),
    ("c2_n100_q1", 1, 0, NO_LEAN, "run2"),
    ("c2_n100", 1, 0, _ring(0, 16, LBFT_BLK_WINDOW=8), "run2l"),
    ("c2_n40", 3, 0, _ring(128, 2048), "run2l"),
    ("c2_n100", 1, 0, _ring(256, 0, LBFT_BLK_WINDOW=256), "run2l"),
    ("c2_n40", 3, 0, _ring(1024, 16, LBFT_BLK_WINDOW=0), "run2l"),
    ("c2_n40", 3, 0, _topup(4), "run2l"),
    ("c2_n40_q1", 3, 0, _ring(0, 4), "run2q"),
    ("c2_n100_q1", 1, 0, _ring(128, 2048), "run2q"),
    ("c2_n40_q1", 3, 0, _ring(256, 4), "run2q"),
    ("c2_n40_q1", 3, 0, _ring(1024, 0), "run2q"),
    ("c2_n40_q1", 3, 0, both(NO_LEAN, _ring(0, 4, LBFT_BLK_WINDOW=256)), "run2"),
    ("c2_n40", 3, 0, both(LEAN2_OFF, _ring(128, 0, LBFT_BLK_WINDOW=8)), "run2"),
    ("c2_n100", 1, 0, both(NO_LEAN, _ring(256, 16)), "run2"),
    ("c2_n40_q1", 3, 0, both(LEAN2_OFF, _ring(1024, 4, LBFT_BLK_WINDOW=0)), "run2"),
    ("c2_n40_q1", 3, 1, dict(LBFT_BLK_WINDOW="0"), "run2q"),
    ("c2_n40_q1", 3, 32, dict(LBFT_BLK_WINDOW="0"), "run2q"),
    ("c2_n40_q1", 3, 1, dict(LBFT_BLK_WINDOW="8"), "run2q"),
    ("c2_n100_q1", 1, 32, dict(LBFT_BLK_WINDOW="8"), "run2q"),
    ("c2_n100_q1", 1, 1, dict(LBFT_BLK_WINDOW="256"), "run2q"),
    ("c2_n40_q1", 3, 32, dict(LBFT_BLK_WINDOW="256"), "run2q"),  # (150 KiB of LDS at 32 lanes hold 8 entries: the planner's halving)
    # rotating rights across an epoch change
    ("c2_n40_epochs_q3", 3, 0, _ring(128, 16, LBFT_BLK_WINDOW=8), "run2q"),
    ("c2_n40_epochs_q3", 3, 0, both(NO_LEAN, _topup(2048)), "run2"),
]
assert len(CLASS2_ROWS) <= 24
ROWS = CLASS0_ROWS + CLASS1_ROWS + CLASS2_ROWS


@pytest.mark.parametrize("batch,m,lanes,switches,kernel", ROWS, ids=["%s-%dx-lpw%d-%s-%s" % (r[0], r[1], r[2], switch_id(r[3]), r[4]) for r in ROWS])
def test_kernel_under_switches_equals_the_oracle(amd, oracle, monkeypatch, batch, m, lanes, switches, kernel):
    run_under(amd, oracle, monkeypatch, batch, m, lanes, switches, kernel)[0].close()


@pytest.mark.parametrize("switches,kernel", [({}, "run0q"), (both(NO_QUAD, NO_POPC), "run0")], ids=["run0q", "run0"])
def test_headline_network_in_cut_launches(amd, oracle, monkeypatch, switches, kernel):
    """Launches of at most 173 steps: the queue's LDS front goes back to its rows and comes in again many times."""
    sim, res = run_under(amd, oracle, monkeypatch, "headline_cpe7", 131, 2, switches, kernel, max_steps_per_launch=173)
    assert res.counters["launches"] > 1
    sim.close()


def test_the_rows_reach_what_they_claim(oracle):
    """Every one of the nine run kernels has a row; the networks commit -- but the four nodes of which two equivocate, whose rounds end by
    timeout alone: the four nodes with one equivocator run the same kernels on the same queue and do commit --; epochs change where a row
    says so."""
    assert {r[4] for r in ROWS} == set(sb.RUN_KERNELS[:9])
    for batch, m in sorted({(r[0], r[1]) for r in ROWS}):
        ref = reference(oracle, batch, m)
        assert ref["active_rounds"].max() >= 4, batch  # (a node's rounds start again with its epoch)
        if batch != "c1_n4_equiv":
            assert ref["commit_counts"].max() >= 1, batch
    assert reference(oracle, "c1_n4_equiv4", 70)["commit_counts"].min() >= 1
    assert sb.planned(oracle, "c1_n4_equiv4", 70)["layout"] == sb.planned(oracle, "c1_n4_equiv", 70)["layout"]
    for batch in ("headline_cpe7", "c2_n40_epochs_q3"):
        b = sb.BATCHES[batch]
        o = oracle.OracleSim(oracle.make_config(math_mode=1, **b["kw"]), int(seeds_of(1)[0])).run_until(b["max_clock"])
        assert max(o.epochs()) >= 1, batch


# ---- 2. the same batch across switches

# (a) reset, then a run under another switch: the state rows are the previous kernel's leftovers, and a change of the ring is a relayout
# of allocated state
RESET_CHAINS = {
    "c2_n40": ("c2_n40", 3, 0, [({}, "run2l"), (dict(LBFT_RING="128"), "run2l"), (dict(LBFT_RING="0"), "run2l"), (NO_LEAN, "run2"), ({}, "run2l")]),
    "c1_n4_equiv": ("c1_n4_equiv", 70, 0, [({}, "run1l"), (NO_LEAN, "run1"), ({}, "run1l")]),
    "headline": ("headline_cpe7", 131, 2, [({}, "run0q"), (both(NO_QUAD, NO_POPC), "run0"), (NO_QUAD, "run0s"), ({}, "run0q")]),
}


@pytest.mark.parametrize("name", sorted(RESET_CHAINS))
def test_reset_then_run_under_another_switch(amd, oracle, monkeypatch, name):
    batch, m, lanes, chain = RESET_CHAINS[name]
    sim, rings = None, []
    for switches, kernel in chain:
        sim, _ = run_under(amd, oracle, monkeypatch, batch, m, lanes, switches, kernel, sim=sim)
        rings.append((sim.layout()["kernel_class"] >> 11) & 1)
    if name == "c2_n40":
        assert rings == [1, 1, 0, 1, 1]
    sim.close()


# (b) the switches are read when a run is prepared, not at every launch: one flipped in the middle of a stepped run changes nothing
@pytest.mark.parametrize("batch,m,lanes,flipped,kernel", [
    ("headline_cpe7", 131, 2, NO_QUAD, "run0q"), ("headline", 1100, 1, NO_QUAD, "run0q"), ("c1_n4_equiv", 70, 0, NO_LEAN, "run1l"),
    ("c1_n7_equiv", 70, 0, NO_LEAN, "run1l"), ("c2_n40", 3, 0, both(NO_LEAN, dict(LBFT_RING="128")), "run2l")],
    ids=["headline-lpw2", "headline-lpw1", "c1_n4_equiv", "c1_n7_equiv", "c2_n40"])
def test_switch_flipped_in_the_middle_of_a_stepped_run(amd, oracle, monkeypatch, batch, m, lanes, flipped, kernel):
    set_switches(monkeypatch, oracle, {})
    sim = started(amd, batch, m, lanes)
    set_switches(monkeypatch, oracle, flipped)
    res = run_to_end(sim, sb.BATCHES[batch]["max_clock"], cuts_of(batch, 211)[1])
    assert res.counters["launches"] >= 3
    assert_equal_to_ref(res, reference(oracle, batch, m))
    assert_ran_on(oracle, sim, batch, m, lanes, {}, kernel)  # still the kernel the run started on
    sim.close()


# (c) checkpoints across kernels whose difference the header does not record: the class-0 kernels share the state rows (the LDS front of
# the queue, the hcbr buffers lbft_k_run0q carries in registers and the others keep in LDS are written back at the end of every launch),
# and the window of block records is rebuilt empty at every launch
CHECKPOINT_ROWS = [
    ("headline_cpe7", 131, 2, {}, "run0q", NO_QUAD, "run0s"),
    ("headline", 131, 2, {}, "run0q", both(NO_QUAD, NO_POPC), "run0"),
    ("headline_cpe7", 1100, 1, {}, "run0q", NO_QUAD, "run0u"),
    ("headline", 131, 8, both(NO_QUAD, NO_POPC), "run0", {}, "run0q"),       # the reverse direction
    ("headline_cpe7", 1100, 1, NO_QUAD, "run0u", both(NO_QUAD, NO_UNI), "run0s"),
    ("c2_n40_q1", 3, 0, {}, "run2q", dict(LBFT_BLK_WINDOW="0"), "run2q"),      # saved with a window of 32 entries
    ("c2_n40_q1", 3, 0, {}, "run2q", dict(LBFT_BLK_WINDOW="256"), "run2q"),
]


@pytest.mark.parametrize("batch,m,lanes,saved,saved_on,loaded,loaded_on", CHECKPOINT_ROWS,
                         ids=["%s-%dx-lpw%d-%s-to-%s-%s" % (r[0], r[1], r[2], r[4], r[6], switch_id(r[5])) for r in CHECKPOINT_ROWS])
def test_checkpoint_resumes_on_another_kernel_of_its_family(amd, oracle, monkeypatch, tmp_path, batch, m, lanes, saved, saved_on, loaded, loaded_on):
    T, path = sb.BATCHES[batch]["max_clock"], str(tmp_path / "ck.bin")
    set_switches(monkeypatch, oracle, saved)
    src = started(amd, batch, m, lanes)
    src.save_checkpoint(path)
    assert_equal_to_ref(run_to_end(src, T, 211), reference(oracle, batch, m))
    plan = assert_ran_on(oracle, src, batch, m, lanes, saved, saved_on)
    src.close()
    set_switches(monkeypatch, oracle, loaded)
    dst = sb.make_sim(amd, batch, np.zeros(m, dtype=np.uint64), lanes)  # (the seeds live in the state)
    dst.load_checkpoint(path)
    assert_equal_to_ref(run_to_end(dst, T, 97), reference(oracle, batch, m))
    other = assert_ran_on(oracle, dst, batch, m, lanes, loaded, loaded_on)
    assert (plan["kernel"], plan["blw"]) != (other["kernel"], other["blw"])
    dst.close()


# (d) ... and across kernel families or ring sizes they are refused, with the message that names the switches; the batch then loads the
# same image without the switch
@pytest.mark.parametrize("batch,m,switch", [("c1_n4_equiv", 70, NO_LEAN), ("c1_n7_equiv", 70, NO_LEAN), ("c2_n40", 3, LEAN2_OFF),
                                                  ("c2_n40", 3, dict(LBFT_RING="128"))],
                         ids=["run1l-NO_LEAN", "run1l-calendar-NO_LEAN", "run2l-LEAN2=0", "ring512-RING=128"])
def test_checkpoint_of_another_family_is_refused(amd, oracle, monkeypatch, tmp_path, batch, m, switch):
    T, path = sb.BATCHES[batch]["max_clock"], str(tmp_path / "ck.bin")
    set_switches(monkeypatch, oracle, {})
    src = started(amd, batch, m, 0)
    src.save_checkpoint(path)
    src.close()
    set_switches(monkeypatch, oracle, switch)
    dst = sb.make_sim(amd, batch, np.zeros(m, dtype=np.uint64))
    with pytest.raises(amd.LbftError) as e:
        dst.load_checkpoint(path)
    assert e.value.code == INVALID
    assert "LBFT_NO_LEAN / LBFT_LEAN2 / LBFT_RING tuning variables" in str(e.value)
    set_switches(monkeypatch, oracle, {})
    dst.load_checkpoint(path)
    assert_equal_to_ref(run_to_end(dst, T, cuts_of(batch, 97)[1]), reference(oracle, batch, m))
    assert_ran_on(oracle, dst, batch, m, 0, {})
    dst.close()


def test_no_switch_is_left_set():
    """The module's last test: monkeypatch has restored the environment after every test above."""
    import oracle_ctypes
    assert [n for n in oracle_ctypes.SWITCHES if n in os.environ] == []
