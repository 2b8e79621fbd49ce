"""Runs on used memory (CPU-only): the host build of the kernel logic started on state rows and an emulated LDS that hold a fill pattern
instead of zeros -- what a batch that ran before, or another batch's freed pages, leave behind on the device -- must still equal the
oracle bit for bit.  Only the rows the device's host code clears before every run (the calendar's head / tail / bitmap rows,
lbft_hip.hip zero_calendar) are cleared here too; every other word has to be written by Simulator::new (SimT::init) before the run
reads it.  A word that is only right because fresh pages are zero fails here under at least one of the patterns."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_commit_times_host_model as ctm  # noqa: E402
import test_node_level_fuzz as nlf  # noqa: E402
import test_param_sets_host_model as psm  # noqa: E402
from support import set_oracle_cfg  # noqa: E402
from test_fuzz_model import draw_caps, draw_config, draw_large_caps, draw_large_config  # noqa: E402
from test_host_model import round_switch_rows  # noqa: E402
from test_save_node import EPOCH_CASES  # noqa: E402

# 0 = fresh pages (the control); all-ones and a mixed pattern (large indices, set flag bits, negative times); 0x00010001 = small
# plausible values (a count of 1, slot / block index 1, bit 0 of every mask) that pass range checks a wild word would trip
FILLS = (0, 0xA5A5A5A5, 0xFFFFFFFF, 0x00010001)
DIRTY = FILLS[1:]

# lbft_hostmodel_last_class: KernelClass of the step (lbft_core.h) | cooperative loop << 8 | heap << 9 | calendar << 10
CLASS_NAMES = {0: "small", 9: "quad", 3: "generic", 1: "mid", 6: "mid_lean", 2: "large", 5: "large_lean", 7: "large_exchange"}
WANTED = set(CLASS_NAMES.values()) | {"heap", "calendar", "coop_128", "coop_256", "coop_512"}
_REACHED = {}

RESULT_KEYS = ("commit_counts", "active_rounds", "last_states", "histories")
COUNTER_KEYS = ("events", "rng_draws", "rounds", "commits", "events_scheduled")


def last_class(oracle):
    import ctypes as C
    f = oracle.hostmodel_lib().lbft_hostmodel_last_class
    f.restype = C.c_uint32
    return int(f())


def ran_as(oracle, caps):
    """The names of WANTED the last host-model run counts for."""
    word = last_class(oracle)
    names = {CLASS_NAMES[word & 0xff]}
    if word & 0xff not in (0, 9, 3):  # (outside class 0 and the generic step: the queue discipline)
        names.add("calendar" if word & 1024 else "heap" if word & 512 else "array")
    if word & 256:
        names.add("coop_%d" % caps["ring"])
    return names


def assert_equal(a, b, what):
    assert not b["faults"].any(), (what, sorted(set(int(f) for f in b["faults"])))
    for key in RESULT_KEYS:
        assert (a[key] == b[key]).all(), (key, what)
    for key in COUNTER_KEYS:
        assert a["counters"][key] == b["counters"][key], (key, what)


def run_under_every_fill(oracle, cfg, kw, seeds, max_clock, caps, history_cap, tag):
    a = oracle.run_batch(cfg, seeds, max_clock, threads=4, history_cap=history_cap)
    for fill in FILLS:
        b = oracle.hostmodel_run_batch(cfg, seeds, max_clock, threads=4, history_cap=history_cap, state_fill=fill, **caps)
        assert_equal(a, b, (tag, hex(fill), kw, caps))
    for name in ran_as(oracle, caps):
        _REACHED[name] = _REACHED.get(name, 0) + 1


# Sized to the CPU part of tests/test_fuzz_model.py (109 s for 288 + 40 draws, one host-model run each): four host-model runs per draw here, and
# the other parts of this file take 45 s -- 160 + 4 draws (the ring sizes and classes the few large draws may miss are FIXED cases below)
SMALL_CHUNKS, SMALL_DRAWS = 10, 16
LARGE_CHUNKS, LARGE_DRAWS = 2, 2


@pytest.mark.parametrize("chunk", range(SMALL_CHUNKS))
def test_drawn_configurations_on_dirty_state_equal_the_oracle(oracle, chunk):
    """tests/test_fuzz_model.py's generator and capacities (other draws): every configuration under every fill pattern."""
    rng = np.random.default_rng(515000 + chunk)
    for _ in range(SMALL_DRAWS):
        kw = draw_config(rng)
        n = kw["num_nodes"]
        max_clock = int(rng.choice([300, 600, 1000])) if n <= 16 else 250
        seeds = rng.integers(1, 2 ** 62, 6 if n <= 16 else 2, dtype=np.uint64)
        cfg = oracle.make_config(math_mode=1, **kw)
        run_under_every_fill(oracle, cfg, kw, seeds, max_clock, draw_caps(rng, kw), 96, "drawn")


@pytest.mark.parametrize("chunk", range(LARGE_CHUNKS))
def test_drawn_large_configurations_on_dirty_state_equal_the_oracle(oracle, chunk):
    """33..128 nodes through the cooperative loop: the ring of pre-generated draws and the LDS window of block records start dirty."""
    rng = np.random.default_rng(626000 + chunk)
    for _ in range(LARGE_DRAWS):
        kw, n, max_clock = draw_large_config(rng)
        seeds = rng.integers(1, 2 ** 62, 1, dtype=np.uint64)
        cfg = oracle.make_config(math_mode=1, **kw)
        run_under_every_fill(oracle, cfg, kw, seeds, max_clock, draw_large_caps(rng, kw), 64, "large")


# One fixed case per entry of WANTED (the issue's hand-picked configurations and the three ring sizes), so that the coverage assertion
# below does not depend on what the draws happen to reach: (configuration, instances, max_clock, capacities, what it must run as)
def _caps(n, **kw):
    caps = dict(qcap=max(4096, 32 * n * n), scap=max(128, 128 * n), bcap=1024, lcap=1024, ql=0, qheap=0, qcal=0)
    caps.update(kw)
    return caps


FIXED = {
    "quad_lds_queue": (dict(num_nodes=4), 8, 1000, _caps(4, qcap=256, scap=64, ql=48), {"quad"}),
    "quad_hbm_queue": (dict(num_nodes=4), 8, 1000, _caps(4, qcap=256, scap=64, ql=0), {"quad"}),
    "small_uniform": (dict(num_nodes=4, delay_model=1, uniform_lo=5, uniform_hi=15), 8, 1000, _caps(4, qcap=256, scap=64, ql=11), {"small"}),
    "force_generic": (dict(num_nodes=4), 8, 1000, _caps(4, qcap=256, scap=64, ql=11, force_generic=1), {"generic"}),
    "n4_epochs": (dict(num_nodes=4, commands_per_epoch=5, quirks=2), 8, 1000, _caps(4, qcap=256, scap=64, ql=16), set()),
    "mid_lean_n8_heap": (dict(num_nodes=8), 6, 600, _caps(8, qheap=1), {"mid_lean", "heap"}),
    "mid_lean_n8_cal": (dict(num_nodes=8), 6, 600, _caps(8, qheap=1, qcal=1), {"mid_lean", "calendar"}),
    "mid_n7_equivocators_lossy": (dict(num_nodes=7, equivocate_every=3, drop_per_million=100000), 6, 1000, _caps(7, qheap=1), {"mid", "heap"}),
    "mid_n7_q3_rotating_cal": (dict(num_nodes=7, quirks=3, commands_per_epoch=9, voting_rights=[2, 1, 1, 3, 1, 2, 1], rights_rotation=3), 6, 1500,
                               _caps(7, qheap=1, qcal=1), {"mid", "calendar"}),
    "large_lean_n40_heap": (dict(num_nodes=40), 2, 250, _caps(40, qheap=1), {"large_lean", "heap"}),
    "large_lean_n40_cal": (dict(num_nodes=40), 2, 250, _caps(40, qheap=1, qcal=1), {"large_lean", "calendar"}),
    "large_lean_n40_coop128": (dict(num_nodes=40), 2, 250, _caps(40, qheap=1, qcal=1, ring=128, ring_topup=4), {"large_lean", "coop_128"}),
    "large_lean_n64_coop256": (dict(num_nodes=64, mean=10.0, variance=400.0), 1, 250, _caps(64, qheap=1, qcal=1, ring=256, ring_topup=16),
                               {"large_lean", "coop_256"}),
    "large_exchange_n66_q1_coop512": (dict(num_nodes=66, quirks=1), 1, 200, _caps(66, scap=6 * 66 * 66 + 16 * 66, qheap=1, qcal=1, ring=512, ring_topup=0),
                                      {"large_exchange", "coop_512"}),
    "large_n40_lossy_partition": (dict(num_nodes=40, drop_per_million=20000, partition_size=13, partition_start=50, partition_end=150), 2, 250,
                                  _caps(40, qheap=1, qcal=1), {"large", "calendar"}),
}


_FIXED_DONE = set()


def run_fixed(oracle, name):
    kw, m, max_clock, caps, must = FIXED[name]
    seeds = np.arange(1, m + 1, dtype=np.uint64) * 104729 + 17
    run_under_every_fill(oracle, oracle.make_config(math_mode=1, **kw), kw, seeds, max_clock, caps, 128, name)
    assert must <= ran_as(oracle, caps), (name, ran_as(oracle, caps))
    _FIXED_DONE.add(name)


@pytest.mark.parametrize("name", sorted(FIXED))
def test_fixed_configurations_on_dirty_state_equal_the_oracle(oracle, name):
    run_fixed(oracle, name)


def test_every_class_ran_on_dirty_state(oracle):
    """Every step specialisation, queue discipline and ring size the CPU fuzz reaches was started on dirty state at least once: by the
    draws and fixed cases above (selected alone, this test runs the fixed cases itself)."""
    for name in sorted(set(FIXED) - _FIXED_DONE):
        run_fixed(oracle, name)
    print("ran as:", dict(sorted(_REACHED.items())))
    assert WANTED <= set(_REACHED), (sorted(WANTED - set(_REACHED)), _REACHED)


@pytest.mark.parametrize("n,max_clock", [(3, 1000), (5, 1500), (8, 600)])
def test_round_trace_on_dirty_state_equals_data_writer(oracle, n, max_clock):
    """The trace rows (first_time[n][rcap], max_round[n]) are written in full by Simulator::new."""
    kw = dict(num_nodes=n) if n != 5 else dict(num_nodes=5, mean=10.0, variance=400.0)
    cfg = oracle.make_config(math_mode=1, **kw)
    seeds = np.arange(50, 54, dtype=np.uint64)
    want = []
    for seed in seeds:
        sim = oracle.OracleSim(cfg, int(seed)).enable_data_writer()
        sim.run_until(max_clock)
        want.append(sim.round_switches()[0])
        assert len(want[-1]) > 3
    for fill in FILLS:
        b = oracle.hostmodel_run_batch(cfg, seeds, max_clock, threads=4, qcap=4096, scap=64, bcap=512, lcap=512, ql=11, rcap=400, state_fill=fill)
        assert not b["faults"].any(), hex(fill)
        for i in range(len(seeds)):
            assert round_switch_rows(b["round_switches"][i], b["max_rounds"][i]) == want[i], (hex(fill), i)


@pytest.mark.parametrize("name", ["n4_q3_cpe5", "n7_rotating_rights_q3_cpe3", "n40_weighted_rotating_q3_cpe3"])
def test_retired_stores_on_dirty_state_equal_the_oracle_image(oracle, name):
    """keep_stores + epoch changes: the archive of retired record stores (an unused entry must read as "no store") and the snapshot-format
    summaries behind the save_node image of every node."""
    kw, seed, horizons = EPOCH_CASES[name]
    cfg = oracle.make_config(math_mode=1, **kw)
    n, t = kw["num_nodes"], horizons[0]
    sim = oracle.OracleSim(cfg, seed).run_until(t)
    want = [sim.save_node(node) for node in range(n)]
    assert max(sim.epochs()) >= 1
    caps = dict(qcap=max(4096, 8 * n * n), scap=(n * n + 8 * n + 64), bcap=1024, lcap=1024, ql=0, qheap=1 if n > 16 else 0, qcal=1 if n > 32 else 0,
                ring=256 if n > 32 else 0, tw=8 if n > 32 else 0, keep_stores=1)
    for fill in FILLS:
        rt = []
        images = oracle.hostmodel_node_images(cfg, seed, t, roundtrip=rt, state_fill=fill, **caps)
        assert images == want, (name, hex(fill), [k for k in range(n) if images[k] != want[k]])
        assert rt == [0] * n, (name, hex(fill), rt)  # save -> scrub -> load_node_image -> save, and the summaries the record exchange reads


class Recorded:
    """A HostSession that keeps every call, view and image it served."""

    def __init__(self, hs):
        self.hs, self.log = hs, []

    def call(self, *a):
        r = self.hs.call(*a)
        self.log.append(("call", a, r))
        return r

    def view(self, *a):
        r = self.hs.view(*a)
        self.log.append(("view", a, r))
        return r

    def save_node(self, *a):
        r = self.hs.save_node(*a)
        self.log.append(("save", a, r))
        return r


def replay(oracle, spec, caps, fill):
    hs = oracle.HostSession(nlf.oracle_config(oracle, spec), [spec["seed"]], spec["max_clock"], caps, state_fill=fill)
    rec = Recorded(hs)
    ora = nlf.OracleSide(oracle, spec)
    stats = nlf.new_stats()
    nlf.drive_single(rec, 0, ora, spec, stats, caps["scap"])
    fault, live, _ = hs.fault(0)
    assert fault == 0 and live == 0, (hex(fill), fault, live)
    nlf.compare_end(nlf.host_end(hs, 0, spec["n"]), ora, spec, stats)
    return rec.log, stats


# (3 nodes with both quirks fixed and two epoch changes; 5 nodes with the record exchange and retired stores; 32 and 65 nodes; 33 nodes with the record exchange)
@pytest.mark.parametrize("seed,n", [(8, None), (13, None), (2, None), (10, None), (1001, 33)])
def test_node_level_session_on_dirty_state_equals_the_zero_fill_replay(oracle, seed, n):
    """lbft_batch_manual_begin on used memory: a session of tests/test_node_level_fuzz.py's generator, call for call against the oracle
    and against its own replay on zeroed rows."""
    spec = nlf.draw_spec(seed, n=n, exchange_big=n is not None)
    caps = oracle.manual_caps(spec["n"], spec["quirks"], spec["max_clock"], keep_stores=spec["keep_stores"])
    try:
        clean, stats = replay(oracle, spec, caps, 0)
    except nlf.Capacity:  # (a pool of the session's automatic capacities ran out on clean rows already: the same session with room)
        caps = oracle.manual_caps(spec["n"], spec["quirks"], spec["max_clock"], keep_stores=spec["keep_stores"], **nlf.roomy_caps(oracle, spec))
        clean, stats = replay(oracle, spec, caps, 0)
    assert stats["calls"] > 20
    for fill in DIRTY:
        log, _ = replay(oracle, spec, caps, fill)
        assert len(log) == len(clean)
        for k, (a, b) in enumerate(zip(log, clean)):
            assert a == b, (hex(fill), k, a[:2])


def test_parameter_set_model_on_dirty_state(oracle, tmp_path_factory):
    L = psm.load_harness(tmp_path_factory.mktemp("ps_dirty"))
    rng = np.random.default_rng(737000)
    classes = set()
    for n in (4, 7):
        while True:  # (a grid for the small class and one for the mid class: the first draw of each that lands there)
            base, sets = psm.draw_batch(rng, n)
            m, max_clock = 24, 500
            set_of = np.arange(m) % len(sets)
            seeds = rng.integers(1, 2 ** 62, m, dtype=np.uint64)
            cls, clean = psm.run_host(L, base, sets, set_of, seeds, max_clock, 64)
            if (n == 4) == (cls == 0):
                break
        classes.add(cls)
        assert not clean["faults"].any()
        for i in range(m):
            s = sets[set_of[i]]
            cfg = oracle.make_config(num_nodes=n, math_mode=1, mean=s.mean, variance=s.variance, delay_model=base.delay_model, uniform_lo=s.uniform_lo,
                                     uniform_hi=s.uniform_hi, commands_per_epoch=base.commands_per_epoch, target_commit_interval=s.target_commit_interval,
                                     delta=s.delta, gamma=s.gamma, lambda_=s.lambda_, quirks=base.quirks, equivocate_every=base.equivocate_every,
                                     drop_per_million=s.drop_per_million, partition_size=s.partition_size, partition_start=s.partition_start,
                                     partition_end=s.partition_end)
            ref = oracle.run_batch(cfg, seeds[i:i + 1], max_clock, history_cap=64)
            for key in RESULT_KEYS:
                assert (clean[key][i] == ref[key][0]).all(), (key, n, i)
        for fill in DIRTY:
            cls2, dirty = psm.run_host(L, base, sets, set_of, seeds, max_clock, 64, state_fill=fill)
            assert cls2 == cls
            for key in RESULT_KEYS + ("faults",):
                assert (dirty[key] == clean[key]).all(), (key, n, hex(fill))
    assert classes == {0, 1}


def test_commit_time_model_on_dirty_state(oracle, tmp_path_factory):
    L = ctm.load_harness(tmp_path_factory.mktemp("ct_dirty"))
    rng = np.random.default_rng(848000)
    classes = set()
    for n, n_sets, small in ((4, 0, True), (7, 0, False), (6, 3, False)):
        base, sets, all_sets, rights = ctm.draw(rng, n, n_sets, small)
        m, max_clock, cap = 12, 400, 64
        set_of = np.arange(m) % max(n_sets, 1)
        seeds = rng.integers(1, 2 ** 62, m, dtype=np.uint64)
        cls, clean = ctm.run_host(L, base, sets, set_of, seeds, max_clock, cap)
        classes.add((cls, bool(n_sets)))
        assert not clean["faults"].any()
        for i in range(m):  # the oracle's histories and the commit times derived from fresh oracle runs
            cfg = set_oracle_cfg(oracle, base, all_sets[set_of[i]], rights)
            ref = oracle.run_batch(cfg, seeds[i:i + 1], max_clock, history_cap=cap)
            assert (clean["commit_counts"][i] == ref["commit_counts"][0]).all() and (clean["histories"][i] == ref["histories"][0]).all(), (n, i)
            want = ctm.cto.commit_times(oracle, cfg, int(seeds[i]), max_clock, cap)
            assert (clean["commit_times"][i] == want).all(), (n, i)
        for fill in DIRTY:
            cls2, dirty = ctm.run_host(L, base, sets, set_of, seeds, max_clock, cap, state_fill=fill)
            assert cls2 == cls
            for key in ("commit_counts", "commit_times", "histories", "startup_times", "faults"):
                assert (dirty[key] == clean[key]).all(), (key, n, hex(fill))
    assert (0, False) in classes and (1, False) in classes and any(s for _, s in classes)
