"""Randomised device test of the twin run kernels of the side libraries: the parameter-set kernels of liblbft_paramsets.so (lbft_k_ps_run0 /
lbft_k_ps_run1) and the commit-time kernels of liblbft_commit_times.so (lbft_k_ct_run0 / 1, lbft_k_ct_ps_run0 / 1), against the oracle.

Each chunk takes the shape of its draws -- node count, size class, batch kind -- from SHAPES, so that the default chunks launch every
twin, and draws everything else at random: delay model, epoch length, quirks, equivocators, voting rights and their rotation, and per
parameter set delay mean / variance or span, pacemaker parameters, target_commit_interval, loss and partitions; 1 .. 16 sets (sometimes one
that no instance uses) assigned blocked, interleaved or at random; lanes per wavefront, multi-launch and the calendar queue.

Per draw: no fault; the layout flags of the kernel that ran; every set against the oracle run of its configuration (commit counts, active
rounds, last states, histories, startup times) and the batch's counters against the sum over the sets.  Timed draws also: the recorded
commit times of every instance against the ones derived from fresh oracle runs (tests/commit_times_oracle.py), the untimed twin of the
same batch giving identical results, and the device latency histogram against numpy.

LBFT_FUZZ_TWIN_CHUNKS=n widens the run (three draws per chunk), LBFT_FUZZ_TWIN_FIRST=k starts at chunk k (other draws)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import commit_times_oracle as cto  # noqa: E402

HOST_THREADS = min(os.cpu_count() or 8, 16)
TIMED, SETS, TIMED_SETS = "timed", "sets", "timed_sets"
# the twin each (size class, batch kind) runs on
KERNELS = {(0, TIMED): "lbft_k_ct_run0", (1, TIMED): "lbft_k_ct_run1", (0, SETS): "lbft_k_ps_run0", (1, SETS): "lbft_k_ps_run1",
           (0, TIMED_SETS): "lbft_k_ct_ps_run0", (1, TIMED_SETS): "lbft_k_ct_ps_run1"}
# (nodes, size class, batch kind): chunk c draws SHAPES[3c], SHAPES[3c + 1], SHAPES[3c + 2] (cyclically).  Class 1 with <= 4 nodes: the
# draw adds what takes a small network out of class 0 (an equivocator, loss, a partition or quirks bit 0).
SHAPES = [
    (4, 0, TIMED_SETS), (20, 1, TIMED_SETS), (7, 1, SETS),
    (2, 0, TIMED), (32, 1, TIMED), (3, 1, TIMED_SETS),
    (1, 0, SETS), (17, 1, TIMED_SETS), (12, 1, TIMED),
    (4, 1, TIMED), (24, 1, SETS), (3, 0, TIMED_SETS),
    (16, 1, TIMED_SETS), (5, 1, TIMED), (4, 0, SETS),
    (31, 1, TIMED_SETS), (8, 1, SETS), (1, 0, TIMED),
]
DRAWS = 3
DEFAULT_CHUNKS = len(SHAPES) // DRAWS
FIRST = int(os.environ.get("LBFT_FUZZ_TWIN_FIRST", "0"))
CHUNKS = int(os.environ.get("LBFT_FUZZ_TWIN_CHUNKS", str(DEFAULT_CHUNKS)))
LAYOUT_SETS, LAYOUT_TIMED = 1 << 16, 1 << 17

# what the chunks of this session saw, for the coverage guard at the end of the module
SEEN = {}


def draw_set(rng, uniform, cls, n):
    s = {}
    if uniform:
        s.update(uniform_lo=int(rng.integers(0, 8)), uniform_hi=int(rng.integers(8, 30)))
    else:
        s.update(mean=float(rng.choice([3.0, 10.0, 10.0, 25.0])), variance=float(rng.choice([0.0, 4.0, 4.0, 100.0, 400.0])))
    if rng.random() < 0.6:
        # (lambda * delta >= 2: a query period of 0 makes every update query all peers and the event population explode)
        s.update(delta=int(rng.choice([5, 10, 20, 40])), gamma=float(rng.choice([1.0, 1.5, 2.0])), lambda_=float(rng.choice([0.5, 1.0])))
    if rng.random() < 0.3:
        s["target_commit_interval"] = int(rng.choice([50, 200, 100000]))
    if cls == 1 and rng.random() < 0.3:
        s["drop_per_million"] = int(rng.choice([1000, 50000, 300000]))
    if cls == 1 and n >= 2 and rng.random() < 0.25:
        start = int(rng.integers(0, 200))
        s["partition"] = (int(rng.integers(1, n)), start, start + int(rng.integers(50, 300)))
    return s


def draw(rng, n, cls, kind):
    """One draw of the shape (n, cls, kind): the batch-wide configuration, the sets, their assignment, seeds, horizon and knobs."""
    d = dict(n=n, cls=cls, kind=kind, uniform=bool(rng.random() < 0.35))
    base = {}
    if rng.random() < 0.45:
        base["commands_per_epoch"] = int(rng.choice([3, 7, 20]))
    base["quirks"] = int(rng.choice([0, 0, 1, 2, 3])) & (2 if cls == 0 else 3)
    if cls == 1 and n >= 2 and rng.random() < 0.35:
        base["equivocate_every"] = int(rng.integers(1, n + 1))
    if rng.random() < 0.4:
        base["voting_rights"] = [int(v) for v in rng.integers(1, 6, n)]
        if "commands_per_epoch" in base and n >= 2 and rng.random() < 0.6:
            base["rights_rotation"] = int(rng.integers(1, n))  # epoch reconfiguration: the rights rotate with the epoch
    n_sets = int(rng.choice([1, 2, 3, 5, 8, 16])) if kind != TIMED else 1
    sets = [draw_set(rng, d["uniform"], cls, n) for _ in range(n_sets)]
    if cls == 1 and n <= 4 and not (base.get("equivocate_every") or base["quirks"] & 1 or
                                    any("drop_per_million" in s or "partition" in s for s in sets)):
        way = int(rng.integers(0, 3 if n >= 2 else 2))
        if way == 0:
            base["quirks"] |= 1
        elif way == 1:
            sets[0]["drop_per_million"] = 50000
        else:
            base["equivocate_every"] = int(rng.integers(1, n + 1))
    # instances: at most 64 (16 for 5 .. 16 nodes, 8 above) -- every one of them gets its commit times by bisection over fresh oracle runs
    per = int(rng.choice([1, 2, 3, 4])) if n <= 16 else int(rng.choice([1, 2]))
    per = min(per, max(1, (64 if n <= 4 else 16 if n <= 16 else 8) // n_sets))
    how = str(rng.choice(["blocked", "interleaved", "random"]))
    k = np.arange(n_sets * per)
    set_of = k // per if how == "blocked" else k % n_sets if how == "interleaved" else rng.integers(0, n_sets, len(k))
    if n_sets >= 2 and rng.random() < 0.3:  # a set that no instance uses
        unused = int(rng.integers(0, n_sets))
        set_of = np.where(set_of == unused, (unused + 1) % n_sets, set_of)
    d.update(base=base, sets=sets, set_of=set_of.astype(np.uint32), how=how)
    d["seeds"] = rng.integers(1, 2 ** 62, len(set_of), dtype=np.uint64)
    # (the bisection re-runs an instance about log2(max_clock) times per distinct commit time: a 1-node network commits at almost every
    # time unit; timed horizons stay short)
    if n > 16:
        d["max_clock"] = 250
    else:
        d["max_clock"] = int(rng.choice([300, 600, 1000] if kind == SETS else [300, 600] if n <= 4 else [300]))
    d["lpw"] = int(rng.choice([0, 1, 2, 8, 32, 64]))
    d["steps"] = int(rng.choice([0, 173]))
    d["calendar"] = bool(rng.random() < 0.6)
    d["auto_snapshots"] = bool(rng.random() < 0.5)
    return d


def chunk_draws(chunk):
    rng = np.random.default_rng(60606 + chunk)
    return [draw(rng, *SHAPES[(chunk * DRAWS + j) % len(SHAPES)]) for j in range(DRAWS)]


def make_batch(amd, d, timed):
    """The draw's batch (a parameter-set batch for the kinds with sets), with the capacities the device fuzz of test_fuzz_model.py uses."""
    n, mc, base = d["n"], d["max_clock"], d["base"]

    def delay(s):
        return amd.RandomDelay.uniform(s["uniform_lo"], s["uniform_hi"]) if d["uniform"] else amd.RandomDelay.new(s["mean"], s["variance"])

    def node_config(s):
        return amd.NodeConfig(s.get("target_commit_interval", 100000), s.get("delta", 20), s.get("gamma", 2.0), s.get("lambda_", 0.5))
    kw = dict(commands_per_epoch=base.get("commands_per_epoch", 30000), voting_rights=base.get("voting_rights"),
              equivocate_every=base.get("equivocate_every", 0), quirks=base["quirks"], rights_rotation=base.get("rights_rotation", 0),
              calendar_queue=d["calendar"], max_steps_per_launch=d["steps"], lanes_per_wavefront=d["lpw"], commit_times=timed,
              # (equivocators propose twice per round: test_fuzz_model.py)
              block_capacity=(2 * mc + 256) if base.get("equivocate_every") else mc + 64)
    if d["cls"] == 1:
        # class 0 keeps the automatic capacities (an explicit queue above 256 or more than 256 snapshot slots leave class 0); class 1:
        # test_fuzz_model.py's rules (0 = automatic snapshots; n > 16 with quirks bit 0: the record exchange's query-all responses)
        kw["queue_capacity"] = max(4096, 64 * n * n)
        q1 = base["quirks"] & 1
        kw["snapshot_capacity"] = (0 if not q1 and d["auto_snapshots"] else
                                   (min(65535, 6 * n * n + 16 * n) if (n > 16 and q1) else max(128, 128 * n)))
    if d["kind"] == TIMED:
        s = d["sets"][0]
        return amd.BatchSimulator.new(d["seeds"], n, delay(s), node_config(s), drop_per_million=s.get("drop_per_million", 0),
                                      partition=s.get("partition"), **kw)
    sets = [amd.ParamSet(delay(s), node_config(s), drop_per_million=s.get("drop_per_million", 0), partition=s.get("partition"))
            for s in d["sets"]]
    return amd.BatchSimulator.with_param_sets(d["seeds"], n, sets, d["set_of"], **kw)


def oracle_config(oracle, d, k):
    base, s = d["base"], d["sets"][k]
    part = s.get("partition") or (0, 0, 0)
    delay = dict(delay_model=1, uniform_lo=s["uniform_lo"], uniform_hi=s["uniform_hi"]) if d["uniform"] else \
        dict(mean=s["mean"], variance=s["variance"])
    return oracle.make_config(num_nodes=d["n"], math_mode=1, commands_per_epoch=base.get("commands_per_epoch", 30000), quirks=base["quirks"],
                              equivocate_every=base.get("equivocate_every", 0), voting_rights=base.get("voting_rights"),
                              rights_rotation=base.get("rights_rotation", 0), target_commit_interval=s.get("target_commit_interval", 100000),
                              delta=s.get("delta", 20), gamma=s.get("gamma", 2.0), lambda_=s.get("lambda_", 0.5),
                              drop_per_million=s.get("drop_per_million", 0), partition_size=part[0], partition_start=part[1],
                              partition_end=part[2], **delay)


def check_draw(amd, oracle, d):
    """Runs the draw and checks it; returns what the coverage guard counts."""
    timed = d["kind"] != SETS
    has_sets = d["kind"] != TIMED
    n, mc, seeds, set_of = d["n"], d["max_clock"], d["seeds"], d["set_of"]
    sim = make_batch(amd, d, timed)
    res = sim.loop_until(mc, allow_faults=True)
    lay = sim.layout()
    flags = lay["kernel_class"]
    why = {k: v for k, v in d.items() if k not in ("seeds", "set_of")}
    assert not res.faults.any(), (why, sorted(set(int(f) for f in res.faults)), res.counters, lay)
    assert flags & 0xff == d["cls"], (hex(flags), why)
    assert bool(flags & LAYOUT_SETS) == has_sets and bool(flags & LAYOUT_TIMED) == timed, (hex(flags), why)
    if d["lpw"]:
        assert lay["lanes_per_wavefront"] == d["lpw"], (lay, why)
    ctr = res.counters
    if not d["steps"]:
        assert ctr["launches"] == 1, ctr
    elif sum(ctr["events"]) > 173 * len(seeds):  # (some instance ran more than one launch's worth of events)
        assert ctr["launches"] > 1, ctr
    cap = max(1, int(res.commit_counts.max()))
    hist = res.committed_histories(cap)
    configs = [oracle_config(oracle, d, k) for k in range(len(d["sets"]))]
    want = {"events": [0, 0, 0, 0], "rng_draws": 0, "rounds": 0, "commits": 0, "events_scheduled": 0}
    for k, cfg in enumerate(configs):
        idx = np.nonzero(set_of == k)[0]
        if not len(idx):
            continue
        ref = oracle.run_batch(cfg, seeds[idx], mc, threads=HOST_THREADS, history_cap=cap)
        assert (res.commit_counts[idx] == ref["commit_counts"]).all(), (k, why)
        assert (res.active_rounds[idx] == ref["active_rounds"]).all(), (k, why)
        assert (res.last_committed_states[idx] == ref["last_states"]).all(), (k, why)
        assert (hist[idx] == ref["histories"]).all(), (k, why)
        for i in idx:
            o = oracle.OracleSim(cfg, int(seeds[i]))
            assert list(res.startup_times[i]) == o.startup_times(), (k, int(i), why)
            o.close()
        rc = ref["counters"]
        want["events"] = [a + b for a, b in zip(want["events"], rc["events"])]
        for key in ("rng_draws", "rounds", "commits", "events_scheduled"):
            want[key] += rc[key]
    for key in want:
        assert ctr[key] == want[key], (key, ctr[key], want[key], why)
    if timed:
        ct = res.commit_times()
        ref_ct = cto.param_set_commit_times(oracle, configs, set_of, seeds, mc, ct.shape[2], HOST_THREADS)
        bad = np.argwhere(ct != ref_ct)
        assert not len(bad), (bad[:5].tolist(), why)
        assert ((ct >= 0).sum(axis=2) == res.commit_counts).all(), why
        untimed = make_batch(amd, d, False)
        cto.same_results(res, untimed.loop_until(mc, allow_faults=True))
        untimed.close()
        groups = len(d["sets"]) if has_sets else 1
        h_dev, s_dev = res.latency_histogram()
        h_np, s_np, _, _ = cto.numpy_histogram(res, 1, mc + 1, set_of if has_sets else None, groups)
        assert (h_dev == h_np).all() and (s_dev == s_np).all(), why
    facts = dict(kernel=KERNELS[(d["cls"], d["kind"])], launches=int(ctr["launches"]), epochs=int(res.epochs.max()),
                 timed_sets_over_16=timed and has_sets and n > 16)
    sim.close()
    return facts


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(FIRST, FIRST + CHUNKS))
def test_twin_kernels_match_the_oracle(oracle, chunk):
    import torch
    assert torch.cuda.is_available(), "this test needs the MI355X"
    import librabft_simulator_amd as amd
    amd.lib()
    SEEN[chunk] = [dict(check_draw(amd, oracle, d), draw=d) for d in chunk_draws(chunk)]


@pytest.mark.gpu
def test_default_chunks_cover_every_twin_and_feature():
    """Guard over the default chunks (run in this session, before this test): every twin ran, and so did each feature the twins'
    device-only code must be seen with."""
    missing = [c for c in range(DEFAULT_CHUNKS) if c not in SEEN]
    if missing:
        pytest.skip("the default chunks %s did not run in this session (run the whole module)" % missing)
    runs = [r for c in range(DEFAULT_CHUNKS) for r in SEEN[c]]
    draws = [r["draw"] for r in runs]
    assert {r["kernel"] for r in runs} == set(KERNELS.values())
    assert any(r["timed_sets_over_16"] for r in runs), "a timed parameter-set batch of more than 16 nodes"
    assert any(d["base"]["quirks"] & 1 for d in draws), "quirks bit 0"
    assert any(r["epochs"] > 0 for r in runs), "an epoch change"
    assert any(d["base"].get("equivocate_every") for d in draws), "equivocators"
    assert any(d["base"].get("rights_rotation") for d in draws), "voting rights rotating with the epoch"
    assert any(d["uniform"] for d in draws), "uniform delays"
    assert any(not d["calendar"] and d["cls"] == 1 for d in draws), "the calendar queue switched off (class 1)"
    assert any(d["lpw"] for d in draws), "lanes per wavefront other than the default"
    assert any(r["launches"] > 1 for r in runs), "more than one launch"
    assert any(d["kind"] != TIMED and (np.bincount(d["set_of"], minlength=len(d["sets"])) == 0).any() for d in draws), "an unused set"
