"""Commit times and commit latency on the device (lbft_batch_record_commit_times, liblbft_commit_times.so): the recorded times equal the ones
derived from fresh oracle runs (tests/commit_times_oracle.py) on both kernel classes and on a parameter-set batch, agree with fresh device
runs to intermediate horizons over a whole 65 536-network batch, leave every other result of the batch as it is, survive run_steps and
checkpoints; the device histogram equals numpy's, bit for bit -- in every pass of a histogram wider than the kernel's LDS, with
instances that faulted, with 256 groups of which some are empty, at extreme binnings and with the default width above 1; and the refusals
hold."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import commit_times_oracle as cto
from support import amd, oracle_cfg  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
HOST_THREADS = min(os.cpu_count() or 8, 16)
BIG = 65536


def layout_flags(sim):
    from librabft_simulator_amd import _lib
    out = np.zeros(8, dtype=np.uint32)
    assert _lib.lib().lbft_batch_layout(sim._h, out.ctypes.data) == 0
    return int(out[7])


def small_sets(amd):
    return [amd.ParamSet(amd.RandomDelay.new(5.0, 2.5), amd.NodeConfig(100000, 10, 2.0, 0.5)),
            amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, 40, 2.0, 0.25)),
            amd.ParamSet(amd.RandomDelay.new(20.0, 10.0), amd.NodeConfig(40, 20, 1.5, 0.75)),
            amd.ParamSet(amd.RandomDelay.new(10.0, 0.0), amd.NodeConfig(100000, 20, 2.0, 0.5))]


numpy_histogram = cto.numpy_histogram


@pytest.fixture(scope="module")
def big(amd):
    """The headline configuration (65 536 x 4 nodes, log-normal(10, 4), clock 1000), timed and plain."""
    seeds = np.arange(1, BIG + 1, dtype=np.uint64)
    timed = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0), commit_times=True)
    rt = timed.loop_until(1000)
    plain = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0))
    rp = plain.loop_until(1000)
    yield seeds, timed, rt, plain, rp
    timed.close()
    plain.close()


def test_class0_commit_times_equal_the_oracle(amd, oracle):
    seeds = (np.arange(256) * 7919 + 5).astype(np.uint64)
    sim = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0), commit_times=True)
    res = sim.loop_until(600)
    assert layout_flags(sim) & 0xff == 0 and layout_flags(sim) & (1 << 17) and not layout_flags(sim) & (0x3f << 10)
    ct = res.commit_times()
    ref = cto.commit_times(oracle, oracle_cfg(oracle, 4, amd.ParamSet(amd.RandomDelay.new(10.0, 4.0))), seeds, 600, ct.shape[2], HOST_THREADS)
    assert (res.faults == 0).all()
    assert (ct == ref).all()
    assert ((ct >= 0).sum(axis=2) == res.commit_counts).all()
    sim.close()


def test_class1_commit_times_equal_the_oracle(amd, oracle):
    seeds = (np.arange(64) * 104729 + 11).astype(np.uint64)
    sim = amd.BatchSimulator.new(seeds, 16, amd.RandomDelay.new(10.0, 4.0), drop_per_million=20000, commit_times=True)
    res = sim.loop_until(300)
    assert layout_flags(sim) & 0xff == 1 and layout_flags(sim) & (1 << 17) and not layout_flags(sim) & (0x3f << 10)
    ct = res.commit_times()
    ref = cto.commit_times(oracle, oracle_cfg(oracle, 16, amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), drop_per_million=20000)),
                           seeds, 300, ct.shape[2], HOST_THREADS)
    assert (res.faults == 0).all()
    assert (ct == ref).all()
    assert res.commit_counts.sum() > 0
    sim.close()


def test_param_set_commit_times_equal_the_oracle(amd, oracle):
    sets = small_sets(amd)
    set_of = (np.arange(64) % len(sets)).astype(np.uint32)
    seeds = (np.arange(64) * 31 + 7).astype(np.uint64)
    sim = amd.BatchSimulator.with_param_sets(seeds, 4, sets, set_of, commit_times=True)
    res = sim.loop_until(500)
    assert layout_flags(sim) & (1 << 16) and layout_flags(sim) & (1 << 17)
    ct = res.commit_times()
    ref = cto.param_set_commit_times(oracle, [oracle_cfg(oracle, 4, ps) for ps in sets], set_of, seeds, 500, ct.shape[2], HOST_THREADS)
    assert (res.faults == 0).all()
    assert (ct == ref).all()
    sim.close()


def test_big_batch_sample_equals_the_oracle(amd, oracle, big):
    seeds, _, rt, _, _ = big
    ct = rt.commit_times()
    idx = np.arange(0, BIG, BIG // 256)
    ref = cto.commit_times(oracle, oracle_cfg(oracle, 4, amd.ParamSet(amd.RandomDelay.new(10.0, 4.0))), seeds[idx], 1000, ct.shape[2],
                           HOST_THREADS)
    assert (ct[idx] == ref).all()


def test_big_batch_agrees_with_fresh_runs_to_three_horizons(amd, big):
    seeds, _, rt, _, _ = big
    ct = rt.commit_times()
    assert (rt.faults == 0).all()
    for t in (137, 500, 999):  # (fresh PLAIN batches: the reference is the untimed kernel path, lbft_k_run0q)
        fresh = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0))
        counts = fresh.loop_until(t).commit_counts
        assert (counts == ((ct >= 0) & (ct <= t)).sum(axis=2)).all(), t
        fresh.close()


_same_results = cto.same_results


def test_recording_changes_nothing_else(amd, big):
    _, _, rt, _, rp = big
    _same_results(rt, rp)
    seeds = np.arange(1, 513, dtype=np.uint64)
    kw = dict(drop_per_million=10000, equivocate_every=5)
    a = amd.BatchSimulator.new(seeds, 16, amd.RandomDelay.new(10.0, 4.0), commit_times=True, **kw)
    b = amd.BatchSimulator.new(seeds, 16, amd.RandomDelay.new(10.0, 4.0), **kw)
    _same_results(a.loop_until(400), b.loop_until(400))
    a.close()
    b.close()


@pytest.mark.parametrize("width,bins", [(1, None), (7, None), (5, 40)])
def test_histogram_equals_numpy_on_a_plain_batch(amd, big, width, bins):
    _, _, rt, _, _ = big
    bins = bins or -(-1001 // width)
    hist, stats = rt.latency_histogram(width, bins)
    h_np, s_np, lat, _ = numpy_histogram(rt, width, bins)
    assert lat.min() >= 0 and lat.max() <= 1000
    assert (hist == h_np).all() and (stats == s_np).all()
    if bins == 40:
        assert hist[0, -1] > 0  # the overflow bin is in use


def test_histogram_and_quantiles_on_a_param_set_batch(amd):
    sets = small_sets(amd)
    set_of = (np.arange(4096) % len(sets)).astype(np.uint32)
    sim = amd.BatchSimulator.with_param_sets(np.arange(1, 4097, dtype=np.uint64), 4, sets, set_of, commit_times=True)
    res = sim.loop_until(1000)
    for width, bins in ((1, 1001), (7, 143), (3, 50)):
        hist, stats = res.latency_histogram(width, bins)
        h_np, s_np, lat, g = numpy_histogram(res, width, bins, set_of, len(sets))
        assert (hist == h_np).all() and (stats == s_np).all(), (width, bins)
    qs = (0.0, 0.25, 0.5, 0.9, 0.99, 1.0)
    rows = res.latency_by_param_set(qs)
    assert len(rows) == len(sets)
    for k, row in enumerate(rows):
        lk = lat[g == k]
        assert row["samples"] == len(lk) and row["min"] == lk.min() and row["max"] == lk.max()
        assert row["mean"] == pytest.approx(lk.mean(), rel=1e-12)
        for q in qs:
            assert row["quantiles"][str(q)] == int(np.quantile(lk, q, method="inverted_cdf")), (k, q)
    sim.close()


def test_steps_and_checkpoint_reproduce_a_straight_run(amd, tmp_path):
    seeds = np.arange(1, 1025, dtype=np.uint64)
    mk = lambda **kw: amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.uniform(3, 17), **kw)
    straight = mk(commit_times=True)
    want = straight.loop_until(800).commit_times(200)
    a = mk(commit_times=True)
    left, _ = a.run_steps(800, 60)
    assert left > 0
    a.save_checkpoint(str(tmp_path / "ck.bin"))
    b = mk(commit_times=True)
    b.load_checkpoint(str(tmp_path / "ck.bin"))
    res = None
    for _ in range(10000):
        left, res = b.run_steps(800, 60)
        if left == 0:
            break
    assert res is not None
    assert (res.commit_times(200) == want).all()
    # ... and the stepped batch itself
    for _ in range(10000):
        left, ra = a.run_steps(800, 60)
        if left == 0:
            break
    assert (ra.commit_times(200) == want).all()
    # a timed checkpoint does not load into an untimed batch
    untimed = mk()
    with pytest.raises(amd.LbftError) as e:
        untimed.load_checkpoint(str(tmp_path / "ck.bin"))
    assert e.value.code == -1
    for s in (straight, a, b, untimed):
        s.close()


def test_refusals(amd):
    from librabft_simulator_amd import _lib
    seeds = np.arange(1, 9, dtype=np.uint64)
    with pytest.raises(amd.LbftError) as e:
        amd.BatchSimulator.new(seeds, 33, amd.RandomDelay.new(10.0, 4.0), commit_times=True)
    assert e.value.code == -3
    sim = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0))
    res = sim.loop_until(300)
    assert _lib.lib().lbft_batch_record_commit_times(sim._h, 1) == _lib.LBFT_ERR_STATE  # after a run
    with pytest.raises(amd.LbftError) as e:
        res.commit_times()
    assert e.value.code == -4
    sim.close()
    timed = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0), commit_times=True)
    with pytest.raises(amd.LbftError) as e:
        timed.manual(300)
    assert e.value.code == -3
    res = timed.loop_until(300)
    image = res.save_node(0, 1)
    with pytest.raises(amd.LbftError) as e:
        timed.load_node(0, 1, image, 300)
    assert e.value.code == -3
    timed.close()


def test_grid_cli_latency(amd):
    args = ["--nodes", "4", "--mean", "5,10", "--delta", "10,40", "--seeds-per-point", "32", "--max-clock", "500", "--assign", "interleaved"]
    out = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid", "--latency"] + args, cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.strip()]
    plain = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr[-2000:]
    plain_lines = [json.loads(l) for l in plain.stdout.splitlines() if l.strip()]
    assert [{k: v for k, v in l.items() if k != "latency"} for l in lines] == plain_lines
    assert all("latency" not in l for l in plain_lines)
    from librabft_simulator_amd import grid
    sets = [amd.ParamSet(amd.RandomDelay.new(m, 4.0), amd.NodeConfig(100000, d, 2.0, 0.5)) for m in (5.0, 10.0) for d in (10, 40)]
    set_of, seed_index = grid.set_assignment(4, 32, "interleaved")
    sim = amd.BatchSimulator.with_param_sets((1 + seed_index).astype(np.uint64), 4, sets, set_of, commit_times=True)
    rows = sim.loop_until(500).latency_by_param_set()
    assert [l["latency"] for l in lines] == json.loads(json.dumps(rows))
    sim.close()


# ---- histogram edges: later passes of the LDS histogram, faulted instances, many groups, extreme binning, reset / checkpoint ------------
LDS_BINS = 8192  # LBFT_HIST_LDS_BINS: wider histograms are binned in passes of this many bins
LOG_OVERFLOW = 1 << 3  # LBFT_FAULT_LOG_OVERFLOW
# a slow 4-node network (edge_cases.SLOW21 scaled down by 4): commit latencies of 2^14 .. 2^17 (on the MI355X: 15 768 .. 83 119), in passes
# 2 .. 8 of a width-1 histogram and past it
SLOW = dict(mean=float(2 ** 12), variance=float(2 ** 22), delta=2 ** 13, target_commit_interval=2 ** 16)
SLOW_CLOCK = 100000  # (> 65 535: the default width is 2)


@pytest.fixture(scope="module")
def slow(amd, oracle):
    seeds = np.arange(1, 513, dtype=np.uint64)
    sim = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(SLOW["mean"], SLOW["variance"]),
                                 amd.NodeConfig(SLOW["target_commit_interval"], SLOW["delta"]), commit_times=True)
    res = sim.loop_until(SLOW_CLOCK)
    assert (res.faults == 0).all()
    ct = res.commit_times()
    idx = np.arange(0, len(seeds), 64)
    ref = cto.commit_times(oracle, oracle.make_config(num_nodes=4, math_mode=1, **SLOW), seeds[idx], SLOW_CLOCK, ct.shape[2], HOST_THREADS)
    assert (ct[idx] == ref).all()
    yield res
    sim.close()


@pytest.mark.parametrize("width", [1, 3, 4096])
def test_histogram_passes_equal_numpy(slow, width):
    _, _, lat, _ = numpy_histogram(slow, 1, 1)
    # (width 1: every latency lies past the first pass, some in pass 3 and some past pass 8 -- the overflow bin of 65 536 bins)
    assert lat.min() >= LDS_BINS and (lat >= 2 * LDS_BINS).sum() > 0 and (lat >= 8 * LDS_BINS).sum() > 0, (lat.min(), lat.max())
    for bins in (8191, 8192, 8193, 16385, 65536):
        hist, stats = slow.latency_histogram(width, bins)
        h_np, s_np, _, _ = numpy_histogram(slow, width, bins)
        assert (hist == h_np).all() and (stats == s_np).all(), (width, bins)
        if width == 1:
            if bins > LDS_BINS:
                assert hist[0, LDS_BINS:].sum() > 0, bins  # counts binned in pass 2 and later
            if bins in (8193, 16385, 65536):
                assert hist[0, -1] > 0, bins  # an overflow bin in pass 2 / 3 / 8


def test_default_width_above_one(slow):
    width, bins = cto.check_default_latency(slow, SLOW_CLOCK)
    assert width == 2 and bins > LDS_BINS


def test_extreme_binning(slow):
    _, s_np, _, _ = numpy_histogram(slow, 1, 1)
    for width, bins in ((1, 1), (5, 1), (2 ** 32 - 1, None), (2 ** 32 - 1, 3)):
        hist, stats = slow.latency_histogram(width, bins)
        h_np, _, _, _ = numpy_histogram(slow, width, hist.shape[1])
        assert (hist == h_np).all() and (stats == s_np).all(), (width, bins)
        assert hist[0, 0] == stats[0, 0] > 0, (width, bins)


def test_histogram_skips_instances_with_a_fault(amd, oracle):
    """A log capacity near the median commit count: some instances, not all, raise LBFT_FAULT_LOG_OVERFLOW.  The histogram counts the
    others only; the faulted ones keep the commit times recorded below the cap, -1 at and beyond it."""
    seeds = np.arange(1, 257, dtype=np.uint64)
    probe = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0))
    cap = int(np.median(probe.loop_until(1000).commit_counts.max(axis=1)))
    probe.close()
    sim = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0), log_capacity=cap, commit_times=True)
    res = sim.loop_until(1000, allow_faults=True)
    faulted = res.faults != 0
    assert 0 < faulted.sum() < len(seeds), faulted.sum()
    assert (res.faults[faulted] & LOG_OVERFLOW).all()
    hist, stats = res.latency_histogram(1, 1001)
    h_np, s_np, _, _ = numpy_histogram(res, 1, 1001)
    assert (hist == h_np).all() and (stats == s_np).all()
    ct = res.commit_times(cap + 4)
    lat_all, _ = cto.latencies(ct, res.committed_histories(cap + 4), res.startup_times)
    assert len(lat_all) > stats[0, 0]  # (the faulted instances do hold samples: the rule matters)
    assert (ct[:, :, cap:] == -1).all()
    assert ((ct >= 0).sum(axis=2) == res.commit_counts).all()
    # up to the first overflow (the oracle's time of entry `cap` of any node) a faulted instance is the oracle's run
    idx = np.nonzero(faulted)[0][:16]
    ref = cto.commit_times(oracle, oracle.make_config(num_nodes=4, math_mode=1), seeds[idx], 1000, cap + 1, HOST_THREADS)
    for r, i in enumerate(idx):
        t_fault = ref[r, :, cap][ref[r, :, cap] >= 0].min()
        before = (ref[r, :, :cap] >= 0) & (ref[r, :, :cap] < t_fault)
        assert before.any() and (ct[i, :, :cap][before] == ref[r, :, :cap][before]).all(), int(i)
        assert (res.commit_counts[i] <= cap).all() and (res.commit_counts[i] == cap).any(), int(i)
    sim.close()


def test_many_groups_of_uneven_size(amd):
    """256 parameter sets, some empty (the last one too), of uneven sizes, one spanning several workgroups, shuffled over the batch."""
    rng = np.random.default_rng(256)
    sizes = np.array([(k * 37) % 23 for k in range(256)])
    sizes[[5, 22, 100, 101, 200, 255]] = 0
    sizes[17] = 700  # 2 800 lanes of 4 nodes: 11 workgroups of the histogram kernel
    set_of = rng.permutation(np.repeat(np.arange(256), sizes)).astype(np.uint32)
    sets = [amd.ParamSet(amd.RandomDelay.new(float(rng.choice([5.0, 10.0, 20.0])), 4.0),
                         amd.NodeConfig(int(rng.choice([40, 100000])), int(rng.choice([10, 20, 40])), 2.0, 0.5)) for _ in range(256)]
    sim = amd.BatchSimulator.with_param_sets(np.arange(1, len(set_of) + 1, dtype=np.uint64), 4, sets, set_of, commit_times=True)
    res = sim.loop_until(400)
    assert (res.faults == 0).all()
    for width, bins in ((1, 401), (7, 50)):
        hist, stats = res.latency_histogram(width, bins)
        h_np, s_np, _, _ = numpy_histogram(res, width, bins, set_of, 256)
        assert (hist == h_np).all() and (stats == s_np).all(), (width, bins)
        assert (hist[sizes == 0] == 0).all() and (stats[sizes == 0] == 0).all()
    cto.check_default_latency(res, 400, set_of, 256)
    rows = res.latency_by_param_set()
    assert all(rows[k]["samples"] == 0 and rows[k]["mean"] is None for k in np.nonzero(sizes == 0)[0])
    assert rows[17]["samples"] > 0
    sim.close()


@pytest.mark.parametrize("n,drop", [(4, 0), (7, 20000)])
def test_reset_to_another_horizon_equals_a_fresh_batch(amd, n, drop):
    """reset() and a run to another horizon: the log capacity (max_clock / 10 + 64 blocks) changes and the commit-time buffer with it."""
    seeds = np.arange(1, 301, dtype=np.uint64)
    mk = lambda: amd.BatchSimulator.new(seeds, n, amd.RandomDelay.uniform(3, 17), drop_per_million=drop, commit_times=True)
    a = mk()
    a.loop_until(300)
    for mc in (1500, 200):
        a.reset()
        ra = a.loop_until(mc)
        fresh = mk()
        rf = fresh.loop_until(mc)
        cto.same_results(ra, rf)
        assert (ra.commit_times() == rf.commit_times()).all(), mc
        assert ra.commit_times().shape == rf.commit_times().shape
        ha, hf = ra.latency_histogram(), rf.latency_histogram()
        assert (ha[0] == hf[0]).all() and (ha[1] == hf[1]).all(), mc
        cto.check_default_latency(ra, mc)
        fresh.close()
    a.close()


def test_mid_class_param_set_steps_and_checkpoint(amd, oracle, tmp_path):
    """lbft_k_ct_ps_run1 (20 nodes, loss in one set) run in pieces with a checkpoint in between equals a straight run and the oracle."""
    n, mc = 20, 300
    sets = [amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, 20, 2.0, 0.5)),
            amd.ParamSet(amd.RandomDelay.new(8.0, 9.0), amd.NodeConfig(100000, 30, 1.5, 0.75), drop_per_million=50000),
            amd.ParamSet(amd.RandomDelay.new(12.0, 2.0), amd.NodeConfig(60, 15, 2.0, 0.25), partition=(7, 100, 200))]
    set_of = (np.arange(24) % 3).astype(np.uint32)
    seeds = np.arange(1, 25, dtype=np.uint64)
    mk = lambda: amd.BatchSimulator.with_param_sets(seeds, n, sets, set_of, commit_times=True)
    straight = mk()
    rs = straight.loop_until(mc)
    assert layout_flags(straight) & 0xff == 1 and layout_flags(straight) & (3 << 16) == 3 << 16
    want = rs.commit_times()
    ref = cto.param_set_commit_times(oracle, [oracle_cfg(oracle, n, ps) for ps in sets], set_of, seeds, mc, want.shape[2], HOST_THREADS)
    assert (want == ref).all() and (want >= 0).any()
    a = mk()
    left, _ = a.run_steps(mc, 60)
    assert left > 0
    a.save_checkpoint(str(tmp_path / "ck.bin"))
    b = mk()
    b.load_checkpoint(str(tmp_path / "ck.bin"))
    for sim in (a, b):
        res = None
        for _ in range(10000):
            left, res = sim.run_steps(mc, 60)
            if left == 0:
                break
        assert res is not None
        cto.same_results(res, rs)
        assert (res.commit_times(want.shape[2]) == want).all()
    for s in (straight, a, b):
        s.close()
