"""Commit timelines on the device (BatchResult.commit_series / stall_histogram / stalls_by_param_set, lbft_k_ct_timeline) against the
numpy reference of the definitions (tests/commit_timeline_reference.py) computed from what the batch itself reads back -- commit times,
commit counts, fault words, set assignment -- on the headline batch, a mid-class batch with loss, the 64-point grid with partitions, a
long-horizon batch whose gaps lie past the first LDS pass, and a batch with faulted instances; against commit times derived from the
oracle for the control / partition scenario; and the calls' state rules, reproducibility, the grid tool and the time against the
read-back they replace."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import commit_timeline_reference as ref
from support import amd, binning  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
HOST_THREADS = min(os.cpu_count() or 8, 16)
BIG = 65536
LOG_OVERFLOW = 1 << 3  # LBFT_FAULT_LOG_OVERFLOW


def check_against_numpy(res, max_clock, binnings, set_of=None, groups=1, since=None):
    """series and stalls of `res` for every (width, bins) of `binnings` (None = the default) equal the reference on res's own read-back.
    Returns the reference's sample families and what the last binning gave."""
    ct, counts, faults = res.commit_times(), res.commit_counts, res.faults
    since_ref = None if since is None else [int(v) for v in np.broadcast_to(since, (groups,))]
    fam = ref.samples(ct, counts, faults, set_of, groups, since_ref, max_clock)
    lat_samples = res.latency_histogram()[1][:, 0]
    for width, bins in binnings:
        series = res.commit_series(width, bins)
        hist, stats = res.stall_histogram(since, width, bins)
        w, b = binning(max_clock, width, bins)
        assert series.shape == hist.shape == (groups, b) and stats.shape == (groups, 16), (width, bins)
        assert series.dtype == hist.dtype == stats.dtype == np.uint64
        assert (series == ref.series(ct, counts, faults, set_of, groups, w, b)).all(), (width, bins)
        want_hist, want_stats = ref.bin_stalls(fam, w, b)
        assert (stats == want_stats).all(), (width, bins, stats, want_stats)
        assert (hist == want_hist).all(), (width, bins)
        assert (series.sum(axis=1) == lat_samples).all()  # one sample per committed entry, as the latency histogram
        assert (hist.sum(axis=1) == stats[:, 0]).all()
    return fam, series, hist, stats


@pytest.fixture(scope="module")
def big(amd):
    """The headline configuration (65 536 x 4 nodes, log-normal(10, 4), clock 1000), recording commit times (class 0 twin)."""
    sim = amd.BatchSimulator.new(np.arange(1, BIG + 1, dtype=np.uint64), 4, amd.RandomDelay.new(10.0, 4.0), commit_times=True)
    res = sim.loop_until(1000)
    yield sim, res
    sim.close()


def grid64(amd):
    """The 64-point grid x 1 024 seeds; every fourth set carries a partition (sizes 1 and 2, windows inside and across the horizon)."""
    parts = {0: (2, 300, 600), 1: (1, 100, 250), 2: (2, 900, 1200), 3: (1, 0, 50)}
    sets = []
    for k, (m, d, lam) in enumerate((m, d, lam) for m in (5.0, 10.0, 20.0, 40.0) for d in (10, 20, 40, 80) for lam in (0.25, 0.5, 0.75, 1.0)):
        sets.append(amd.ParamSet(amd.RandomDelay.new(m, 4.0), amd.NodeConfig(100000, d, 2.0, lam), partition=parts[k // 4 % 4] if k % 4 == 0 else None))
    from librabft_simulator_amd import grid
    set_of, si = grid.set_assignment(len(sets), 1024, "interleaved")
    return sets, set_of, (1 + si).astype(np.uint64)


@pytest.fixture(scope="module")
def grid_batch(amd):
    sets, set_of, seeds = grid64(amd)
    sim = amd.BatchSimulator.with_param_sets(seeds, 4, sets, set_of, quirks=3, commit_times=True)
    res = sim.loop_until(1000, allow_faults=True)
    yield sim, res, sets, set_of
    sim.close()


def test_headline_batch_equals_numpy(big):
    _, res = big
    assert (res.faults == 0).all()
    # the exact default, bins = 1, a last bin that overflows, more bins than one LDS pass
    fam, series, _, stats = check_against_numpy(res, 1000, [(None, None), (1, 1), (7, None), (5, 40), (1, ref.LDS_BINS + 5), (13, 1)])
    assert len(fam[0][ref.GAPS]) > 4_000_000 and len(fam[0][ref.LONGEST]) == BIG * 4
    hist40 = res.stall_histogram(None, 5, 10)[0]
    assert hist40[0, -1] > 0 and res.commit_series(5, 40)[0, -1] > 0  # the overflow bins are in use
    # since in the middle of the run: `first` changes, nothing else does
    _, _, _, stats500 = check_against_numpy(res, 1000, [(None, None)], since=500)
    assert (stats500[:, :4] == stats[:, :4]).all() and (stats500[:, 8:] == res.stall_histogram()[1][:, 8:]).all()


def test_mid_class_batch_with_loss_equals_numpy(amd):
    sim = amd.BatchSimulator.new(np.arange(1, 513, dtype=np.uint64), 16, amd.RandomDelay.new(10.0, 4.0), drop_per_million=20000, commit_times=True)
    res = sim.loop_until(400)
    assert sim.layout()["kernel_class"] & 0xff == 1
    assert (res.faults == 0).all() and res.commit_counts.sum() > 0
    check_against_numpy(res, 400, [(None, None), (1, 1), (3, 20), (1, 2 * ref.LDS_BINS + 1), (2 ** 32 - 1, None)])
    check_against_numpy(res, 400, [(None, None)], since=137)
    sim.close()


def test_grid_with_partitions_equals_numpy(grid_batch):
    sim, res, sets, set_of = grid_batch
    mc = 1000
    since = [0 if ps.partition is None else min(ps.partition[2], mc) for ps in sets]
    assert sorted(set(since)) == [0, 50, 250, 600, 1000]
    assert (res.stall_histogram("partition_end")[1] == res.stall_histogram(since)[1]).all()
    assert (res.stall_histogram("partition_end")[0] == res.stall_histogram(since)[0]).all()
    fam, _, hist, stats = check_against_numpy(res, mc, [(1, 1), (9, 30), (1, ref.LDS_BINS + 1), (None, None)], set_of, len(sets), since)
    # (a different `since` per group reaches the kernel: the partition sets' recovery differs from their time to the first commit)
    assert (res.stall_histogram()[1][:, 4:8] != stats[:, 4:8]).any()
    from librabft_simulator_amd.simulator import histogram_quantile
    qs = (0.0, 0.5, 0.9, 0.99, 1.0)
    rows = res.stalls_by_param_set("partition_end", qs)
    assert len(rows) == len(sets)
    for g, row in enumerate(rows):
        assert row["set"] == g and row["since"] == since[g]
        for f, (name, count) in enumerate((("gaps", "samples"), ("first", "nodes"), ("tail", "nodes"), ("longest", "nodes"))):
            s = fam[g][f]
            if not len(s):
                assert row[name][count] == 0 and row[name]["mean"] is None and row[name]["min"] is None and row[name]["max"] is None
                continue
            assert row[name][count] == len(s) and row[name]["min"] == s.min() and row[name]["max"] == s.max(), (g, name)
            assert row[name]["mean"] == pytest.approx(s.mean(), rel=1e-12)
        for q in qs:
            want = int(np.quantile(fam[g][ref.GAPS], q, method="inverted_cdf")) if len(fam[g][ref.GAPS]) else None
            assert row["gaps"]["quantiles"][str(q)] == want == histogram_quantile(hist[g], 1, q), (g, q)
    clean = res.faults == 0
    assert all(rows[g]["longest"]["nodes"] == 4 * int((clean & (set_of == g)).sum()) for g in range(len(sets)))


def test_groups_of_uneven_size_and_an_empty_one(amd):
    """Three-node networks in six sets of 1, 0, 7, 300, 13 and 0 instances, shuffled over the batch: row counts that fill no workgroup
    step, a group that spans several workgroups, empty groups (the last one too)."""
    rng = np.random.default_rng(6)
    sizes = np.array([1, 0, 7, 300, 13, 0])
    set_of = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.uint32)
    sets = [amd.ParamSet(amd.RandomDelay.new(float(5 + 3 * k), 4.0), amd.NodeConfig(100000, 10 + 5 * k, 2.0, 0.5),
                         partition=(1, 100, 200) if k % 2 else None) for k in range(len(sizes))]
    sim = amd.BatchSimulator.with_param_sets(np.arange(1, len(set_of) + 1, dtype=np.uint64), 3, sets, set_of, quirks=3, commit_times=True)
    res = sim.loop_until(500)
    assert (res.faults == 0).all()
    since = [0, 200, 0, 200, 0, 200]
    _, series, hist, stats = check_against_numpy(res, 500, [(None, None), (1, 1), (6, 20)], set_of, len(sizes), since)
    assert (res.stall_histogram("partition_end", 6, 20)[1] == stats).all()
    assert not series[sizes == 0].any() and not hist[sizes == 0].any() and not stats[sizes == 0].any()
    assert (stats[:, 12] == 3 * sizes).all()  # one `longest` sample per node
    rows = res.stalls_by_param_set("partition_end")
    assert rows[1]["gaps"] == {"samples": 0, "mean": None, "min": None, "max": None, "quantiles": {"0.5": None, "0.9": None, "0.99": None}}
    assert rows[5]["longest"] == {"nodes": 0, "mean": None, "min": None, "max": None}
    sim.close()


def test_gaps_past_the_first_lds_pass(amd):
    """A slow 4-node network to clock 100 000 (default width 2): gaps and commit times of tens of thousands of ticks, binned in later
    passes of the LDS histogram and in overflow bins there."""
    sim = amd.BatchSimulator.new(np.arange(1, 513, dtype=np.uint64), 4, amd.RandomDelay.new(float(2 ** 12), float(2 ** 22)),
                                 amd.NodeConfig(2 ** 16, 2 ** 13), commit_times=True)
    res = sim.loop_until(100000)
    assert (res.faults == 0).all()
    fam, _, hist, _ = check_against_numpy(res, 100000, [(None, None), (1, 100001), (1, 8191), (1, 8193), (3, 16385), (1, 65536), (4096, 30),
                                                      (2 ** 32 - 1, 3), (1, 2 * ref.LDS_BINS)])
    assert hist.shape[1] == 2 * ref.LDS_BINS and hist[0, ref.LDS_BINS:].sum() > 0, fam[0][ref.GAPS].max()  # gaps binned in the second pass
    assert res.commit_series(1, ref.LDS_BINS + 1)[0, -1] > 0  # an overflow bin in the second pass
    assert res.commit_series().shape == (1, 50001)
    sim.close()


def test_oracle_scenario_end_to_end(amd, oracle):
    """Control and partition (2, 300, 600), quirks = 3, seeds 1..32, clock 1500: the device's series and stalls equal the reference computed
    on commit times DERIVED FROM THE ORACLE, and show the stall and the recovery."""
    sc = ref.SCENARIO
    ct, counts, set_of, seeds = ref.scenario_oracle(oracle, HOST_THREADS)
    d = amd.RandomDelay.new(sc["mean"], sc["variance"])
    sets = [amd.ParamSet(d, amd.NodeConfig()), amd.ParamSet(d, amd.NodeConfig(), partition=sc["partition"])]
    sim = amd.BatchSimulator.with_param_sets(seeds, sc["nodes"], sets, set_of, quirks=sc["quirks"], commit_times=True)
    mc, end = sc["max_clock"], sc["partition"][2]
    res = sim.loop_until(mc)
    assert (res.faults == 0).all() and (res.commit_counts == counts).all()
    for width, bins in ((20, None), (1, None), (50, 10)):
        w, b = binning(mc, width, bins)
        series = res.commit_series(width, bins)
        assert (series == ref.series(ct, counts, None, set_of, 2, w, b)).all(), (width, bins)
        for since in (None, [0, end], "partition_end"):
            hist, stats = res.stall_histogram(since, width, bins)
            want = ref.stalls(ct, counts, None, set_of, 2, None if since is None else [0, end], w, b, mc)
            assert (hist == want[0]).all() and (stats == want[1]).all(), (width, bins, since)
    ref.check_scenario(res.commit_series(20), 20, res.stall_histogram("partition_end")[1])
    rows = res.stalls_by_param_set("partition_end")
    assert rows[1]["first"]["nodes"] == 128 and rows[1]["longest"]["min"] >= ref.SCENARIO_STALL > rows[0]["longest"]["max"]
    print("scenario: control longest %s, partition longest %s, recovery %s" % (rows[0]["longest"], rows[1]["longest"], rows[1]["first"]))
    sim.close()


def test_faulted_instances_are_skipped(amd):
    """A log capacity near the median commit count: some instances, not all, raise LBFT_FAULT_LOG_OVERFLOW; they give no sample."""
    seeds = np.arange(1, 257, dtype=np.uint64)
    probe = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0))
    cap = int(np.median(probe.loop_until(1000).commit_counts.max(axis=1)))
    probe.close()
    sim = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0), log_capacity=cap, commit_times=True)
    res = sim.loop_until(1000, allow_faults=True)
    faulted = res.faults != 0
    assert 0 < faulted.sum() < len(seeds), faulted.sum()
    assert (res.faults[faulted] & LOG_OVERFLOW).all()
    fam, series, _, stats = check_against_numpy(res, 1000, [(None, None), (10, 20)])
    clean = int((~faulted).sum())
    assert stats[0, 8] == stats[0, 12] == 4 * clean  # one tail and one longest sample per node of the clean instances
    unmasked = ref.series(res.commit_times(), res.commit_counts, None, None, 1, 10, 20)
    assert unmasked.sum() > series.sum()  # (the faulted instances do hold entries: the rule matters)
    sim.close()


def run_in_steps(sim, max_clock, steps=60):
    for _ in range(10000):
        left, res = sim.run_steps(max_clock, steps)
        if left == 0:
            return res
    raise AssertionError("the stepped run did not finish")


def timelines(res, since=None):
    return [res.commit_series(), res.commit_series(7, 50)] + list(res.stall_histogram(since)) + list(res.stall_histogram(since, 3, 40))


def test_calls_are_reproducible_and_follow_the_batch_state(amd, tmp_path):
    from librabft_simulator_amd import _lib
    seeds = np.arange(1, 1025, dtype=np.uint64)
    mk = lambda **kw: amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.uniform(3, 17), partition=(2, 200, 350), quirks=3, **kw)  # noqa: E731
    straight = mk(commit_times=True)
    # before a run: LBFT_ERR_STATE, from both calls
    for call in (lambda r: r.commit_series(), lambda r: r.stall_histogram()):
        with pytest.raises(amd.LbftError) as e:
            call(amd.BatchResult(straight))
        assert e.value.code == _lib.LBFT_ERR_STATE
    rs = straight.loop_until(800)
    want = timelines(rs, "partition_end")
    check_against_numpy(rs, 800, [(None, None), (3, 40)], since=350)
    assert all((a == b).all() for a, b in zip(want, timelines(rs, 350)))  # "partition_end" of a plain batch is the batch's
    assert all((a == b).all() for a, b in zip(want, timelines(rs, "partition_end")))  # two calls: identical arrays
    # a since outside [0, max_clock] at the C ABI: LBFT_ERR_INVALID, nothing written
    hist, stats = np.full(801, 7, dtype=np.uint64), np.full(16, 7, dtype=np.uint64)
    for bad in (-1, 801, 2 ** 40):
        since = np.array([bad], dtype=np.int64)
        rc = _lib.lib().lbft_batch_commit_stalls(straight._h, since.ctypes.data, 1, 801, hist.ctypes.data, stats.ctypes.data)
        assert rc == _lib.LBFT_ERR_INVALID and (hist == 7).all() and (stats == 7).all(), bad
    assert _lib.lib().lbft_batch_commit_series(straight._h, 1, 2 ** 31 + 1, hist.ctypes.data) == _lib.LBFT_ERR_INVALID  # groups x bins > 2^31
    # a run split by run_steps, and one resumed from a checkpoint, give the straight run's arrays
    a = mk(commit_times=True)
    left, _ = a.run_steps(800, 60)
    assert left > 0
    with pytest.raises(amd.LbftError) as e:  # (an unfinished run is no finished run)
        amd.BatchResult(a).commit_series()
    assert e.value.code == _lib.LBFT_ERR_STATE
    a.save_checkpoint(str(tmp_path / "ck.bin"))
    b = mk(commit_times=True)
    b.load_checkpoint(str(tmp_path / "ck.bin"))
    for sim in (a, b):
        got = timelines(run_in_steps(sim, 800), "partition_end")
        assert all((x == y).all() for x, y in zip(want, got))
    # a batch that does not record commit times: LBFT_ERR_STATE
    untimed = mk()
    ru = untimed.loop_until(800)
    for call in (lambda r: r.commit_series(), lambda r: r.stall_histogram(), lambda r: r.stalls_by_param_set()):
        with pytest.raises(amd.LbftError) as e:
            call(ru)
        assert e.value.code == _lib.LBFT_ERR_STATE
    # reset() and a second run to another horizon: that horizon's timelines (the log capacity and max_clock change)
    for mc in (1500, 200):
        straight.reset()
        r2 = straight.loop_until(mc)
        assert r2.commit_series().shape == (1, mc + 1)
        _, _, _, stats = check_against_numpy(r2, mc, [(None, None), (11, 9)], since=min(350, mc))
        fresh = mk(commit_times=True)
        assert all((x == y).all() for x, y in zip(timelines(r2, "partition_end"), timelines(fresh.loop_until(mc), "partition_end")))
        fresh.close()
    for s in (straight, a, b, untimed):
        s.close()


def test_grid_cli_stalls_and_series(amd):
    args = ["--nodes", "4", "--mean", "5,10", "--seeds-per-point", "32", "--max-clock", "1000", "--assign", "interleaved"]
    new = ["--stalls", "--partition", "none,2:300:600", "--series", "50"]
    out = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid"] + new + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.strip()]
    assert [(l["mean"], l["partition"]) for l in lines] == [(5.0, None), (5.0, [2, 300, 600]), (10.0, None), (10.0, [2, 300, 600])]
    plain = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr[-2000:]
    plain_lines = [json.loads(l) for l in plain.stdout.splitlines() if l.strip()]
    assert len(plain_lines) == 2 and all(not {"partition", "stalls", "series", "latency"} & set(l) for l in plain_lines)
    strip = lambda l: {k: v for k, v in l.items() if k not in ("partition", "stalls", "series")}  # noqa: E731
    assert [strip(l) for l in lines[0::2]] == plain_lines  # the points without a partition are the plain grid's
    from librabft_simulator_amd import grid
    sets = [amd.ParamSet(amd.RandomDelay.new(m, 4.0), amd.NodeConfig(100000, 20, 2.0, 0.5), partition=p) for m in (5.0, 10.0)
            for p in (None, (2, 300, 600))]
    set_of, seed_index = grid.set_assignment(4, 32, "interleaved")
    sim = amd.BatchSimulator.with_param_sets((1 + seed_index).astype(np.uint64), 4, sets, set_of, commit_times=True)
    res = sim.loop_until(1000, allow_faults=True)
    assert [l["stalls"] for l in lines] == json.loads(json.dumps(res.stalls_by_param_set("partition_end")))
    assert [l["series"] for l in lines] == res.commit_series(bin_width=50).tolist()
    assert [l["stalls"]["since"] for l in lines] == [0, 600, 0, 600] and all(len(l["series"]) == 21 for l in lines)
    sim.close()


def median_ms(fn, calls=7):
    ms = []
    for _ in range(calls + 1):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms[1:]))  # (the first call is dropped: warm)


def test_device_calls_do_not_take_longer_than_the_read_back(big, grid_batch):
    """(a) commit_series + stall_histogram against (b) commit_times() alone, the read-back they replace (without any numpy on it): warm,
    median of 7, in one process.  No margin: the read-back moves over PCIe at least what the kernel reads once from HBM."""
    for name, res in (("65536x4", big[1]), ("64-point grid x 1024", grid_batch[1])):
        cap = max(int(res.commit_counts.max()), 1)
        a = median_ms(lambda: (res.commit_series(), res.stall_histogram()))
        b = median_ms(lambda: res.commit_times(cap), calls=5)
        print("%s: (a) series + stalls %.3f ms, (b) commit_times() %.3f ms" % (name, a, b))
        assert a <= b, (name, a, b)
