"""Commit times and commit latency on the device (lbft_batch_record_commit_times, liblbft_commit_times.so): the recorded times equal the ones
derived from fresh oracle runs (tests/commit_times_oracle.py) on both kernel classes and on a parameter-set batch, agree with fresh device
runs to intermediate horizons over a whole 65 536-network batch, leave every other result of the batch as it is, survive run_steps and
checkpoints; the device histogram equals numpy's, bit for bit; and the refusals hold."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import commit_times_oracle as cto  # noqa: E402

pytestmark = pytest.mark.gpu
HOST_THREADS = min(os.cpu_count() or 8, 16)
BIG = 65536


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import librabft_simulator_amd as L
    L.lib()
    return L


def layout_flags(sim):
    from librabft_simulator_amd import _lib
    out = np.zeros(8, dtype=np.uint32)
    assert _lib.lib().lbft_batch_layout(sim._h, out.ctypes.data) == 0
    return int(out[7])


def oracle_cfg(oc, n, delay, node_config, **kw):
    return oc.make_config(num_nodes=n, mean=delay.mean, variance=delay.variance, delay_model=delay.model, uniform_lo=delay.lo, uniform_hi=delay.hi,
                          target_commit_interval=node_config.target_commit_interval, delta=node_config.delta, gamma=node_config.gamma,
                          lambda_=node_config.lambda_, math_mode=1, **kw)


def ps_oracle_cfg(oc, n, ps):
    part = ps.partition or (0, 0, 0)
    return oracle_cfg(oc, n, ps.network_delay, ps.node_config, drop_per_million=ps.drop_per_million, partition_size=part[0],
                      partition_start=part[1], partition_end=part[2])


def small_sets(amd):
    return [amd.ParamSet(amd.RandomDelay.new(5.0, 2.5), amd.NodeConfig(100000, 10, 2.0, 0.5)),
            amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, 40, 2.0, 0.25)),
            amd.ParamSet(amd.RandomDelay.new(20.0, 10.0), amd.NodeConfig(40, 20, 1.5, 0.75)),
            amd.ParamSet(amd.RandomDelay.new(10.0, 0.0), amd.NodeConfig(100000, 20, 2.0, 0.5))]


def numpy_histogram(res, width, bins, set_of=None, groups=1):
    ct = res.commit_times()
    lat, inst = cto.latencies(ct, res.committed_histories(ct.shape[2]), res.startup_times, res.faults)
    g = np.zeros(len(lat), dtype=np.int64) if set_of is None else np.asarray(set_of, dtype=np.int64)[inst]
    hist = np.zeros((groups, bins), dtype=np.uint64)
    stats = np.zeros((groups, 4), dtype=np.uint64)
    binned = np.minimum(lat // width, bins - 1)
    for k in range(groups):
        sel = g == k
        hist[k] = np.bincount(binned[sel], minlength=bins)
        if sel.any():
            stats[k] = (sel.sum(), lat[sel].sum(), lat[sel].min(), lat[sel].max())
    return hist, stats, lat, g


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
    ref = cto.commit_times(oracle, oracle_cfg(oracle, 4, amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig()), seeds, 600, ct.shape[2], HOST_THREADS)
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
    ref = cto.commit_times(oracle, oracle_cfg(oracle, 16, amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(), drop_per_million=20000),
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
    ref = cto.param_set_commit_times(oracle, [ps_oracle_cfg(oracle, 4, ps) for ps in sets], set_of, seeds, 500, ct.shape[2], HOST_THREADS)
    assert (res.faults == 0).all()
    assert (ct == ref).all()
    sim.close()


def test_big_batch_sample_equals_the_oracle(amd, oracle, big):
    seeds, _, rt, _, _ = big
    ct = rt.commit_times()
    idx = np.arange(0, BIG, BIG // 256)
    ref = cto.commit_times(oracle, oracle_cfg(oracle, 4, amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig()), seeds[idx], 1000, ct.shape[2],
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


def _same_results(a, b):
    for name in ("commit_counts", "last_committed_states", "active_rounds", "startup_times", "faults", "epochs"):
        assert (getattr(a, name) == getattr(b, name)).all(), name
    cap = int(a.commit_counts.max())
    assert (a.committed_histories(cap) == b.committed_histories(cap)).all()
    ca, cb = a.counters, b.counters
    for name in ("events", "rng_draws", "rounds", "commits", "events_scheduled", "faulted_instances", "max_queue", "max_snapshots", "max_blocks"):
        assert ca[name] == cb[name], name


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
