"""Epoch statistics on the device (BatchResult.epoch_stats / epochs_by_param_set, lbft_k_ps_epochs) against the oracle: in every case the
device's three arrays equal the definitions restated over the ORACLE's node images, record hashes, commit counts, startup times and
epochs (tests/epoch_stats_reference.py), for the default binning and for (7, 5) -- fault words come from the device only where a case
provokes a capacity fault.  The cases are those of the host test as plain batches (every kernel class, two node rounds, boundaries at
and around the chunk edge, a segment over three chunks, no chain at all, more than 256 epochs), a parameter-set batch of unequal sets,
a handover histogram of two LDS passes, a batch with faulted instances, one with more instances than the grid has wavefronts, sums of
times past 2^32, and the lifecycle: reset, steps, checkpoint, timed and traced batches, a node-level session.  On every result the
identities of include/lbft.h hold."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_cases
import epoch_stats_cases as cases
import epoch_stats_reference as ref
from support import amd, device_batch, oracle_cfg, plain, same  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
BINNINGS = ((None, None), (7, 5))
CPE5 = dict(cases.Q3, commands_per_epoch=5)


def check(res, instances, max_clock, epoch_bins=64, binnings=BINNINGS, **groups):
    """epoch_stats() for every binning equals the reference on the oracle's instances, and the identities hold.  Returns the last arrays."""
    clean = res.faults == 0
    set_of, n_groups = groups.get("set_of"), groups.get("groups", 1)
    member = lambda g: clean & ((set_of == g) if set_of is not None else True)
    longest = res.commit_counts.max(axis=1)
    lengths = [int(longest[member(g)].sum()) for g in range(n_groups)]
    with_chain = [int((longest[member(g)] > 0).sum()) for g in range(n_groups)]
    for width, bins in binnings:
        got = res.epoch_stats(width, bins, epoch_bins)
        want = cases.expected(instances, max_clock, epoch_bins, width, bins, **groups)
        print("binning (%s, %s): stats %s table %s" % (width, bins, got[2].tolist(), got[1][:, :8].tolist()))
        for name, a, b in zip(("handover_hist", "epoch_table", "stats"), got, want):
            assert a.dtype == np.uint64 and a.shape == b.shape and (a == b).all(), (name, width, bins, a.tolist(), b.tolist())
        ref.identities(*got, lengths_sum=lengths, with_chain=with_chain)
    return got


def arrays(res):
    return list(res.epoch_stats()) + list(res.epoch_stats(7, 5, 3))


def fam(stats, f, g=0):
    return [int(v) for v in stats[g, 4 * f:4 * f + 4]]


# ---- the host cases as plain batches ----
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_host_cases_as_plain_batches(amd, oracle, name):
    kw, max_clock, seeds, epoch_bins = cases.CASES[name]
    sim = device_batch(amd, kw, seeds)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    instances = cases.case_instances(oracle, name)
    hist, table, stats = check(res, instances, max_clock, epoch_bins)
    assert res.epochs.tolist() == [i["node_epochs"] for i in instances]
    row = res.epochs_by_param_set(epoch_bins)[0]
    if name == "n4_default":  # one open segment per instance, no boundary, nothing stranded
        assert row["handover_cost"] is None and row["stranded_per_epoch"] is None and row["behind_share"] == 0.0 and len(row["per_epoch"]) == 1
        assert row["handover"] == {"boundaries": 0, "mean": None, "min": None, "max": None, "quantiles": {"0.5": None, "0.9": None, "0.99": None}}
    if name == "n4_cpe5_q3":  # the README's figures
        assert row["stranded"]["mean"] == 16.5 and row["stranded_per_epoch"] == pytest.approx(66 / 19) and row["handover"]["quantiles"]["0.5"] is not None
        assert row["handover_cost"] == pytest.approx(1436 / 19 - 2071 / (95 - 19)) and [e["entries"] for e in row["per_epoch"]] == [20, 20, 20, 20, 20, 3]
    if name == "n4_cpe50_q0":  # the stall after the first epoch change
        assert row["behind_share"] == 0.5 and row["behind"]["max"] == 1 and row["segments"]["max"] == 1 and row["length"]["segments"] == 0
        assert sorted(res.epochs[0].tolist()) == [0, 0, 1, 1]
    if name == "n4_empty_chain":
        assert not res.commit_counts.any() and fam(stats, ref.SEGMENTS) == [3, 0, 0, 0] and not hist.any() and table[0, 0].tolist() == [0, 0, 0, 0, 0, 0, 3]
    if name == "n65_cpe4_q3":
        assert sim.layout()["kernel_class"] & 0xff == 2 and fam(stats, ref.NODE_EPOCH)[0] == 130
    if name == "n4_cpe1_q3_above_256_epochs":
        assert table[0, 256:, ref.COL_HANDOVER].sum() > 0 and table[0, 300, ref.COL_SEGMENTS] == 1 and row["handover"]["quantiles"] is None
    sim.close()


# ---- parameter sets of unequal size ----
def test_parameter_sets_of_1_5_and_10_instances(amd, oracle):
    n, max_clock = 4, 600
    sets = [amd.ParamSet(), amd.ParamSet(amd.RandomDelay.new(20.0, 9.0)), amd.ParamSet(drop_per_million=20000)]
    set_of = np.array([1, 2, 2, 1, 0, 2, 2, 1, 2, 2, 1, 2, 2, 1, 2, 2], dtype=np.uint32)
    assert [(set_of == k).sum() for k in range(3)] == [1, 5, 10]
    seeds = np.arange(1, len(set_of) + 1, dtype=np.uint64)
    instances = []
    for i, seed in enumerate(seeds):
        o = oracle.OracleSim(oracle_cfg(oracle, n, sets[set_of[i]], quirks=3, commands_per_epoch=5), int(seed)).run_until(max_clock)
        instances.append(ref.instance(o, n))
        o.close()
    sim = amd.BatchSimulator.with_param_sets(seeds, n, sets, set_of, quirks=3, commands_per_epoch=5)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    hist, table, stats = check(res, instances, max_clock, set_of=set_of, groups=3)
    assert stats[:, 4 * ref.BLOCKS].tolist() == [1, 5, 10] and stats[:, 4 * ref.NODE_EPOCH].tolist() == [4, 20, 40] and (stats[:, 4 * ref.HANDOVER] > 0).all()
    rows = res.epochs_by_param_set()
    assert [r["set"] for r in rows] == [0, 1, 2]
    hist1, table1, stats1 = res.epoch_stats()
    for g, row in enumerate(rows):
        assert row["blocks"]["instances"] == (set_of == g).sum() and row["handover"]["boundaries"] == int(stats1[g, 4 * ref.HANDOVER])
        complete = int(stats1[g, 4 * ref.LENGTH])
        assert row["stranded_per_epoch"] == pytest.approx(int(stats1[g, 4 * ref.STRANDED + 1]) / complete)
        inner = int(stats1[g, 4 * ref.DURATION + 1]) / (int(stats1[g, 4 * ref.LENGTH + 1]) - complete)
        assert row["handover_cost"] == pytest.approx(int(stats1[g, 4 * ref.HANDOVER + 1]) / int(stats1[g, 4 * ref.HANDOVER]) - inner)
        assert [e["entries"] for e in row["per_epoch"]] == [int(v) for v in table1[g, :len(row["per_epoch"]), ref.COL_ENTRIES]]
        assert table1[g, len(row["per_epoch"]):].sum() == 0 and row["behind_share"] is not None
    sim.close()


# ---- a handover histogram wider than the LDS holds ----
def test_handover_histogram_in_two_lds_passes(amd, oracle):
    """Width 1 at clock 5000: 5 001 bins are two passes of 4 096, and the run's eight handovers all lie in the first.  Then a run whose
    second pass holds samples too: two of four nodes cut off during [1000, 5400) hold the chain at an epoch boundary, one handover of
    about 4 500 ticks per instance (the oracle: 4 of 88, the largest 4 546)."""
    name = "n4_cpe70_q3"
    kw, max_clock, seeds, _ = cases.CASES[name]
    sim = device_batch(amd, kw, seeds)
    res = sim.loop_until(max_clock)
    hist, _, stats = check(res, cases.case_instances(oracle, name), max_clock, binnings=((None, None), (1, 5001)))
    assert res.epoch_stats()[0].shape[1] == 2501 and hist.shape[1] == 5001 and hist.sum() == fam(stats, ref.HANDOVER)[0] == 8
    sim.close()
    kw = dict(cases.Q3, commands_per_epoch=1, partition_size=2, partition_start=1000, partition_end=5400)
    instances = cases.oracle_instances(oracle, kw, 6000, cases.SEEDS)
    sim = device_batch(amd, kw, cases.SEEDS)
    res = sim.loop_until(6000)
    assert (res.faults == 0).all()
    hist, _, stats = check(res, instances, 6000, epoch_bins=512, binnings=((1, 6001),))
    print("handovers beyond 4096 ticks:", int(hist[0, 4096:].sum()), "largest", fam(stats, ref.HANDOVER)[3])
    assert hist[0, 4096:].sum() == 4 and fam(stats, ref.HANDOVER) == [88, 23590, 54, 4546]
    sim.close()


# ---- instances faulted by a small block capacity ----
def test_faulted_instances_are_skipped_and_the_others_equal_the_oracle(amd, oracle):
    kw, max_clock, seeds = CPE5, 1000, range(1, 131)
    probe = device_batch(amd, kw, seeds)
    high = probe.loop_until(max_clock).counters["max_blocks"]
    probe.close()
    sim = device_batch(amd, kw, seeds, block_capacity=high - 1)
    res = sim.loop_until(max_clock, allow_faults=True)
    faulted = res.faults != 0
    print("max_blocks %d, faulted instances %s" % (high, np.nonzero(faulted)[0].tolist()))
    assert 1 <= faulted.sum() < len(faulted) // 2
    _, _, stats = check(res, cases.oracle_instances(oracle, kw, max_clock, seeds), max_clock, faults=res.faults)
    assert stats[0, 4 * ref.BLOCKS] == (~faulted).sum() and stats[0, 4 * ref.NODE_EPOCH] == 4 * (~faulted).sum()
    sim.close()


# ---- more instances than the grid has wavefronts ----
def test_4102_networks_where_a_wavefront_takes_a_second_instance(amd, oracle):
    kw, max_clock, seeds = CPE5, 300, range(1, 4103)
    sim = device_batch(amd, kw, seeds)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    _, _, stats = check(res, cases.oracle_instances(oracle, kw, max_clock, seeds), max_clock, binnings=((None, None),))
    assert stats[0, 4 * ref.BLOCKS] == 4102 and stats[0, 4 * ref.HANDOVER] > 0
    sim.close()


# ---- sums of times past 2^32 ----
def test_duration_and_handover_sums_past_2_to_the_32(amd, oracle):
    """The slow network of the long-horizon edge cases (mean delay 2^24, run to the top of the clock range) with an epoch every 5 commands:
    eight instances sum both the durations and the handovers past 2^32 (the oracle: 8 275 832 660 and 6 916 999 120)."""
    kw, max_clock, seeds = dict(CPE5, **edge_cases.SLOW), edge_cases.MAX_CLOCK_LIMIT, range(1, 9)
    instances = cases.oracle_instances(oracle, kw, max_clock, seeds)
    sim = device_batch(amd, kw, seeds)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    hist, table, stats = check(res, instances, max_clock)
    assert fam(stats, ref.DURATION)[1] == 8275832660 > 1 << 32 and fam(stats, ref.HANDOVER)[1] == 6916999120 > 1 << 32
    assert table[0, :, ref.COL_DURATION].sum() == 8275832660 and table[0, :, ref.COL_HANDOVER].sum() == 6916999120
    assert res.epoch_stats()[0].shape[1] == 4096
    sim.close()


# ---- timed and traced batches ----
def test_timed_and_traced_batches_give_the_plain_batch_statistics(amd, oracle):
    kw, max_clock, seeds, _ = cases.CASES["n4_cpe5_q3"]
    base = device_batch(amd, kw, seeds)
    mine = arrays(base.loop_until(max_clock))
    timed = device_batch(amd, kw, seeds, commit_times=True)
    rt = timed.loop_until(max_clock)
    check(rt, cases.case_instances(oracle, "n4_cpe5_q3"), max_clock)
    assert timed.layout()["kernel_class"] & (1 << 17) and same(mine, arrays(rt))
    traced = device_batch(amd, kw, seeds)
    assert same(mine, arrays(traced.loop_until(max_clock, round_trace=256)))
    for s in (base, timed, traced):
        s.close()


# ---- lifecycle: reset, steps, checkpoint, a node-level session ----
def test_reset_steps_checkpoint_and_manual_sessions(amd, oracle, tmp_path):
    from librabft_simulator_amd import _lib
    kw, max_clock, seeds, _ = cases.CASES["n4_cpe5_q3"]
    sim = device_batch(amd, kw, seeds)
    for call in (lambda r: r.epoch_stats(), lambda r: r.epochs_by_param_set()):  # before the run
        with pytest.raises(amd.LbftError) as e:
            call(amd.BatchResult(sim))
        assert e.value.code == _lib.LBFT_ERR_STATE
    res = sim.loop_until(max_clock)
    check(res, cases.case_instances(oracle, "n4_cpe5_q3"), max_clock)
    want = arrays(res)
    counts, epochs = res.commit_counts.copy(), res.epochs.copy()
    assert same(want, arrays(res)) and (res.commit_counts == counts).all() and (amd.BatchResult(sim).epochs == epochs).all()  # no state changes
    sim.reset()
    with pytest.raises(amd.LbftError) as e:  # between reset() and the next run
        amd.BatchResult(sim).epoch_stats()
    assert e.value.code == _lib.LBFT_ERR_STATE
    assert same(want, arrays(sim.loop_until(max_clock)))
    sim.close()
    a = device_batch(amd, kw, seeds)
    left, _ = a.run_steps(max_clock, 150)
    assert left > 0
    with pytest.raises(amd.LbftError) as e:  # (an unfinished run is no finished run)
        amd.BatchResult(a).epoch_stats()
    assert e.value.code == _lib.LBFT_ERR_STATE
    a.save_checkpoint(str(tmp_path / "ck.bin"))
    a.close()
    b = device_batch(amd, kw, seeds)
    b.load_checkpoint(str(tmp_path / "ck.bin"))
    done = None
    for _ in range(10000):
        left, done = b.run_steps(max_clock, 150)
        if left == 0:
            break
    assert done is not None and same(want, arrays(done))
    b.close()
    # a node-level session: legal after manual_finalize, as lbft_batch_commit_counts is; nothing was proposed
    c = device_batch(amd, kw, list(seeds)[:2])
    c.manual(max_clock)
    with pytest.raises(amd.LbftError) as e:
        amd.BatchResult(c).epoch_stats()
    assert e.value.code == _lib.LBFT_ERR_STATE
    hist, table, stats = c.manual_finalize().epoch_stats()
    assert not hist.any() and not table[0, 1:].any() and table[0, 0, :6].tolist() == [0] * 6
    assert stats[0, 0::4].tolist() == [2, 8, 8, 0, 0, 0, 0, 0, 2, 2] and not stats[0, 4 * ref.SEGMENTS + 1] and not stats[0, 4 * ref.STRANDED + 1]
    c.close()


# ---- refusals ----
def test_refusals(amd):
    from librabft_simulator_amd import _lib
    sim = device_batch(amd, CPE5, range(1, 5))
    L = _lib.lib()
    outs = [np.full(k, 7, dtype=np.uint64) for k in (8, 7 * 8, 40)]
    p = [a.ctypes.data for a in outs]
    assert L.lbft_batch_epoch_stats(sim._h, 1, 0, 8, *p) == _lib.LBFT_ERR_INVALID  # the binning before the state
    assert L.lbft_batch_epoch_stats(sim._h, 1, 8, 0, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_epoch_stats(sim._h, 1, 8, 513, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_epoch_stats(sim._h, 1, 8, 8, *p) == _lib.LBFT_ERR_STATE
    res = sim.loop_until(400)
    assert L.lbft_batch_epoch_stats(sim._h, 1, 0, 8, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_epoch_stats(sim._h, 0, 8, 8, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_epoch_stats(sim._h, 1, 8, 0, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_epoch_stats(sim._h, 1, 8, 513, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_epoch_stats(sim._h, 1, 2 ** 31 + 1, 8, *p) == _lib.LBFT_ERR_INVALID  # groups x bins > 2^31
    for k in range(3):
        q = list(p)
        q[k] = None
        assert L.lbft_batch_epoch_stats(sim._h, 1, 8, 8, *q) == _lib.LBFT_ERR_INVALID
    assert all((a == 7).all() for a in outs)
    assert L.lbft_batch_epoch_stats(sim._h, 1, 8, 8, *p) == _lib.LBFT_OK
    hist, table, stats = outs
    assert hist.sum() == stats[4 * ref.HANDOVER] > 0 and table[ref.COL_BLOCKS::7].sum() == stats[4 * ref.BLOCKS + 1] and stats[4 * ref.BLOCKS] == 4
    with pytest.raises(ValueError):
        res.epoch_stats(epoch_bins=513)
    assert res.epoch_stats(epoch_bins=512)[1].shape == (1, 512, 7) and res.epoch_stats(epoch_bins=1)[1].shape == (1, 1, 7)
    sim.close()


# ---- the grid tool ----
def test_grid_cli_epochs(amd):
    args = ["--nodes", "4", "--delta", "10,20", "--seeds-per-point", "8", "--max-clock", "300", "--assign", "interleaved", "--commands-per-epoch", "5"]
    out = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid", "--epochs"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.strip()]
    assert [l["delta"] for l in lines] == [10, 20]
    from librabft_simulator_amd import grid
    sets = [amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, d, 2.0, 0.5)) for d in (10, 20)]
    set_of, seed_index = grid.set_assignment(2, 8, "interleaved")
    sim = amd.BatchSimulator.with_param_sets((1 + seed_index).astype(np.uint64), 4, sets, set_of, commands_per_epoch=5)
    res = sim.loop_until(300, allow_faults=True)
    for l in lines:
        assert set(l["epochs"]) == {"set", "handover_cost", "stranded_per_epoch", "behind_share", "per_epoch", *ref.FAMILIES} and l["faulted"] == 0
        assert l["epochs"]["blocks"]["instances"] == 8 and l["epochs"]["node_epoch"]["nodes"] == 32
    assert [l["epochs"] for l in lines] == json.loads(json.dumps(res.epochs_by_param_set()))
    sim.close()
