"""Vote statistics on the device (BatchResult.vote_stats / votes_by_param_set, lbft_k_ps_votes) against the oracle: in every case the
device's four arrays equal the definitions restated over the ORACLE's node images, record hashes and commit counts
(tests/vote_stats_reference.py), for the default binning and for (7, 5) -- fault words come from the device only where a case provokes a
capacity fault.  The cases are those of the host test as plain batches (every kernel class, one to three voter words, two node rounds,
chains and pools beyond one chunk of 64, no chain at all), a parameter-set batch of unequal sets, a margin histogram of two LDS passes,
a batch with faulted instances, one with more instances than the grid has wavefronts, and the lifecycle: reset, steps, checkpoint,
timed and traced batches, a node-level session.  On every result the identities of include/lbft.h hold."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import vote_stats_cases as cases
import vote_stats_reference as ref
from support import amd, device_batch, oracle_cfg, plain, same  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
BINNINGS = ((None, None), (7, 5))


def check(res, instances, n, rights, binnings=BINNINGS, **groups):
    """vote_stats() for every binning equals the reference on the oracle's instances, and the identities hold.  Returns the last arrays."""
    clean = res.faults == 0
    set_of, n_groups = groups.get("set_of"), groups.get("groups", 1)
    lengths = [int(res.commit_counts.max(axis=1)[clean & ((set_of == g) if set_of is not None else True)].sum()) for g in range(n_groups)]
    for width, bins in binnings:
        got = res.vote_stats(width, bins)
        want = cases.expected(instances, n, rights, width, bins, **groups)
        print("binning (%s, %s): stats %s nodes %s" % (width, bins, got[3].tolist(), got[2].tolist()))
        for name, a, b in zip(("margin_hist", "votes_hist", "node_table", "stats"), got, want):
            assert a.dtype == np.uint64 and a.shape == b.shape and (a == b).all(), (name, width, bins, a.tolist(), b.tolist())
        ref.identities(*got, lengths_sum=lengths, unit=rights is None)
    return got


def arrays(res):
    return list(res.vote_stats()) + list(res.vote_stats(7, 5))


# ---- the host cases as plain batches ----
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_host_cases_as_plain_batches(amd, oracle, name):
    kw, max_clock, seeds = cases.CASES[name]
    sim = device_batch(amd, kw, seeds)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    margin, votes, nodes, stats = check(res, cases.case_instances(oracle, name), kw["num_nodes"], kw.get("voting_rights"))
    if name == "n4_empty_chain":
        assert not res.commit_counts.any() and stats[0, 4 * ref.PENDING + 1] == stats[0, 4 * ref.BLOCKS + 1] > 0 and not margin.any()
        row = res.votes_by_param_set()[0]
        assert row["round_utilisation"] is None and row["orphan_rate"] is None and row["nodes"][0]["participation"] is None
    if name == "n65_q3":
        assert sim.layout()["kernel_class"] & 0xff == 2 and nodes[0, 64, ref.VOTED] > 0
    if name == "n5_weighted":  # the figures of the README: node 0 is in every certificate
        row = res.votes_by_param_set()[0]
        assert row["nodes"][0]["participation"] == 1.0 and row["votes_hist"] == [0, 0, 0, 225, 30, 35]
        assert row["margin"]["quantiles"] == {"0.5": 0, "0.9": 2, "0.99": 2} and row["votes"]["entries"] == 290
        assert row["orphan_rate"] == pytest.approx(28 / (341 - 23)) and row["round_utilisation"] == pytest.approx(282 / (282 + 25))
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
        o = oracle.OracleSim(oracle_cfg(oracle, n, sets[set_of[i]]), int(seed)).run_until(max_clock)
        instances.append(ref.instance(o, n))
        o.close()
    sim = amd.BatchSimulator.with_param_sets(seeds, n, sets, set_of)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    margin, votes, nodes, stats = check(res, instances, n, None, set_of=set_of, groups=3)
    assert stats[:, 4 * ref.BLOCKS].tolist() == [1, 5, 10]
    rows = res.votes_by_param_set()
    assert [r["set"] for r in rows] == [0, 1, 2]
    for g, row in enumerate(rows):
        assert row["votes_hist"] == votes[g].tolist() and [c["voted"] for c in row["nodes"]] == nodes[g, :, ref.VOTED].tolist()
        assert row["blocks"]["instances"] == (set_of == g).sum() and row["margin"]["quantiles"] == {"0.5": 0, "0.9": 0, "0.99": 0}
        decided = int(stats[g, 4 * ref.BLOCKS + 1] - stats[g, 4 * ref.PENDING + 1])
        assert row["orphan_rate"] == pytest.approx(int(stats[g, 4 * ref.ORPHANED + 1]) / decided)
        assert all(c["participation"] == pytest.approx(c["voted"] / int(stats[g, 0])) for c in row["nodes"])
    sim.close()


# ---- a margin histogram wider than the LDS holds ----
@pytest.mark.parametrize("heavy,bins", [(5000, 5005), (20000, 6668)])
def test_margin_histogram_in_two_lds_passes(amd, oracle, heavy, bins):
    """Rights [heavy, 1, 1, 1, 1] at width 1: 5 005 bins are two passes of 4 096 whose second stays empty (the margins end at 1 667);
    with 20 000 the margins are 6 665 and more, so every sample is counted in the second pass.  The heavy node leads every round and
    a round takes one tick: a block per tick, which the automatic block capacity (a block per ten ticks) does not hold."""
    kw, max_clock, seeds = dict(num_nodes=5, voting_rights=[heavy, 1, 1, 1, 1]), 120, range(1, 9)
    instances = cases.oracle_instances(oracle, kw, max_clock, seeds)
    sim = device_batch(amd, kw, seeds, block_capacity=256)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    margin, _, _, stats = check(res, instances, 5, kw["voting_rights"], ((1, bins), (None, None), (7, 5)))
    total, quorum = heavy + 4, 2 * (heavy + 4) // 3 + 1
    assert res.vote_stats()[0].shape[1] == min(total - quorum + 1, 4096)
    exact = res.vote_stats(1, bins)[0]
    assert exact[0, 4096:].sum() == (stats[0, 4 * ref.MARGIN] if heavy == 20000 else 0) and exact.sum() == stats[0, 4 * ref.MARGIN] > 0
    assert (res.votes_by_param_set()[0]["margin"]["quantiles"] is None) == (heavy == 20000)
    sim.close()


# ---- instances faulted by a small queue capacity ----
def test_faulted_instances_are_skipped_and_the_others_equal_the_oracle(amd, oracle):
    kw, max_clock, seeds = dict(num_nodes=4), 1000, range(1, 131)
    probe = device_batch(amd, kw, seeds)
    high = probe.loop_until(max_clock).counters["max_queue"]
    probe.close()
    sim = device_batch(amd, kw, seeds, queue_capacity=high - 1)
    res = sim.loop_until(max_clock, allow_faults=True)
    faulted = res.faults != 0
    print("max_queue %d, faulted instances %s" % (high, np.nonzero(faulted)[0].tolist()))
    assert 1 <= faulted.sum() < len(faulted) // 2
    _, _, _, stats = check(res, cases.oracle_instances(oracle, kw, max_clock, seeds), 4, None, faults=res.faults)
    assert stats[0, 4 * ref.BLOCKS] == (~faulted).sum()
    sim.close()


# ---- more instances than the grid has wavefronts ----
def test_4102_networks_where_a_wavefront_takes_a_second_instance(amd, oracle):
    kw, max_clock, seeds = dict(num_nodes=4), 200, range(1, 4103)
    sim = device_batch(amd, kw, seeds)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    _, _, _, stats = check(res, cases.oracle_instances(oracle, kw, max_clock, seeds), 4, None)
    assert stats[0, 4 * ref.BLOCKS] == 4102
    sim.close()


# ---- timed and traced batches ----
def test_timed_and_traced_batches_give_the_plain_batch_statistics(amd, oracle):
    kw, max_clock, seeds = cases.CASES["n4"]
    base = device_batch(amd, kw, seeds)
    mine = arrays(base.loop_until(max_clock))
    timed = device_batch(amd, kw, seeds, commit_times=True)
    rt = timed.loop_until(max_clock)
    check(rt, cases.case_instances(oracle, "n4"), 4, None)
    assert timed.layout()["kernel_class"] & (1 << 17) and same(mine, arrays(rt))
    traced = device_batch(amd, kw, seeds)
    assert same(mine, arrays(traced.loop_until(max_clock, round_trace=256)))
    for s in (base, timed, traced):
        s.close()


# ---- lifecycle: reset, steps, checkpoint, a node-level session ----
def test_reset_steps_checkpoint_and_manual_sessions(amd, oracle, tmp_path):
    from librabft_simulator_amd import _lib
    kw, max_clock, seeds = cases.CASES["n4"]
    sim = device_batch(amd, kw, seeds)
    for call in (lambda r: r.vote_stats(), lambda r: r.votes_by_param_set()):  # before the run
        with pytest.raises(amd.LbftError) as e:
            call(amd.BatchResult(sim))
        assert e.value.code == _lib.LBFT_ERR_STATE
    res = sim.loop_until(max_clock)
    check(res, cases.case_instances(oracle, "n4"), 4, None)
    want = arrays(res)
    counts = res.commit_counts.copy()
    assert same(want, arrays(res)) and (res.commit_counts == counts).all()  # the call changes no state
    sim.reset()
    with pytest.raises(amd.LbftError) as e:  # between reset() and the next run
        amd.BatchResult(sim).vote_stats()
    assert e.value.code == _lib.LBFT_ERR_STATE
    assert same(want, arrays(sim.loop_until(max_clock)))
    sim.close()
    a = device_batch(amd, kw, seeds)
    left, _ = a.run_steps(max_clock, 150)
    assert left > 0
    with pytest.raises(amd.LbftError) as e:  # (an unfinished run is no finished run)
        amd.BatchResult(a).vote_stats()
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
        amd.BatchResult(c).vote_stats()
    assert e.value.code == _lib.LBFT_ERR_STATE
    margin, votes, nodes, stats = c.manual_finalize().vote_stats()
    assert not margin.any() and not votes.any() and not nodes.any()
    assert stats[0, 0::4].tolist() == [0, 0, 0, 0, 2, 2, 2, 2] and not stats[0, 1::4].any()
    c.close()


# ---- refusals ----
def test_refusals(amd):
    from librabft_simulator_amd import _lib
    sim = device_batch(amd, dict(num_nodes=4), range(1, 5))
    L = _lib.lib()
    outs = [np.full(k, 7, dtype=np.uint64) for k in (8, 5, 12, 32)]
    p = [a.ctypes.data for a in outs]
    assert L.lbft_batch_vote_stats(sim._h, 1, 0, *p) == _lib.LBFT_ERR_INVALID  # the binning before the state
    assert L.lbft_batch_vote_stats(sim._h, 1, 8, *p) == _lib.LBFT_ERR_STATE
    res = sim.loop_until(200)
    assert L.lbft_batch_vote_stats(sim._h, 1, 0, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_vote_stats(sim._h, 0, 8, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_vote_stats(sim._h, 1, 2 ** 31 + 1, *p) == _lib.LBFT_ERR_INVALID  # groups x bins > 2^31
    for k in range(4):
        q = list(p)
        q[k] = None
        assert L.lbft_batch_vote_stats(sim._h, 1, 8, *q) == _lib.LBFT_ERR_INVALID
    assert all((a == 7).all() for a in outs)
    assert L.lbft_batch_vote_stats(sim._h, 1, 8, *p) == _lib.LBFT_OK
    margin, votes, nodes, stats = outs
    assert margin.sum() == votes.sum() == stats[0] > 0 and nodes[0::3].sum() == stats[4 * ref.BLOCKS + 1]
    with pytest.raises(ValueError):
        res.vote_stats(bins=0)
    sim.close()


# ---- the grid tool ----
def test_grid_cli_votes(amd):
    args = ["--nodes", "4", "--delta", "10,20", "--seeds-per-point", "8", "--max-clock", "300", "--assign", "interleaved"]
    out = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid", "--votes"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.strip()]
    assert [l["delta"] for l in lines] == [10, 20]
    from librabft_simulator_amd import grid
    sets = [amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, d, 2.0, 0.5)) for d in (10, 20)]
    set_of, seed_index = grid.set_assignment(2, 8, "interleaved")
    sim = amd.BatchSimulator.with_param_sets((1 + seed_index).astype(np.uint64), 4, sets, set_of)
    res = sim.loop_until(300, allow_faults=True)
    for l in lines:
        assert set(l["votes"]) == {"set", "votes_hist", "nodes", "orphan_rate", "round_utilisation", *ref.FAMILIES} and l["faulted"] == 0
        assert l["votes"]["blocks"]["instances"] == 8 and 0 < l["votes"]["round_utilisation"] <= 1
    assert [l["votes"] for l in lines] == json.loads(json.dumps(res.votes_by_param_set()))
    sim.close()
