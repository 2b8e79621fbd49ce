"""Commit finality on the device (BatchResult.finality_histogram / finality_by_param_set, lbft_k_ct_finality): in every case the device's
arrays equal the numpy reference of the definitions (tests/commit_finality_reference.py) evaluated on the batch's own read-backs --
commit_times(), committed_histories, startup_times, faults, commit_counts, which other tests hold against the oracle -- and once on commit
times derived from the oracle end to end.  The shapes are the smallest that reach each mechanism: chains of three 64-entry chunks, of
less than one and of none at all on instance-major class-0 rows, 64-wide tiles with a partial tile, 32 nodes (the tile's last row),
weighted and rotating rights, a partition, parameter sets with an unused set and instances that overflowed their logs, the binnings'
edges, repeated calls, reset, stepping and checkpoints, the refusals and the grid tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_stats_reference as chain_ref
import commit_finality_reference as ref
from support import amd, oracle_cfg, plain, run_to_end, same  # noqa: F401
from support import check_finality as check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
LOG_OVERFLOW = 1 << 3  # LBFT_FAULT_LOG_OVERFLOW


def arrays(res):
    return list(res.finality_histogram()) + list(res.finality_histogram(7, 30))


# ---- class 0, instance-major rows ----
SMALL = dict(n=4, seeds=np.arange(1, 97, dtype=np.uint64))


@pytest.mark.parametrize("max_clock", [4000, 300, 0, 20])
def test_class_0_chains_of_three_chunks_of_less_than_one_and_of_none(amd, max_clock):
    sim = plain(amd, SMALL["seeds"], SMALL["n"], amd.ParamSet(), commit_times=True)
    res = sim.loop_until(max_clock)
    assert sim.layout()["kernel_class"] & 0xff == 0 and (res.faults == 0).all()
    fam, fin, spread, first, stats = check(res, max_clock, [(None, None), (1, 2 * ref.LDS_BINS + 7), (7, 5), (1, 1)])
    f = fam[0]
    lengths = res.commit_counts.max(axis=1)
    if max_clock == 4000:  # three chunks of 64 entries
        assert lengths.min() > 128
        assert same(arrays(res), arrays(res))  # two calls: identical arrays
        clamp = res.finality_histogram(7, 5)
        assert clamp[0][0, -1] == (f[ref.QUORUM] >= 28).sum() > 0 and clamp[1][0, -1] == (f[ref.SPREAD] >= 28).sum()  # the last bin counts all above it
        assert (clamp[3] == res.finality_histogram()[3]).all()  # the binning leaves the statistics as they are
        assert len(f[ref.FIRST]) == lengths.sum() and 0 < len(f[ref.ALL]) <= len(f[ref.QUORUM])
    elif max_clock == 300:
        assert 0 < lengths.min() and lengths.max() < 64 and len(f[ref.QUORUM]) > 0
    else:  # no commit anywhere: every family is empty except `open`, with one zero sample per instance
        assert stats[0].tolist() == [0] * 20 + [96, 0, 0, 0]
        assert not fin.any() and not spread.any() and not first.any()
        row = res.finality_by_param_set()[0]
        assert row["first_share"] is None and row["quorum"]["mean"] is None and row["open"] == {"instances": 96, "mean": 0.0, "min": 0, "max": 0}
    sim.close()


def test_oracle_derived_commit_times_end_to_end(amd, oracle):
    """The reference on the ORACLE's histories, startup times and commit times derived from fresh oracle runs: nothing of the device."""
    import commit_times_oracle as cto
    n, seeds, max_clock = 4, np.arange(1, 17, dtype=np.uint64), 300
    ps = amd.ParamSet()
    cfg = oracle_cfg(oracle, n, ps)
    histories, counts, startup = chain_ref.oracle_runs(oracle, cfg, seeds, max_clock)
    ct = cto.commit_times(oracle, cfg, seeds, max_clock, histories.shape[2])
    want = ref.samples(ct, counts, histories, startup, None, None, 0, 30000, None, 1)
    sim = plain(amd, seeds, n, ps, commit_times=True)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all() and (res.commit_counts == counts).all()
    check(res, max_clock, [(None, None), (7, 5)], want=want)
    sim.close()


# ---- class 1, 64-wide tiles: one full tile and a partial one ----
def test_mid_class_tiles_with_equivocators_and_loss(amd):
    n, max_clock, seeds = 7, 1000, np.arange(1, 71, dtype=np.uint64)
    sim = plain(amd, seeds, n, amd.ParamSet(drop_per_million=50000), quirks=3, equivocate_every=3, commit_times=True)
    res = sim.loop_until(max_clock)
    assert sim.layout()["kernel_class"] & 0xff == 1 and (res.faults == 0).all()
    fam, _, _, first, _ = check(res, max_clock, [(None, None), (3, 40)])
    assert len(fam[0][ref.FIRST]) >= len(fam[0][ref.ALL]) > 0 and (first[0] > 0).sum() > 1
    sim.close()


# ---- 32 nodes: the tile's last row and the widest column ----
def test_thirty_two_nodes(amd):
    n, max_clock, seeds = 32, 400, np.arange(1, 4, dtype=np.uint64)
    sim = plain(amd, seeds, n, amd.ParamSet(), commit_times=True)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    fam, _, _, _, stats = check(res, max_clock, [(None, None), (2, 5)])
    assert stats[0, 4 * ref.OPEN] == 3 and len(fam[0][ref.QUORUM]) > 0 and (res.commit_counts[:, n - 1] > 0).all()
    sim.close()


# ---- weighted rights and epochs ----
@pytest.mark.parametrize("max_clock,kw", [(1000, {}), (1500, dict(commands_per_epoch=3, rights_rotation=1, quirks=3))])
def test_weighted_and_rotating_rights(amd, max_clock, kw):
    n, seeds, rights = 5, np.arange(1, 9, dtype=np.uint64), [5, 1, 1, 1, 1]
    sim = plain(amd, seeds, n, amd.ParamSet(), voting_rights=rights, commit_times=True, **kw)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    rule = dict(rights=rights, rotation=kw.get("rights_rotation", 0), commands_per_epoch=kw.get("commands_per_epoch", 30000))
    # on the reference first: the rights matter on this data -- under unit rights (quorum 4 of 5 nodes, not 7 of 9 votes) at least one
    # entry's quorum time is another, or defined where it was not
    weighted, unit = ref.of_result(res, **rule)[0][0], ref.of_result(res)[0][0]
    differ = len(weighted[ref.QUORUM]) != len(unit[ref.QUORUM]) or (weighted[ref.QUORUM] != unit[ref.QUORUM]).any()
    print("quorum samples: weighted %d, unit %d" % (len(weighted[ref.QUORUM]), len(unit[ref.QUORUM])))
    assert differ
    if kw:  # and so does the rotation: the fixed rights give other quorum times than the rotating ones
        fixed = ref.of_result(res, rights=rights)[0][0]
        assert len(fixed[ref.QUORUM]) != len(weighted[ref.QUORUM]) or (fixed[ref.QUORUM] != weighted[ref.QUORUM]).any()
        assert (res.epochs == res.commit_counts // 3).all() and res.epochs.min() > 2  # the entry index gives the epoch
    check(res, max_clock, [(None, None), (5, 20)], **rule)
    sim.close()


# ---- a partition ----
def test_partition_spreads_the_commits_of_an_entry(amd):
    """Nodes {0, 1} of 4 cut off during [300, 600), quirks = 3, seeds 1..32, clock 1500, beside a control set."""
    n, max_clock, per = 4, 1500, 32
    set_of = np.repeat(np.arange(2), per).astype(np.uint32)
    seeds = np.tile(np.arange(1, per + 1), 2).astype(np.uint64)
    d = amd.RandomDelay.new(10.0, 4.0)
    sets = [amd.ParamSet(d, amd.NodeConfig()), amd.ParamSet(d, amd.NodeConfig(), partition=(2, 300, 600))]
    sim = amd.BatchSimulator.with_param_sets(seeds, n, sets, set_of, quirks=3, commit_times=True)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    fam, _, _, first, stats = check(res, max_clock, [(None, None), (20, None)], set_of=set_of, groups=2)
    rows = res.finality_by_param_set()
    print("control %s\npartition %s" % (json.dumps(rows[0]), json.dumps(rows[1])))
    assert rows[1]["spread"]["max"] > rows[0]["spread"]["max"] + 250 and rows[1]["all"]["max"] > rows[0]["all"]["max"] + 250
    assert (first.sum(axis=1) == stats[:, 4 * ref.FIRST]).all() and rows[0]["first"]["samples"] == sum(rows[0]["first_committer"])
    assert abs(rows[1]["quorum"]["quantiles"]["0.5"] - rows[0]["quorum"]["quantiles"]["0.5"]) <= 2  # the typical entry is final as fast
    for k, row in enumerate(rows):
        for f, name in enumerate(ref.NAMES):
            s = fam[k][f]
            assert row[name]["instances" if name == "open" else "samples"] == len(s) and row[name]["min"] == s.min() and row[name]["max"] == s.max()
            assert row[name]["mean"] == pytest.approx(s.mean(), rel=1e-12)
        for name in ("quorum", "spread"):
            for q in (0.5, 0.9, 0.99):
                assert row[name]["quantiles"][str(q)] == int(np.quantile(fam[k][ref.NAMES.index(name)], q, method="inverted_cdf")), (k, name, q)
        assert row["first_share"] == [c / sum(row["first_committer"]) for c in row["first_committer"]]
    sim.close()


# ---- parameter sets: a set nobody uses, instances that overflowed their logs ----
def test_parameter_sets_with_an_unused_set_and_log_overflows(amd):
    n, max_clock, lcap = 4, 1000, 64
    sets = [amd.ParamSet(), amd.ParamSet(amd.RandomDelay.new(20.0, 9.0)), amd.ParamSet(amd.RandomDelay.new(3.0, 1.0)), amd.ParamSet(drop_per_million=10000)]
    set_of = np.array([0, 2, 1, 0, 2, 0, 1, 2, 0, 1, 2, 0, 0], dtype=np.uint32)  # 6, 3 and 4 instances; set 3 is unused
    seeds = np.arange(1, len(set_of) + 1, dtype=np.uint64)
    sim = amd.BatchSimulator.with_param_sets(seeds, n, sets, set_of, log_capacity=lcap, commit_times=True)
    res = sim.loop_until(max_clock, allow_faults=True)
    assert (res.faults == np.where(set_of == 2, LOG_OVERFLOW, 0)).all(), res.faults  # only the fast set's instances outgrow 64 entries
    fam, fin, spread, first, stats = check(res, max_clock, [(None, None), (5, 20)], set_of=set_of, groups=len(sets), log_capacity=lcap)
    assert not stats[2].any() and not stats[3].any() and not first[2:].any() and not fin[2:].any() and not spread[2:].any()  # all faulted; unused
    assert stats[0, 4 * ref.OPEN] == 6 and stats[1, 4 * ref.OPEN] == 3 and stats[0, 4 * ref.QUORUM] > 0
    rows = res.finality_by_param_set()
    assert [r["set"] for r in rows] == [0, 1, 2, 3] and rows[3]["first_share"] is None and rows[2]["open"]["instances"] == 0
    for k in (0, 1):  # every group row is the plain batch of that set
        p = plain(amd, seeds[set_of == k], n, sets[k], commit_times=True)
        pr = p.loop_until(max_clock)
        assert same([a[0] for a in pr.finality_histogram()], [a[k] for a in res.finality_histogram()])
        assert pr.finality_by_param_set()[0] == dict(rows[k], set=0)
        p.close()
    sim.close()


# ---- lifecycle: reset, steps, checkpoint ----
def test_reset_steps_and_checkpoint(amd, tmp_path):
    from librabft_simulator_amd import _lib
    n, max_clock, seeds = 4, 500, np.arange(1, 17, dtype=np.uint64)
    mk = lambda: plain(amd, seeds, n, amd.ParamSet(partition=(1, 200, 300)), quirks=3, commit_times=True)  # noqa: E731
    sim = mk()
    res = sim.loop_until(max_clock)
    check(res, max_clock)
    want = arrays(res)
    counts = res.commit_counts.copy()
    assert same(want, arrays(res)) and (res.commit_counts == counts).all()  # the call changes no state
    other = [res.latency_histogram(), res.stall_histogram()]
    assert same(want, arrays(res)) and same(list(other[0]) + list(other[1]), list(res.latency_histogram()) + list(res.stall_histogram()))
    sim.reset()
    with pytest.raises(amd.LbftError) as e:  # between reset() and the next run
        amd.BatchResult(sim).finality_histogram()
    assert e.value.code == _lib.LBFT_ERR_STATE
    assert same(want, arrays(sim.loop_until(max_clock)))
    sim.close()
    a = mk()
    assert same(want, arrays(run_to_end(a, max_clock, 150)))  # run_steps to the end
    a.close()
    a = mk()
    left, _ = a.run_steps(max_clock, 150)
    assert left > 0
    with pytest.raises(amd.LbftError) as e:  # (an unfinished run is no finished run)
        amd.BatchResult(a).finality_histogram()
    assert e.value.code == _lib.LBFT_ERR_STATE
    a.save_checkpoint(str(tmp_path / "ck.bin"))
    a.close()
    b = mk()  # a fresh timed batch
    b.load_checkpoint(str(tmp_path / "ck.bin"))
    assert same(want, arrays(run_to_end(b, max_clock, 150)))
    b.close()


# ---- refusals ----
def test_refusals(amd):
    from librabft_simulator_amd import _lib
    L = _lib.lib()
    seeds = np.arange(1, 5, dtype=np.uint64)
    fin, spread = np.full(8, 7, dtype=np.uint64), np.full(8, 7, dtype=np.uint64)
    first, stats = np.full(4, 7, dtype=np.uint64), np.full(24, 7, dtype=np.uint64)
    p = [a.ctypes.data for a in (fin, spread, first, stats)]
    untimed = plain(amd, seeds, 4, amd.ParamSet())
    ru = untimed.loop_until(200)
    assert L.lbft_batch_commit_finality(untimed._h, 1, 8, *p) == _lib.LBFT_ERR_STATE == -4  # an untimed batch
    for call in (lambda r: r.finality_histogram(), lambda r: r.finality_by_param_set()):
        with pytest.raises(amd.LbftError) as e:
            call(ru)
        assert e.value.code == _lib.LBFT_ERR_STATE
    ru.chain_stats()  # ... which still answers what it can
    untimed.close()
    sim = plain(amd, seeds, 4, amd.ParamSet(), commit_times=True)
    assert L.lbft_batch_commit_finality(sim._h, 1, 8, *p) == _lib.LBFT_ERR_STATE  # before the run
    res = sim.loop_until(200)
    assert L.lbft_batch_commit_finality(sim._h, 1, 0, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_commit_finality(sim._h, 0, 8, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_commit_finality(sim._h, 1, 2 ** 31 + 1, *p) == _lib.LBFT_ERR_INVALID  # groups x bins > 2^31
    for k in range(4):
        q = list(p)
        q[k] = None
        assert L.lbft_batch_commit_finality(sim._h, 1, 8, *q) == _lib.LBFT_ERR_INVALID
    assert (fin == 7).all() and (spread == 7).all() and (first == 7).all() and (stats == 7).all()
    # after the refusals the batch still answers, and runs again
    assert L.lbft_batch_commit_finality(sim._h, 1, 8, *p) == _lib.LBFT_OK and fin.sum() == stats[4 * ref.QUORUM] and first.sum() == stats[0] > 0
    with pytest.raises(ValueError):
        res.finality_histogram(bins=0)
    check(res, 200)
    sim.reset()
    check(sim.loop_until(300), 300)
    sim.close()


# ---- the grid tool ----
def test_grid_cli_finality(amd):
    args = ["--nodes", "4", "--delta", "10,20", "--seeds-per-point", "8", "--max-clock", "300", "--assign", "interleaved"]
    out = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid", "--finality"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.strip()]
    assert [l["delta"] for l in lines] == [10, 20]
    from librabft_simulator_amd import grid
    sets = [amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, d, 2.0, 0.5)) for d in (10, 20)]
    set_of, seed_index = grid.set_assignment(2, 8, "interleaved")
    sim = amd.BatchSimulator.with_param_sets((1 + seed_index).astype(np.uint64), 4, sets, set_of, commit_times=True)
    res = sim.loop_until(300, allow_faults=True)
    for l in lines:
        assert set(l["finality"]) == {"set", "first_committer", "first_share", *ref.NAMES} and l["faulted"] == 0 and l["finality"]["open"]["instances"] == 8
    assert [l["finality"] for l in lines] == json.loads(json.dumps(res.finality_by_param_set()))
    sim.close()
