"""The per-instance statistics on the device (BatchResult.instance_stats / seed_spread, lbft_k_ct_instances): in every case the device's
table equals the numpy reference (tests/instance_stats_reference.py: the grouped calls' references with every instance a group of its
own) evaluated on the batch's own read-backs -- commit_times(), committed_histories, startup_times, faults, commit_counts, which other
tests hold against the oracle -- and once on commit times derived from the oracle end to end; and, without any reference, the rows of
a group add up to what the grouped calls report for it.  The shapes are the smallest that reach each mechanism: a second 64-entry
chunk, a partition with `since` at its end, weighted rotating rights, 1, 3 and 32 nodes, 64-wide tiles, parameter sets with faulted
instances between clean ones, and the smallest batch in which a wavefront takes a second instance.  Every case asserts its own
precondition on the reference."""
import numpy as np
import pytest

import chain_stats_reference as chain_ref
import instance_stats_reference as ref
import strided_shapes as S
from support import amd, oracle_cfg, plain, run_to_end  # noqa: F401

pytestmark = pytest.mark.gpu
F = ref


def grouped(res, since, groups):
    """[groups, 11, 4]: the statistics of the three grouped calls side by side, in the order of a row."""
    return np.concatenate([res.latency_histogram()[1], res.stall_histogram(since)[1], res.finality_histogram()[3]], axis=1).reshape(groups, ref.FAMILIES, 4)


def consistent(res, rows, since, set_of, groups):
    """Without a reference: per group and family, the rows' samples and sums add up to the grouped call's, the least minimum over the
    rows with samples is its minimum, the largest maximum its maximum."""
    whole = grouped(res, since, groups)
    set_of = np.zeros(len(rows), dtype=np.int64) if set_of is None else np.asarray(set_of)
    for g in range(groups):
        mine = rows[set_of == g]
        assert (mine[:, :, ref.SAMPLES].sum(axis=0) == whole[g, :, ref.SAMPLES]).all() and (mine[:, :, ref.SUM].sum(axis=0) == whole[g, :, ref.SUM]).all(), g
        for f in range(ref.FAMILIES):
            have = mine[:, f, ref.SAMPLES] > 0
            assert whole[g, f, ref.MIN] == (mine[have, f, ref.MIN].min() if have.any() else 0), (g, f)
            assert whole[g, f, ref.MAX] == (mine[have, f, ref.MAX].max() if have.any() else 0), (g, f)
    return whole


def check(res, max_clock, since=None, set_of=None, groups=1, want=None, **rule):
    """instance_stats(since) equals the reference on the batch's own read-backs (or `want`), and its rows add up to the grouped calls'."""
    per_group = res._since(since)
    if want is None:
        want = ref.instance_stats(res, max_clock, per_group, set_of, **rule)
    got = res.instance_stats(since)
    assert got.shape == (res._sim.num_instances, ref.FAMILIES, 4) and got.dtype == np.uint64
    bad = np.argwhere(got != want)
    print("rows %d, samples per family %s" % (len(got), got[:, :, ref.SAMPLES].sum(axis=0).tolist()))
    assert not len(bad), (bad[:8], got[got != want][:8], want[got != want][:8])
    assert not got[res.faults != 0].any()
    clean = res.faults == 0
    assert (got[clean, F.OPEN, ref.SAMPLES] == 1).all() and (got[clean, F.TAIL, ref.SAMPLES] == res._sim.num_nodes).all()  # one per instance, one per node
    consistent(res, got, since, set_of, groups)
    return want, got


# ---- a second chunk; a partition ----
SEEDS = np.arange(1, 65, dtype=np.uint64)
PARTITION = (2, 300, 600)


def test_chains_of_more_than_one_chunk(amd):
    sim = plain(amd, SEEDS, 4, amd.ParamSet(), commit_times=True)
    res = sim.loop_until(2500)
    lengths = res.commit_counts.max(axis=1)
    print("chain lengths %d .. %d" % (lengths.min(), lengths.max()))
    assert (res.faults == 0).all() and lengths.max() > 64  # a chain with a second chunk
    want, _ = check(res, 2500)
    assert (want[:, F.LATENCY, ref.SAMPLES] == res.commit_counts.sum(axis=1)).all() and (want[:, F.GAPS, ref.SAMPLES] > 0).all()
    want, _ = check(res, 2500, since=1203)
    assert (want[:, F.FIRST, ref.SAMPLES] == 4).all() and want[:, F.FIRST, ref.MAX].max() > 0
    check(res, 2500, since=2500)
    sim.close()


@pytest.fixture(scope="module")
def partitioned(amd):
    sim = plain(amd, SEEDS, 4, amd.ParamSet(partition=PARTITION), quirks=3, commit_times=True)
    res = sim.loop_until(1500)
    assert (res.faults == 0).all()
    yield sim, res
    sim.close()


def test_partition_with_since_at_its_end(partitioned):
    sim, res = partitioned
    assert res._since("partition_end").tolist() == [600]
    want, got = check(res, 1500, since="partition_end")
    assert want[:, F.OPEN, ref.SUM].max() > 0 and want[:, F.FIRST, ref.SAMPLES].sum() > 0  # an open entry somewhere; a `first` sample exists
    assert want[:, F.LONGEST, ref.MAX].max() >= 260  # a stall through the partition (commit_timeline_reference.SCENARIO_STALL)
    assert (got != res.instance_stats()).any()  # `since` matters on this data


def test_seed_spread_and_the_replay_of_the_worst_seed(amd, partitioned):
    sim, res = partitioned
    table = ref.instance_stats(res, 1500, [600]).astype(np.float64)
    commits = res.commit_counts.min(axis=1).astype(np.float64)
    (row,) = res.seed_spread(since="partition_end")
    assert (row["set"], row["instances"], row["faulted"]) == (0, 64, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        values = {"commits": (commits, np.ones(64, dtype=bool)),
                  "latency_mean": (table[:, 0, 1] / table[:, 0, 0], table[:, 0, 0] > 0), "latency_max": (table[:, 0, 3], table[:, 0, 0] > 0),
                  "longest_stall": (table[:, 4, 3], table[:, 4, 0] > 0), "recovery": (table[:, 2, 3], table[:, 2, 0] > 0),
                  "finality_quorum_mean": (table[:, 7, 1] / table[:, 7, 0], table[:, 7, 0] > 0), "finality_quorum_max": (table[:, 7, 3], table[:, 7, 0] > 0),
                  "spread_max": (table[:, 9, 3], table[:, 9, 0] > 0), "open": (table[:, 10, 1], table[:, 10, 0] > 0)}
    assert set(row) == {"set", "instances", "faulted", *values}
    for name, (v, have) in values.items():
        idx = np.nonzero(have)[0]
        v = v[idx]
        assert len(v) >= 2, name
        std = float(np.std(v, ddof=1))
        assert row[name] == {"instances": len(v), "mean": float(np.mean(v)), "std": std, "stderr": std / float(np.sqrt(len(v))), "min": float(v.min()),
                             "max": float(v.max()), "min_seed": int(SEEDS[idx[np.argmin(v)]]), "max_seed": int(SEEDS[idx[np.argmax(v)]])}, name
    # the replay the feature promises: the seed with the longest stall, run alone, is that instance
    seed = row["longest_stall"]["max_seed"]
    i = int(np.nonzero(SEEDS == seed)[0][0])
    ps = amd.ParamSet(partition=PARTITION)
    one = amd.Simulator.new(seed, 4, ps.network_delay, ps.node_config, quirks=3, partition=PARTITION)
    one.loop_until(1500)
    assert (one.result.commit_counts[0] == res.commit_counts[i]).all() and res.commit_counts[i].min() == commits[i]
    one._batch.close()


# ---- rights, sizes, the other layout ----
def test_weighted_rotating_rights(amd):
    rights, kw = [5, 1, 1, 1, 1], dict(commands_per_epoch=3, rights_rotation=1, quirks=3)
    sim = plain(amd, np.arange(1, 9, dtype=np.uint64), 5, amd.ParamSet(), voting_rights=rights, commit_times=True, **kw)
    res = sim.loop_until(1500)
    assert (res.faults == 0).all() and res.epochs.min() >= 2  # the rights rotated, more than once
    rule = dict(rights=rights, rotation=1, commands_per_epoch=3)
    want, _ = check(res, 1500, since=700, **rule)
    fixed = ref.instance_stats(res, 1500, [700], rights=rights)
    assert (fixed[:, F.FIN_QUORUM] != want[:, F.FIN_QUORUM]).any()  # the rotation matters on this data
    sim.close()


@pytest.mark.parametrize("n,kw", [(1, {}), (3, {}), (32, {}), (20, dict(drop_per_million=50000))], ids=["n1", "n3", "n32", "n20_lossy_tiles"])
def test_network_sizes_and_64_wide_tiles(amd, n, kw):
    sim = plain(amd, np.arange(1, 17, dtype=np.uint64), n, amd.ParamSet(**kw), commit_times=True)
    res = sim.loop_until(500)
    assert (res.faults == 0).all()
    if kw:
        assert sim.layout()["kernel_class"] & 0xff == 1  # 64-wide tiles: the other layout
    want, _ = check(res, 500, since=250)
    # (with loss some networks commit nothing by clock 500: rows without a latency sample beside rows with many)
    assert want[:, F.LATENCY, ref.SAMPLES].max() > 0 and want[:, F.FIN_QUORUM, ref.SAMPLES].max() > 0 and res.commit_counts[:, n - 1].max() > 0
    sim.close()


def test_oracle_derived_commit_times_end_to_end(amd, oracle):
    """The reference on the ORACLE's histories, startup times and commit times derived from fresh oracle runs: nothing of the device."""
    import commit_times_oracle as cto
    n, seeds, max_clock = 4, np.arange(1, 17, dtype=np.uint64), 300
    ps = amd.ParamSet()
    cfg = oracle_cfg(oracle, n, ps)
    histories, counts, startup = chain_ref.oracle_runs(oracle, cfg, seeds, max_clock)
    ct = cto.commit_times(oracle, cfg, seeds, max_clock, histories.shape[2])
    want = ref.instance_stats(ref.Readbacks(ct, histories, counts, startup), max_clock, [150])
    assert (want[:, F.LATENCY, ref.SAMPLES] == counts.sum(axis=1)).all() and want[:, F.FIN_ALL, ref.SAMPLES].min() > 0
    sim = plain(amd, seeds, n, ps, commit_times=True)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all() and (res.commit_counts == counts).all()
    check(res, max_clock, since=150, want=want)
    sim.close()


# ---- parameter sets, faulted instances between clean ones ----
def test_parameter_sets_with_faulted_instances(amd, oracle):
    """The 256-set layout of tests/strided_shapes.py with the log capacity about half of the fast group's instances outgrow: wavefronts
    of the strided groups take faulted and clean instances in turn.  The reference is evaluated on the strided groups' instances (the
    fast group's long chains included); the sums against the grouped calls cover every instance."""
    set_of, seeds, oracle_want = S.oracle_layout(oracle, "class0")
    lcap, expected = S.fault_case(oracle_want, set_of)
    sim = amd.BatchSimulator.with_param_sets(seeds, 4, S.param_sets("class0"), set_of, log_capacity=lcap, commit_times=True)
    res = sim.loop_until(S.MAX_CLOCK, allow_faults=True)
    assert (res.faults == expected).all()
    fast = S.members(set_of, S.FAST)
    assert 0 < (expected[fast] != 0).sum() < len(fast)  # faulted and clean instances in one strided group
    since = (np.arange(S.GROUPS) * 7) % (S.MAX_CLOCK + 1)  # one per set
    got = res.instance_stats(since)
    assert not got[expected != 0].any() and got[expected == 0][:, F.OPEN, ref.SAMPLES].all()
    consistent(res, got, since, set_of, S.GROUPS)
    idx = np.sort(np.concatenate([S.members(set_of, g) for g in S.STRIDED]))
    ct = res.commit_times()
    sub = ref.Readbacks(ct[idx], res.committed_histories(ct.shape[2])[idx], res.commit_counts[idx], res.startup_times[idx], res.faults[idx])
    want = ref.instance_stats(sub, S.MAX_CLOCK, since, set_of[idx], log_capacity=lcap)
    assert (got[idx] == want).all(), np.argwhere(got[idx] != want)[:8]
    lost = np.nonzero(expected[idx] != 0)[0]
    neighbours = [k for k in np.r_[lost - 1, lost + 1] if 0 <= k < len(idx) and expected[idx[k]] == 0]
    assert len(lost) and len(neighbours) and want[neighbours][:, F.LATENCY, ref.SAMPLES].all()  # clean rows beside the zero rows
    assert len({int(since[g]) for g in S.STRIDED}) == len(S.STRIDED) and want[:, F.FIRST, ref.SAMPLES].sum() > 0
    sim.close()


# ---- striding: a plain batch in which a wavefront takes a second instance ----
def test_smallest_batches_that_stride_and_one_instance(amd):
    """min(1024, ceil(m / 4)) workgroups of 4 wavefronts (tests/test_instance_stats_host.py pins the rule): at m = 4097 wavefront 0 of
    workgroup 0 takes instance 4096 after instance 0 and no other wavefront makes a second trip."""
    m, max_clock = 4097, 150
    sim = plain(amd, np.arange(1, m + 1, dtype=np.uint64), 4, amd.ParamSet(), commit_times=True)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    want, _ = check(res, max_clock, since=75)
    assert want[0, F.LATENCY, ref.SAMPLES] > 0 and want[4096, F.LATENCY, ref.SAMPLES] > 0 and (want[0] != want[4096]).any()  # two trips, unlike rows
    sim.close()
    sim = plain(amd, np.array([7], dtype=np.uint64), 4, amd.ParamSet(), commit_times=True)
    want, _ = check(sim.loop_until(300), 300)
    assert want[0, F.FIN_QUORUM, ref.SAMPLES] > 0
    sim.close()


# ---- call order and state ----
def test_call_order_and_state(amd, tmp_path):
    from librabft_simulator_amd import _lib
    L = _lib.lib()
    n, max_clock, seeds = 4, 500, np.arange(1, 17, dtype=np.uint64)
    mk = lambda: plain(amd, seeds, n, amd.ParamSet(partition=(1, 200, 300)), quirks=3, commit_times=True)  # noqa: E731
    rows = np.full((len(seeds), 44), 7, dtype=np.uint64)
    since = np.zeros(1, dtype=np.int64)
    untimed = plain(amd, seeds, n, amd.ParamSet())
    ru = untimed.loop_until(200)
    assert L.lbft_batch_instance_stats(untimed._h, None, rows.ctypes.data) == _lib.LBFT_ERR_STATE == -4  # an untimed batch
    with pytest.raises(amd.LbftError) as e:
        ru.instance_stats()
    assert e.value.code == _lib.LBFT_ERR_STATE
    untimed.close()
    sim = mk()
    assert L.lbft_batch_instance_stats(sim._h, None, rows.ctypes.data) == _lib.LBFT_ERR_STATE  # before the run
    res = sim.loop_until(max_clock)
    assert L.lbft_batch_instance_stats(sim._h, None, None) == _lib.LBFT_ERR_INVALID
    for bad in (-1, max_clock + 1):
        since[0] = bad
        assert L.lbft_batch_instance_stats(sim._h, since.ctypes.data, rows.ctypes.data) == _lib.LBFT_ERR_INVALID
    assert (rows == 7).all()  # nothing was written
    since[0] = max_clock
    assert L.lbft_batch_instance_stats(sim._h, since.ctypes.data, rows.ctypes.data) == _lib.LBFT_OK and (rows != 7).any()
    other = lambda r: [r.commit_counts.copy(), r.commit_times(), *r.latency_histogram(), *r.stall_histogram("partition_end"), *r.finality_histogram()]  # noqa: E731
    before = other(res)
    want, got = check(res, max_clock, since="partition_end")
    assert (res.instance_stats("partition_end") == got).all()  # twice in a row
    assert all((a == b).all() for a, b in zip(before, other(res)))  # the batch's other results are as they were
    sim.reset()
    with pytest.raises(amd.LbftError) as e:  # between reset() and the next run
        amd.BatchResult(sim).instance_stats()
    assert e.value.code == _lib.LBFT_ERR_STATE
    assert (sim.loop_until(max_clock).instance_stats("partition_end") == got).all()
    sim.close()
    a = mk()
    left, _ = a.run_steps(max_clock, 150)
    assert left > 0
    with pytest.raises(amd.LbftError) as e:  # (an unfinished run is no finished run)
        amd.BatchResult(a).instance_stats()
    assert e.value.code == _lib.LBFT_ERR_STATE
    a.save_checkpoint(str(tmp_path / "ck.bin"))
    assert (run_to_end(a, max_clock, 150).instance_stats("partition_end") == got).all()  # a drained run_steps
    a.close()
    b = mk()  # a fresh timed batch
    b.load_checkpoint(str(tmp_path / "ck.bin"))
    assert (run_to_end(b, max_clock, 150).instance_stats("partition_end") == got).all()
    b.close()
