"""The commit phases on the device (BatchResult.phase_histogram / phases_by_param_set, lbft_k_ct_phases): in every case the device's
arrays equal the numpy reference of the definitions (tests/commit_phases_reference.py) evaluated on the batch's own read-backs --
commit_times(), committed_histories, startup_times, faults, commit_counts, which other tests hold against the oracle --; with one phase
they are latency_histogram()'s and finality_histogram()'s bit for bit, and for any edges the phases add up to that.  The shapes are the
smallest that reach each mechanism: a second 64-entry chunk with an edge inside a chunk, eight phases with empty ones, a partition
whose three phases exceed one LDS pass, weighted rotating rights, 1, 3 and 32 nodes, 64-wide tiles, and the layouts of
tests/strided_shapes.py in which a wavefront takes a second and a third instance, with faulted instances between clean ones.  Every
case asserts its own precondition on the reference."""
import numpy as np
import pytest

import commit_phases_reference as ref
import strided_shapes as S
from support import amd, binning, plain, run_to_end, same  # noqa: F401

pytestmark = pytest.mark.gpu
BINNINGS = [(None, None), (7, 5)]  # the default (exact); the last bin clamps


def one_phase_is_the_pooled_calls(res, width=None, bins=None):
    """phases == 1: bit for bit the latency histogram's (hist, stats) and the finality's finality_hist and families 0 to 4."""
    lat, fin, stats = res.phase_histogram([], width, bins)
    l_hist, l_stats = res.latency_histogram(width, bins)
    f_hist, _, _, f_stats = res.finality_histogram(width, bins)
    groups = l_hist.shape[0]
    assert lat.shape == fin.shape == (groups, 1, l_hist.shape[1]) and stats.shape == (groups, 1, ref.FAMILIES, 4)
    assert (lat[:, 0] == l_hist).all() and (fin[:, 0] == f_hist).all()
    assert (stats[:, 0, ref.LATENCY] == l_stats).all() and (stats[:, 0, 1:].reshape(groups, 20) == f_stats[:, :20]).all()
    return lat, fin, stats


def check(res, max_clock, edges, binnings=BINNINGS, set_of=None, groups=1, log_capacity=None, **rule):
    """phase_histogram(edges) equals the reference on the batch's own read-backs for every binning, and its phases add up to the
    one-phase result, which is the pooled calls'.  -> (the reference's families, the arrays of the default binning)."""
    per_group = res._phase_edges(edges)
    ct = res.commit_times()
    fam = ref.samples(ct, res.commit_counts, res.committed_histories(ct.shape[2]), res.startup_times, res.faults,
                      rule.get("rights"), rule.get("rotation", 0), rule.get("commands_per_epoch", 30000), set_of, groups, per_group, log_capacity)
    first = None
    for width, bins in binnings:
        got = res.phase_histogram(edges, width, bins)
        w, b = binning(max_clock, width, bins)
        want = ref.bin_phases(fam, w, b, max_clock)
        assert all(a.dtype == np.uint64 for a in got) and got[0].shape == got[1].shape == (groups, per_group.shape[1] + 1, b)
        print("binning (%s, %s): samples per phase and family %s" % (width, bins, got[2][:, :, :, ref.SAMPLES].sum(axis=0).tolist()))
        for name, a, c in zip(("latency_hist", "finality_hist", "stats"), got, want):
            assert (a == c).all(), (name, width, bins, np.argwhere(a != c)[:8], a[a != c][:8], c[a != c][:8])
        whole = one_phase_is_the_pooled_calls(res, width, bins)
        assert same([a[:, 0] for a in whole], list(ref.pooled(*got))), (width, bins)
        first = first or got
    return fam, first


# ---- a second chunk; eight phases ----
SEEDS = np.arange(1, 65, dtype=np.uint64)
PARTITION = (2, 300, 600)


@pytest.fixture(scope="module")
def long_chains(amd):
    sim = plain(amd, SEEDS, 4, amd.ParamSet(), commit_times=True)
    res = sim.loop_until(2500)
    assert (res.faults == 0).all() and res.commit_counts.max() > 64  # a chain with a second chunk
    yield sim, res
    sim.close()


@pytest.mark.parametrize("edges", [[400, 2000], [0, 300, 300, 1203, 1204, 2500, 2501]], ids=["warm_up_and_cool_down", "eight_phases"])
def test_chains_of_more_than_one_chunk(long_chains, edges):
    sim, res = long_chains
    fam, (lat, fin, stats) = check(res, 2500, edges)
    filled = stats[0, :, ref.QUORUM, ref.SAMPLES] > 0
    assert filled.sum() >= 2 and any(ref.splits_a_chunk(p) for p in ref.chain_phases(res, edges))  # an edge between two entries of one chunk
    if len(edges) == 7:
        assert not stats[0, [0, 2, 7]].any() and filled[[1, 3, 5]].all()  # edge 0, equal edges and max_clock + 1: empty phases
    rows = res.phases_by_param_set(edges, (0.0, 0.5, 1.0))
    assert len(rows) == 1 and rows[0]["set"] == 0 and [(r["from"], r["to"]) for r in rows[0]["phases"]] == list(zip([0] + edges, edges + [2501]))
    for p, row in enumerate(rows[0]["phases"]):
        for f, name in enumerate(ref.NAMES):
            s = fam[0][p][f]
            if not len(s):
                assert row[name] == {"samples": 0, "mean": None, "min": None, "max": None, **({"quantiles": {"0.0": None, "0.5": None, "1.0": None}} if f in (ref.LATENCY, ref.QUORUM) else {})}
                continue
            assert (row[name]["samples"], row[name]["min"], row[name]["max"]) == (len(s), s.min(), s.max()) and row[name]["mean"] == pytest.approx(s.mean(), rel=1e-12)
            if f in (ref.LATENCY, ref.QUORUM):
                assert [row[name]["quantiles"][q] for q in ("0.0", "0.5", "1.0")] == [int(np.quantile(s, q, method="inverted_cdf")) for q in (0.0, 0.5, 1.0)]


# ---- a partition: before, during, after ----
@pytest.fixture(scope="module")
def partitioned(amd):
    """The partition fixture: nodes {0, 1} of 4 cut off during [300, 600), quirks = 3, 64 seeds to clock 1500."""
    sim = plain(amd, SEEDS, 4, amd.ParamSet(partition=PARTITION), quirks=3, commit_times=True)
    res = sim.loop_until(1500)
    assert (res.faults == 0).all()
    yield sim, res
    sim.close()


def test_partition_phases(partitioned):
    """edges="partition" on the partition fixture: with the default binning 3 x 1 501 bins take two LDS passes; width 7 with 5 bins
    clamps into the last bin.  The precondition on the reference: neither side of the cut holds a quorum and messages across it are
    dropped, not delayed, so no block proposed during [300, 600) is ever committed -- "during" is empty in every family, on the
    reference as on the device -- and what the phases show is the cohort rule: the entries proposed just before the cut are committed
    after it ends and belong to "before", whose quorum finality therefore exceeds the partition's length, while "after" is back to
    normal.  Measured, quorum finality (samples, sum, min, max): before (706, 109118, 62, 576), during (0, 0, 0, 0), after (1760,
    149164, 63, 172).  (A "during" cohort with the largest maximum cannot be had under this rule: whatever delays an entry proposed in
    the window delays the last entries proposed before it by at least as much.  test_partition_of_one_node has a partition whose
    "during" cohort commits: there all three phases have quorum samples.)"""
    sim, res = partitioned
    assert res._phase_edges("partition").tolist() == [[300, 600]] and 3 * 1501 > ref.LDS_BINS
    want = ref.bin_phases(ref.of_result(res, [300, 600]), 1, 1501, 1500)[2][0, :, ref.QUORUM]
    print("reference, quorum finality before / during / after: %s" % want.tolist())
    assert want[0, ref.SAMPLES] > 0 and want[2, ref.SAMPLES] > 0 and want[0, ref.MAX] > 300 > want[2, ref.MAX]  # the partition matters on this data
    assert not want[1].any()  # nothing proposed inside the window commits: an empty phase between two full ones
    fam, (lat, fin, stats) = check(res, 1500, "partition")
    assert same(res.phase_histogram("partition"), res.phase_histogram([300, 600])) and (stats[0, :, ref.QUORUM] == want).all()


def test_partition_of_one_node(amd):
    """Node 0 of 4 cut off during [300, 600): the other three hold a quorum (3 of 4 rights) and go on committing what they propose, so
    "during" has quorum samples; node 0 commits those entries only after it is back, so the all-node finality of "during" is far above
    that of "after"."""
    sim = plain(amd, SEEDS, 4, amd.ParamSet(partition=(1, 300, 600)), quirks=3, commit_times=True)
    res = sim.loop_until(1500)
    assert (res.faults == 0).all() and res._phase_edges("partition").tolist() == [[300, 600]]
    fam, (lat, fin, stats) = check(res, 1500, "partition")
    print("quorum %s all %s" % (stats[0, :, ref.QUORUM].tolist(), stats[0, :, ref.ALL].tolist()))
    assert (stats[0, :, ref.QUORUM, ref.SAMPLES] > 0).all() and stats[0, 1, ref.ALL, ref.SAMPLES] > 0
    assert stats[0, 1, ref.ALL, ref.MAX] > stats[0, 2, ref.ALL, ref.MAX]
    sim.close()


# ---- rights, sizes, the other layout ----
def test_weighted_rotating_rights(amd):
    rights, kw = [5, 1, 1, 1, 1], dict(commands_per_epoch=3, rights_rotation=1, quirks=3)
    sim = plain(amd, np.arange(1, 9, dtype=np.uint64), 5, amd.ParamSet(), voting_rights=rights, commit_times=True, **kw)
    res = sim.loop_until(1500)
    assert (res.faults == 0).all() and res.epochs.min() >= 2  # the rights rotated, more than once
    rule = dict(rights=rights, rotation=1, commands_per_epoch=3)
    fam, (lat, fin, stats) = check(res, 1500, [500, 1000], **rule)
    fixed = ref.bin_phases(ref.of_result(res, [500, 1000], rights=rights), 1, 1501)[2]
    assert (fixed[0, :, ref.QUORUM] != stats[0, :, ref.QUORUM]).any() and (stats[0, :, ref.QUORUM, ref.SAMPLES] > 0).all()  # the rotation matters
    sim.close()


@pytest.mark.parametrize("n,kw", [(1, {}), (3, {}), (32, dict(drop_per_million=20000))], ids=["n1", "n3", "n32_lossy_tiles"])
def test_network_sizes_and_64_wide_tiles(amd, n, kw):
    sim = plain(amd, np.arange(1, 9, dtype=np.uint64), n, amd.ParamSet(**kw), commit_times=True)
    res = sim.loop_until(500)
    assert (res.faults == 0).all()
    if kw:
        assert sim.layout()["kernel_class"] & 0xff == 1  # 64-wide tiles: the other layout
    fam, (lat, fin, stats) = check(res, 500, [150, 300])
    assert (stats[0, :, ref.LATENCY, ref.SAMPLES] > 0).sum() >= 2 and stats[0, :, ref.QUORUM, ref.SAMPLES].max() > 0
    sim.close()


# ---- where a wavefront takes several instances ----
def group_edges():
    """Different edges per group: 0 to 3 of them would not do (every group needs the same number), so two per group, spread over the clock."""
    g = np.arange(S.GROUPS)
    return np.stack([(g * 7) % 500, 500 + (g * 13) % 502], axis=1)


def layout(amd, **kw):
    f = S.FLAVOURS["partition"]
    set_of, seeds = S.assignment(f["background"])
    return set_of, amd.BatchSimulator.with_param_sets(seeds, f["n"], S.param_sets("partition"), set_of, quirks=f["quirks"], commit_times=True, **kw)


def test_strided_parameter_sets_clean_and_with_faults(amd):
    """The 256-set layout of tests/strided_shapes.py (a set with a partition, quirks = 3): groups of 38, 33 and 17 instances under 4
    workgroups of 4 wavefronts per group.  Then the same layout with a log capacity that about half of the fast group's instances
    outgrow: a wavefront's trips mix faulted and clean instances."""
    set_of, sim = layout(amd)
    res = sim.loop_until(S.MAX_CLOCK)
    assert (res.faults == 0).all()
    gx = S.grid_x(S.GROUPS, 38, 4 << 16)  # (the new kernel's grid: an instance gives at most n x log capacity samples, the capacity below 2^16)
    assert max(S.trips(38, gx)) == 3 and max(S.trips(33, gx)) == 3 and max(S.trips(17, gx)) == 2  # a second and a third trip
    edges = group_edges()
    assert len({tuple(edges[g]) for g in S.STRIDED}) == len(S.STRIDED)
    fam, (lat, fin, stats) = check(res, S.MAX_CLOCK, edges, [(None, None), (1, 2 * ref.LDS_BINS + 7)], set_of, S.GROUPS)
    sizes = S.group_sizes()
    assert not stats[sizes == 0].any() and not lat[sizes == 0].any() and stats[S.FAST, :, ref.QUORUM, ref.SAMPLES].all()
    lengths = res.commit_counts.max(axis=1)
    sim.close()
    fast = S.members(set_of, S.FAST)
    lcap = int(np.median(lengths[fast]))
    expected = np.where(lengths > lcap, 1 << 3, 0).astype(np.uint32)  # LBFT_FAULT_LOG_OVERFLOW
    assert 0 < (expected[fast] != 0).sum() < len(fast)
    set_of, sim = layout(amd, log_capacity=lcap)
    res = sim.loop_until(S.MAX_CLOCK, allow_faults=True)
    assert (res.faults == expected).all()
    fam, (lat, fin, stats) = check(res, S.MAX_CLOCK, edges, [(None, None)], set_of, S.GROUPS, log_capacity=lcap)
    clean = ref.bin_phases(ref.of_result(res, edges, set_of=set_of, groups=S.GROUPS, log_capacity=lcap), 1, S.MAX_CLOCK + 1)[2]
    assert (clean[S.FAST] == stats[S.FAST]).all()
    ct = res.commit_times()
    everyone = ref.samples(ct, res.commit_counts, res.committed_histories(ct.shape[2]), res.startup_times, None, None, 0, 30000, set_of, S.GROUPS, edges, lcap)
    assert sum(len(p[ref.QUORUM]) for p in everyone[S.FAST]) > stats[S.FAST, :, ref.QUORUM, ref.SAMPLES].sum() > 0  # the faulted instances do hold samples
    sim.close()


def test_strided_plain_batch_of_4102_instances(amd):
    shape = S.PLAIN
    sim = plain(amd, S.plain_seeds(shape), shape["n"], amd.ParamSet(), commit_times=True)
    res = sim.loop_until(shape["max_clock"])
    assert (res.faults == 0).all()
    gx = S.grid_x(1, shape["m"], shape["n"] << 16)
    assert sorted(set(S.trips(shape["m"], gx))) == [1, 2]  # grp_inst == NULL, some wavefronts make a second trip
    fam, (lat, fin, stats) = check(res, shape["max_clock"], [100, 200], [(None, None)])
    assert stats[0, :, ref.FIRST, ref.SAMPLES].sum() == res.commit_counts.max(axis=1).sum() and (stats[0, :, ref.QUORUM, ref.SAMPLES] > 0).all()
    sim.close()


# ---- call order and state ----
def test_call_order_and_state(amd, tmp_path):
    from librabft_simulator_amd import _lib
    L = _lib.lib()
    n, max_clock, seeds = 4, 500, np.arange(1, 17, dtype=np.uint64)
    mk = lambda: plain(amd, seeds, n, amd.ParamSet(partition=(1, 200, 300)), quirks=3, commit_times=True)  # noqa: E731
    bins = max_clock + 1
    lat, fin, stats = np.full((3, bins), 7, dtype=np.uint64), np.full((3, bins), 7, dtype=np.uint64), np.full((3, 24), 7, dtype=np.uint64)
    edges = np.array([200, 300], dtype=np.int64)
    call = lambda h, e=edges: L.lbft_batch_commit_phases(h, e.ctypes.data, 3, 1, bins, lat.ctypes.data, fin.ctypes.data, stats.ctypes.data)  # noqa: E731
    untimed = plain(amd, seeds, n, amd.ParamSet())
    ru = untimed.loop_until(200)
    assert call(untimed._h) == _lib.LBFT_ERR_STATE == -4  # an untimed batch
    with pytest.raises(amd.LbftError) as e:
        ru.phase_histogram([100])
    assert e.value.code == _lib.LBFT_ERR_STATE
    untimed.close()
    sim = mk()
    assert call(sim._h) == _lib.LBFT_ERR_STATE  # before the run
    assert call(sim._h, np.array([300, 200], dtype=np.int64)) == _lib.LBFT_ERR_STATE  # (the state is looked at before the edges)
    assert L.lbft_batch_commit_phases(sim._h, None, 3, 1, bins, lat.ctypes.data, fin.ctypes.data, stats.ctypes.data) == _lib.LBFT_ERR_INVALID
    res = sim.loop_until(max_clock)
    hashes = res.last_committed_states.copy()
    for bad in ([300, 200], [-1, 5], [0, max_clock + 2], [max_clock + 2, max_clock + 2]):
        assert call(sim._h, np.array(bad, dtype=np.int64)) == _lib.LBFT_ERR_INVALID, bad
    assert L.lbft_batch_commit_phases(sim._h, edges.ctypes.data, 9, 1, bins, lat.ctypes.data, fin.ctypes.data, stats.ctypes.data) == _lib.LBFT_ERR_INVALID
    assert (lat == 7).all() and (fin == 7).all() and (stats == 7).all()  # nothing was written
    assert call(sim._h, np.array([0, max_clock + 1], dtype=np.int64)) == _lib.LBFT_OK and (stats != 7).any()
    other = lambda r: [r.commit_counts.copy(), r.commit_times(), *r.latency_histogram(), *r.stall_histogram("partition_end"), *r.finality_histogram()]  # noqa: E731
    before = other(res)
    fam, got = check(res, max_clock, "partition")
    assert same(res.phase_histogram("partition"), got)  # twice in a row
    assert all((a == b).all() for a, b in zip(before, other(res)))  # the batch's other results are as they were
    assert (amd.BatchResult(sim).last_committed_states == hashes).all()
    sim.reset()
    with pytest.raises(amd.LbftError) as e:  # between reset() and the next run
        amd.BatchResult(sim).phase_histogram("partition")
    assert e.value.code == _lib.LBFT_ERR_STATE
    assert same(sim.loop_until(max_clock).phase_histogram("partition"), got)
    sim.close()
    a = mk()
    left, _ = a.run_steps(max_clock, 150)
    assert left > 0
    with pytest.raises(amd.LbftError) as e:  # (an unfinished run is no finished run)
        amd.BatchResult(a).phase_histogram("partition")
    assert e.value.code == _lib.LBFT_ERR_STATE
    a.save_checkpoint(str(tmp_path / "ck.bin"))
    assert same(run_to_end(a, max_clock, 150).phase_histogram("partition"), got)  # run_steps once it reports 0
    a.close()
    b = mk()  # a fresh timed batch
    b.load_checkpoint(str(tmp_path / "ck.bin"))
    assert same(run_to_end(b, max_clock, 150).phase_histogram("partition"), got)
    b.close()
