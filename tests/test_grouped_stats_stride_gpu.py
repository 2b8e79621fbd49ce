"""The grouped statistics on the device where a wavefront takes several instances.  The wavefronts of lbft_k_cs_chain, lbft_k_ct_finality
and lbft_k_rs_rounds stride over the instances of their group; at every shape of the other device tests the stride loop's body runs at
most once per wavefront.  Here it runs two and three times (tests/strided_shapes.py has the shapes, tests/test_strided_shapes_host.py
states on the CPU that they stride): the per-instance registers start afresh on every trip, a faulted instance in the middle of a
wavefront's trips is skipped, the finality kernel's LDS tile is reused from one instance to the next, the statistics registers
accumulate over trips, the wavefronts of one workgroup leave the loop after different numbers of trips, and all of it again per LDS
pass.  In every case the device's arrays equal the numpy references of the definitions -- chain statistics on the ORACLE's histories,
finality on the batch's own read-backs, round statistics on the device's round_tables(), which are held against the oracle's tables for
the strided groups -- for the default binning, one whose last bin clamps and one of three LDS passes.
(What no device test can show: the chain kernel's `differing` and `inversions` are 0 for every instance a run can produce, and its
`carry_start` is overwritten by entry 0 before it is read, so keeping these three from one trip to the next changes no output here; the
audit families fire on the hand-written logs of tests/test_chain_stats_host.py.)

  A  256 parameter sets, clean: lane-private class-0 rows ("class0"), and with a set whose partition ends inside the horizon and
     quirks = 3, which the planner runs on 64-wide tiles ("partition"); the rows of the three groups of 38 equal plain batches of their
     sets and seeds, which do not stride
  B  the class-0 layout with a log capacity that about half of the fast group's instances outgrow: faulted and clean trips mixed
  C  7 nodes, quirks = 3, 2 % loss: 64-wide tiles with seven rows of commit times per instance
  D  plain batches of 4102 instances, grp_inst == NULL, the second with weighted rights that rotate every 3 commands
  E  repeated and interleaved calls"""
import numpy as np
import pytest

import chain_stats_reference as chain_ref
import commit_finality_reference as fin_ref
import commit_timeline_reference as timeline_ref
import commit_times_oracle as cto
import round_stats_reference as round_ref
import strided_shapes as S
from support import amd, check_chain_stats, check_finality, check_round_histograms, oracle_cfg, plain, same  # noqa: F401

pytestmark = pytest.mark.gpu
assert chain_ref.LDS_BINS == fin_ref.LDS_BINS == round_ref.LDS_BINS
BINNINGS = [(None, None), (7, 5), (1, 2 * chain_ref.LDS_BINS + 7)]  # the default; the last bin clamps; three LDS passes
QUANTILES = (0.0, 0.5, 0.9, 1.0)
THREE = {S.FAST: "fast", S.DEFAULT: "default", S.THIRD: "third"}  # the groups of 38


def layout_batch(amd, flavour, **kw):
    f = S.FLAVOURS[flavour]
    set_of, seeds = S.assignment(f["background"])
    return amd.BatchSimulator.with_param_sets(seeds, f["n"], S.param_sets(flavour), set_of, quirks=f["quirks"], **kw)


@pytest.fixture(scope="module")
def batches(amd):
    """get(flavour, timed) -> (sim, res): the clean layout batches, run once -- timed (commit times: chain statistics and finality) or
    traced (round statistics; a traced batch runs the class-1 kernels)."""
    made = {}

    def get(flavour, timed):
        if (flavour, timed) not in made:
            sim = layout_batch(amd, flavour, commit_times=True) if timed else layout_batch(amd, flavour)
            res = sim.loop_until(S.MAX_CLOCK) if timed else sim.loop_until(S.MAX_CLOCK, round_trace=S.ROUND_TRACE)
            assert (res.faults == 0).all(), np.nonzero(res.faults)[0]
            made[flavour, timed] = (sim, res)
        return made[flavour, timed]

    yield get
    for sim, _ in made.values():
        sim.close()


def empty_rows_are_zero(arrays, sizes):
    assert (sizes == 0).sum() > 10 and sizes[S.EMPTY_LAST] == 0
    for a in arrays:
        assert not a[sizes == 0].any() and a[sizes > 0].any()


def check_timed(res, want, max_clock, set_of=None, groups=1, faults=None, log_capacity=None, **rule):
    """Chain statistics against the reference on the oracle's histories `want`, finality against the reference on the read-backs, for
    every binning.  -> (chain families, finality families, the arrays of the last binning)."""
    c_fam, _, hist, authors, c_stats = check_chain_stats(res, want, max_clock, BINNINGS, set_of, groups, faults, log_capacity)
    f_fam, fin, spread, first, f_stats = check_finality(res, max_clock, BINNINGS, set_of=set_of, groups=groups, log_capacity=log_capacity, **rule)
    assert (res.chain_stats()[2] == c_stats).all() and (res.finality_histogram()[3] == f_stats).all()  # three passes: the default's statistics
    return c_fam, f_fam, (hist, authors, c_stats, fin, spread, first, f_stats)


def check_rounds(res, max_clock, set_of=None, groups=1):
    """Round statistics against the reference on the device's own tables, for every binning.  -> (tables, families, the last arrays)."""
    tables = res.round_tables()
    fam, stay, skew, stats = check_round_histograms(res, tables, max_clock, BINNINGS, set_of, groups)
    assert (res.round_histogram()[2] == stats).all()
    return tables, fam, (stay, skew, stats)


def tables_equal_the_oracles(oracle, tables, instances, cfg, seeds, max_clock):
    t, max_rounds, messages = tables
    t_o, max_rounds_o, messages_o = round_ref.oracle_tables(oracle, cfg, seeds, max_clock)
    assert (max_rounds[instances] == max_rounds_o).all() and (messages[instances] == messages_o).all()
    rows = t_o.shape[1]
    assert t.shape[1] >= rows and (t[instances][:, :rows] == t_o).all() and (t[instances][:, rows:] == round_ref.EMPTY).all()


def exact_quantiles(row, samples):
    for q in QUANTILES:
        assert row["quantiles"][str(q)] == int(np.quantile(samples, q, method="inverted_cdf")), q


# ---- A: 256 groups, clean ----
@pytest.mark.parametrize("flavour", ["class0", "partition"])
def test_a_chain_statistics_and_finality_of_256_groups(amd, oracle, batches, flavour):
    f = S.FLAVOURS[flavour]
    set_of, seeds, want = S.oracle_layout(oracle, flavour)
    sim, res = batches(flavour, True)
    assert sim.layout()["kernel_class"] & 0xff == (0 if flavour == "class0" else 1)
    c_fam, f_fam, arrays = check_timed(res, want, S.MAX_CLOCK, set_of, S.GROUPS)
    empty_rows_are_zero(arrays, S.group_sizes())
    assert c_fam[S.FAST][chain_ref.LENGTH].min() > 128 and c_fam[S.FAST][chain_ref.TENURE].max() > 1  # carries across the chunk seams, per trip
    c_rows, f_rows = res.chain_by_param_set(QUANTILES), res.finality_by_param_set(QUANTILES)
    for g, kind in THREE.items():  # 38 instances in ONE group do not stride: the group's rows are that plain batch's
        p = plain(amd, seeds[S.members(set_of, g)], f["n"], S.param_set(kind, flavour), quirks=f["quirks"], commit_times=True)
        pr = p.loop_until(S.MAX_CLOCK)
        assert same([a[0] for a in pr.chain_stats()], [a[g] for a in res.chain_stats()]), g
        assert same([a[0] for a in pr.finality_histogram()], [a[g] for a in res.finality_histogram()]), g
        assert pr.chain_by_param_set(QUANTILES)[0] == dict(c_rows[g], set=0) and pr.finality_by_param_set(QUANTILES)[0] == dict(f_rows[g], set=0)
        p.close()
        exact_quantiles(c_rows[g]["interval"], c_fam[g][chain_ref.INTERVAL])
        exact_quantiles(f_rows[g]["quorum"], f_fam[g][fin_ref.QUORUM])
        exact_quantiles(f_rows[g]["spread"], f_fam[g][fin_ref.SPREAD])
        assert c_rows[g]["length"]["instances"] == f_rows[g]["open"]["instances"] == 38
    if flavour == "partition":  # the partition does spread an entry's commits: the set matters on this data
        assert f_rows[S.THIRD]["spread"]["max"] > f_rows[S.DEFAULT]["spread"]["max"] + 100
    if flavour == "class0":  # the batch's other statistics, whose kernels do not stride this way: cheap cross-checks
        cto.check_default_latency(res, S.MAX_CLOCK, set_of, S.GROUPS)
        t_fam = timeline_ref.samples(res.commit_times(), res.commit_counts, res.faults, set_of, S.GROUPS, None, S.MAX_CLOCK)
        hist, stats = res.stall_histogram()
        want_hist, want_stats = timeline_ref.bin_stalls(t_fam, 1, S.MAX_CLOCK + 1)
        assert (hist == want_hist).all() and (stats == want_stats).all()


@pytest.mark.parametrize("flavour", ["class0", "partition"])
def test_a_round_statistics_of_256_groups(amd, oracle, batches, flavour):
    f = S.FLAVOURS[flavour]
    set_of, seeds = S.assignment()
    sim, res = batches(flavour, False)
    assert sim.layout()["kernel_class"] & 0xff == 1
    tables, fam, arrays = check_rounds(res, S.MAX_CLOCK, set_of, S.GROUPS)
    empty_rows_are_zero(arrays, S.group_sizes())
    for g in S.STRIDED:  # the tables the reference worked on are the oracle's, for every instance of the strided groups
        idx = S.members(set_of, g)
        cfg = oracle_cfg(oracle, f["n"], S.param_set(S.kind_of_group(g), flavour), quirks=f["quirks"])
        tables_equal_the_oracles(oracle, tables, idx, cfg, seeds[idx], S.MAX_CLOCK)
    assert int(tables[1][S.members(set_of, S.FAST)].min()) > 128  # three 64-round chunks, per trip
    rows = res.rounds_by_param_set(QUANTILES)
    for g, kind in THREE.items():
        p = plain(amd, seeds[S.members(set_of, g)], f["n"], S.param_set(kind, flavour), quirks=f["quirks"])
        pr = p.loop_until(S.MAX_CLOCK, round_trace=S.ROUND_TRACE)
        assert same([a[0] for a in pr.round_histogram()], [a[g] for a in res.round_histogram()]), g
        assert pr.rounds_by_param_set(QUANTILES)[0] == dict(rows[g], set=0)
        p.close()
        exact_quantiles(rows[g]["stay"], fam[g][round_ref.STAY])
        exact_quantiles(rows[g]["skew"], fam[g][round_ref.SKEW])
    if flavour == "partition":  # the cut-off node jumps rounds when it catches up
        assert fam[S.THIRD][round_ref.SKIPPED].max() > 0


# ---- B: the same layout, faulted and clean trips mixed ----
def test_b_mixed_faults(amd, oracle):
    set_of, seeds, want = S.oracle_layout(oracle, "class0")
    lcap, expected = S.fault_case(want, set_of)
    sizes = S.group_sizes()
    fast = S.members(set_of, S.FAST)
    whole = [g for g in range(S.GROUPS) if sizes[g] and (expected[S.members(set_of, g)] != 0).all()]
    assert whole and 0 < (expected[fast] != 0).sum() < len(fast)
    timed = layout_batch(amd, "class0", log_capacity=lcap, commit_times=True)
    res = timed.loop_until(S.MAX_CLOCK, allow_faults=True)
    assert timed.layout()["kernel_class"] & 0xff == 0
    assert (res.faults == expected).all(), np.nonzero(res.faults != expected)[0]  # the oracle-predicted fault words
    c_fam, f_fam, arrays = check_timed(res, want, S.MAX_CLOCK, set_of, S.GROUPS, faults=res.faults, log_capacity=lcap)
    for a in arrays:  # a group that is faulted throughout gives all-zero rows
        assert not a[whole].any() and a[S.FAST].any()
    clean = int((expected[fast] == 0).sum())
    assert arrays[2][S.FAST, 4 * chain_ref.LENGTH] == arrays[6][S.FAST, 4 * fin_ref.OPEN] == clean
    # the faulted instances do hold samples: the rule matters
    everyone = chain_ref.samples(*want, None, set_of, S.GROUPS, lcap)[0]
    assert len(everyone[S.FAST][chain_ref.INTERVAL]) > len(c_fam[S.FAST][chain_ref.INTERVAL]) == arrays[2][S.FAST, 0]
    lost = fast[expected[fast] != 0]
    ct = res.commit_times()
    skipped = fin_ref.samples(ct[lost], res.commit_counts[lost], res.committed_histories(ct.shape[2])[lost], res.startup_times[lost], None, None, 0,
                              30000, None, 1, lcap)[0][0]
    assert len(skipped[fin_ref.QUORUM]) > 100 * len(lost)
    timed.close()
    traced = layout_batch(amd, "class0", log_capacity=lcap)
    rt = traced.loop_until(S.MAX_CLOCK, allow_faults=True, round_trace=S.ROUND_TRACE)
    assert (rt.faults == expected).all()
    tables, fam, r_arrays = check_rounds(rt, S.MAX_CLOCK, set_of, S.GROUPS)
    for a in r_arrays:
        assert not a[whole].any() and a[S.FAST].any()
    r_everyone = round_ref.samples(tables[0], tables[1], None, set_of, S.GROUPS)
    assert len(r_everyone[S.FAST][round_ref.STAY]) > len(fam[S.FAST][round_ref.STAY]) == r_arrays[2][S.FAST, 0]
    traced.close()


# ---- C: 64-wide tiles ----
def test_c_tiles_of_seven_nodes_with_loss(amd, oracle):
    set_of, seeds, want = S.oracle_layout(oracle, "tiles")
    sizes = S.group_sizes(False)
    timed = layout_batch(amd, "tiles", commit_times=True)
    res = timed.loop_until(S.MAX_CLOCK)
    assert timed.layout()["kernel_class"] & 0xff == 1 and (res.faults == 0).all()
    c_fam, f_fam, arrays = check_timed(res, want, S.MAX_CLOCK, set_of, S.GROUPS)
    empty_rows_are_zero(arrays, sizes)
    assert np.median(c_fam[S.FAST][chain_ref.LENGTH]) > 128 and len(f_fam[S.THIRD][fin_ref.ALL]) > 0
    timed.close()
    traced = layout_batch(amd, "tiles")
    rt = traced.loop_until(S.MAX_CLOCK, round_trace=S.ROUND_TRACE)
    assert traced.layout()["kernel_class"] & 0xff == 1 and (rt.faults == 0).all()
    tables, fam, r_arrays = check_rounds(rt, S.MAX_CLOCK, set_of, S.GROUPS)
    empty_rows_are_zero(r_arrays, sizes)
    idx = S.members(set_of, S.G17)  # (the oracle's 7-node tables take their time: the group whose one wavefront strides)
    tables_equal_the_oracles(oracle, tables, idx, oracle_cfg(oracle, 7, S.param_set(S.kind_of_group(S.G17), "tiles"), quirks=3), seeds[idx], S.MAX_CLOCK)
    traced.close()


# ---- D: plain batches of 4102 instances, grp_inst == NULL ----
@pytest.mark.parametrize("shape", [S.PLAIN, S.WEIGHTED], ids=["unit_rights", "rotating_weighted_rights"])
def test_d_plain_batch_of_4102_instances(amd, oracle, shape):
    n, max_clock, kw = shape["n"], shape["max_clock"], shape["kw"]
    seeds, want = S.oracle_plain(oracle, shape)
    ps = amd.ParamSet()
    rule = dict(rights=kw["voting_rights"], rotation=kw["rights_rotation"], commands_per_epoch=kw["commands_per_epoch"]) if kw else {}
    timed = plain(amd, seeds, n, ps, commit_times=True, **kw)
    res = timed.loop_until(max_clock)
    assert (res.faults == 0).all() and (res.commit_counts == want[1]).all()
    if kw:  # the rights matter on this data: under unit rights the quorum times are others
        weighted, unit = fin_ref.of_result(res, **rule)[0][0][fin_ref.QUORUM], fin_ref.of_result(res)[0][0][fin_ref.QUORUM]
        assert len(weighted) != len(unit) or (weighted != unit).any()
        assert res.epochs.min() >= 2 and res.epochs.max() >= 3  # the rights rotated, more than once
    c_fam, _, arrays = check_timed(res, want, max_clock, **rule)
    assert arrays[2][0, 4 * chain_ref.LENGTH] == arrays[6][0, 4 * fin_ref.OPEN] == shape["m"]  # every instance, whichever trip took it
    timed.close()
    traced = plain(amd, seeds, n, ps, **kw)
    rt = traced.loop_until(max_clock, round_trace=S.ROUND_TRACE)
    assert (rt.faults == 0).all()
    tables, _, _ = check_rounds(rt, max_clock)
    idx = np.r_[0:8, 4096:shape["m"]]  # workgroups 0 and 1: both trips of the wavefronts that make two
    tables_equal_the_oracles(oracle, tables, idx, oracle_cfg(oracle, n, ps, **kw), seeds[idx], max_clock)
    traced.close()


# ---- E: repeated calls ----
def test_e_repeated_and_interleaved_calls(batches):
    _, res = batches("class0", True)
    chain = lambda: list(res.chain_stats()) + list(res.chain_stats(7, 5))  # noqa: E731
    finality = lambda: list(res.finality_histogram()) + list(res.finality_histogram(1, 2 * fin_ref.LDS_BINS + 7))  # noqa: E731
    c, f = chain(), finality()
    assert same(c, chain()) and same(f, finality())  # two calls: identical arrays
    again = finality()
    chain()
    assert same(again, finality()) and same(f, again)  # a call of one statistic between two calls of another changes nothing
    res.latency_histogram()
    assert same(c, chain())
    _, rt = batches("class0", False)
    rounds = lambda: list(rt.round_histogram()) + list(rt.round_histogram(7, 5)) + list(rt.round_tables())  # noqa: E731
    r = rounds()
    rt.chain_stats()
    assert same(r, rounds())
