"""Round statistics on the device (BatchResult.round_tables / round_histogram / rounds_by_param_set, lbft_k_rs_rounds) against the oracle:
in every case round_tables() equals the oracle's round_switches() for every instance, and round_histogram() equals the numpy reference of
the definitions (tests/round_stats_reference.py) evaluated on the ORACLE's tables and the device's fault words -- on a mid-class network
whose cut-off node jumps rounds, a parameter-set batch with interleaved sets, a large-class batch with instance-major rows, a lossy
network whose rounds not every node enters, on tables three 64-round chunks deep with a jump over a chunk seam, at the binnings' edges, with instances that overflowed the trace, through reset, run_steps
and a checkpoint, at the calls' refusals and through the grid tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import round_stats_reference as ref
from support import amd, oracle_cfg, plain, same  # noqa: F401
from support import check_round_histograms as check_histograms, check_round_tables as check_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
TRACE_OVERFLOW = 1 << 11  # LBFT_FAULT_TRACE_OVERFLOW


# ---- case 1: class 1, a node that jumps rounds ----
JUMPS = dict(n=4, quirks=3, partition=(1, 300, 600), max_clock=1000, seeds=np.arange(1, 17, dtype=np.uint64))


@pytest.fixture(scope="module")
def jumps_oracle(amd, oracle):
    ps = amd.ParamSet(partition=JUMPS["partition"])
    return ref.oracle_tables(oracle, oracle_cfg(oracle, JUMPS["n"], ps, quirks=JUMPS["quirks"]), JUMPS["seeds"], JUMPS["max_clock"])


def jumps_batch(amd):
    return plain(amd, JUMPS["seeds"], JUMPS["n"], amd.ParamSet(partition=JUMPS["partition"]), quirks=JUMPS["quirks"])


@pytest.fixture(scope="module")
def jumps(amd):
    sim = jumps_batch(amd)
    res = sim.loop_until(JUMPS["max_clock"], round_trace=JUMPS["max_clock"] + 64)
    yield sim, res
    sim.close()


def test_mid_class_network_whose_cut_off_node_jumps_rounds(jumps, jumps_oracle):
    sim, res = jumps
    assert sim.layout()["kernel_class"] & 0xff == 1 and (res.faults == 0).all()
    tables, _, _ = check_tables(res, jumps_oracle)
    for i in (0, 7, 15):  # the bulk read-back is the single one
        rows, messages = res.round_switches(i)
        assert [[ref.EMPTY if v is None else v for v in row] for row in rows] == tables[i, :len(rows)].tolist()
    fam, stay, skew, stats = check_histograms(res, jumps_oracle, JUMPS["max_clock"], [(None, None)])
    # (the oracle's own tables hold what this case is about: jumps, rounds not every node entered, a zero stay)
    assert (fam[0][ref.SKIPPED] > 0).any() and (fam[0][ref.REACH] < JUMPS["n"]).any() and (fam[0][ref.STAY] == 0).any()
    assert stats[0, 0] == stats[0, 4] == len(fam[0][ref.STAY]) and stats[0, 7] == fam[0][ref.SKIPPED].max() > 0
    assert stay.sum() == stats[0, 0] and skew.sum() == stats[0, 8]
    # an explicit cap: fewer rows than the tables have, and more
    for cap in (5, 40, 0):
        t, mr, _ = res.round_tables(cap)
        assert t.shape == (16, cap, 4) and (mr == jumps_oracle[1]).all()
        k = min(cap, tables.shape[1])
        assert (t[:, :k] == tables[:, :k]).all() and (t[:, k:] == ref.EMPTY).all()


# ---- case 2: parameter sets, interleaved ----
def test_parameter_sets_interleaved(amd, oracle):
    n, per, max_clock = 7, 8, 600
    sets = [amd.ParamSet(), amd.ParamSet(partition=(2, 100, 400)), amd.ParamSet(drop_per_million=50000)]
    from librabft_simulator_amd import grid
    set_of, seed_index = grid.set_assignment(len(sets), per, "interleaved")
    seeds = (1 + seed_index).astype(np.uint64)
    per_set = [ref.oracle_tables(oracle, oracle_cfg(oracle, n, ps, quirks=3), np.arange(1, per + 1), max_clock) for ps in sets]
    rows = max(t.shape[1] for t, _, _ in per_set)
    tables_o = np.full((len(set_of), rows, n), ref.EMPTY, dtype=np.int64)
    max_rounds_o = np.zeros(len(set_of), dtype=np.uint64)
    messages_o = np.zeros(len(set_of), dtype=np.uint64)
    for k, (t, mr, msgs) in enumerate(per_set):
        tables_o[set_of == k, :t.shape[1]], max_rounds_o[set_of == k], messages_o[set_of == k] = t, mr, msgs
    want = (tables_o, max_rounds_o, messages_o)
    sim = amd.BatchSimulator.with_param_sets(seeds, n, sets, set_of, quirks=3)
    res = sim.loop_until(max_clock, round_trace=256)
    assert sim.layout()["kernel_class"] & 65536 and (res.faults == 0).all()
    check_tables(res, want)
    fam, stay, skew, stats = check_histograms(res, want, max_clock, [(3, 40), (None, None)], set_of, len(sets))
    assert (fam[1][ref.SKIPPED] > 0).any() and not (fam[0][ref.SKIPPED] > 0).any()  # the partition set's nodes jump, the control's do not
    assert (stats[:, 0] > 0).all() and len({tuple(r) for r in stats.tolist()}) == len(sets)
    summary = res.rounds_by_param_set((0.0, 0.5, 1.0))
    for k, ps in enumerate(sets):  # every group row is the plain batch of that set
        p = plain(amd, np.arange(1, per + 1), n, ps, quirks=3)
        pr = p.loop_until(max_clock, round_trace=256)
        p_stay, p_skew, p_stats = pr.round_histogram()
        assert (p_stay[0] == stay[k]).all() and (p_skew[0] == skew[k]).all() and (p_stats[0] == stats[k]).all(), k
        assert (pr.round_tables(rows)[0] == tables_o[set_of == k]).all()
        assert pr.rounds_by_param_set((0.0, 0.5, 1.0))[0] == dict(summary[k], set=0)
        p.close()
        for f, name in enumerate(("stay", "skipped", "skew", "reach")):
            s = fam[k][f]
            assert summary[k][name]["samples"] == len(s) and summary[k][name]["min"] == s.min() and summary[k][name]["max"] == s.max()
            assert summary[k][name]["mean"] == pytest.approx(s.mean(), rel=1e-12)
        for name, f in (("stay", ref.STAY), ("skew", ref.SKEW)):
            for q in (0.0, 0.5, 1.0):
                assert summary[k][name]["quantiles"][str(q)] == int(np.quantile(fam[k][f], q, method="inverted_cdf")), (k, name, q)
    sim.close()


# ---- case 3: class 2, instance-major rows ----
def test_large_class_with_instance_major_rows(amd, oracle):
    n, max_clock, seeds = 40, 300, np.arange(1, 9, dtype=np.uint64)
    want = ref.oracle_tables(oracle, oracle_cfg(oracle, n, amd.ParamSet()), seeds, max_clock)
    sim = plain(amd, seeds, n, amd.ParamSet())
    res = sim.loop_until(max_clock, round_trace=128)
    assert sim.layout()["kernel_class"] & 0xff == 2 and (res.faults == 0).all()
    check_tables(res, want)
    fam, _, _, stats = check_histograms(res, want, max_clock, [(None, None), (2, 5)])
    assert fam[0][ref.REACH].min() == fam[0][ref.REACH].max() == n and stats[0, 8] == int(want[1].sum()) - len(seeds)  # every row >= 1 has a skew
    sim.close()


# ---- case 4: rounds that not every node enters ----
def test_lossy_network_reach_below_n(amd, oracle):
    n, max_clock, seeds = 16, 1000, np.arange(1, 33, dtype=np.uint64)
    ps = amd.ParamSet(drop_per_million=20000)
    want = ref.oracle_tables(oracle, oracle_cfg(oracle, n, ps), seeds, max_clock)
    sim = plain(amd, seeds, n, ps)
    res = sim.loop_until(max_clock, round_trace=264)
    assert sim.layout()["kernel_class"] & 0xff == 1 and (res.faults == 0).all()
    check_tables(res, want)
    fam, _, _, _ = check_histograms(res, want, max_clock, [(None, None)])
    assert fam[0][ref.REACH].min() < n and fam[0][ref.REACH].max() == n
    sim.close()


# ---- tables deeper than the 64 rounds a wavefront takes at a time ----
def seam_pairs(tables, max_rounds, seam):
    """(instance, node, round, next round) of a node's consecutive recorded rounds that lie on both sides of row `seam` with rounds
    jumped over between them: the predecessor of such a cell comes out of the previous 64-round chunk, not out of its own."""
    out = []
    for i in range(len(max_rounds)):
        for j in range(tables.shape[2]):
            r = np.nonzero(tables[i, :int(max_rounds[i]), j] != ref.EMPTY)[0]
            out += [(i, j, int(a), int(b)) for a, b in zip(r[:-1], r[1:]) if a < seam <= b and b - a > 1]
    return out


@pytest.mark.parametrize("partition,seam", [((1, 1500, 1800), 64), ((1, 3000, 3400), 128)])
def test_tables_of_three_chunks_with_a_jump_over_a_chunk_seam(amd, oracle, partition, seam):
    # 4 nodes to clock 5000 are 175 to 195 rounds deep: three chunks of 64 rounds; node 0, cut off while the others pass round `seam`,
    # jumps over that row when it catches up
    n, max_clock, seeds = 4, 5000, np.arange(1, 9, dtype=np.uint64)
    ps = amd.ParamSet(partition=partition)
    want = ref.oracle_tables(oracle, oracle_cfg(oracle, n, ps, quirks=3), seeds, max_clock)
    assert int(want[1].min()) > 128 and seam_pairs(want[0], want[1], seam)
    sim = plain(amd, seeds, n, ps, quirks=3)
    res = sim.loop_until(max_clock, round_trace=256)
    assert sim.layout()["kernel_class"] & 0xff == 1 and (res.faults == 0).all()
    _, max_rounds, _ = check_tables(res, want)
    assert int(max_rounds.min()) > 128
    fam, _, _, stats = check_histograms(res, want, max_clock, [(None, None), (7, 5)])
    assert stats[0, 7] == fam[0][ref.SKIPPED].max() > 0
    sim.close()


def test_instance_major_rows_deeper_than_one_chunk(amd, oracle):
    n, max_clock, seeds = 40, 1900, np.arange(1, 2, dtype=np.uint64)
    want = ref.oracle_tables(oracle, oracle_cfg(oracle, n, amd.ParamSet()), seeds, max_clock)
    assert int(want[1].min()) > 64
    sim = plain(amd, seeds, n, amd.ParamSet())
    res = sim.loop_until(max_clock, round_trace=128)
    assert sim.layout()["kernel_class"] & 0xff == 2 and (res.faults == 0).all()
    check_tables(res, want)
    check_histograms(res, want, max_clock, [(None, None)])
    sim.close()


# ---- case 5: binning ----
def test_binnings(jumps, jumps_oracle):
    _, res = jumps
    fam, stay, skew, _ = check_histograms(res, jumps_oracle, JUMPS["max_clock"],
                                          [(7, 5), (1, ref.LDS_BINS + 1), (1, 1), (2 ** 32 - 1, 3), (1, 2 * ref.LDS_BINS + 7), (None, 10), (None, None)])
    clamp = res.round_histogram(7, 5)
    assert clamp[0][0, -1] == (fam[0][ref.STAY] >= 28).sum() > 0 and clamp[1][0, -1] == (fam[0][ref.SKEW] >= 28).sum() > 0
    assert stay.shape == (1, JUMPS["max_clock"] + 1)


# ---- case 6: instances that overflowed the trace are skipped ----
def test_faulted_instances_are_skipped(amd, jumps_oracle):
    tables_o, max_rounds_o, _ = jumps_oracle
    cap = int(np.median(max_rounds_o))  # (an instance overflows when a node passes round `cap`)
    assert 0 < (max_rounds_o > cap).sum() < len(max_rounds_o)
    sim = jumps_batch(amd)
    res = sim.loop_until(JUMPS["max_clock"], allow_faults=True, round_trace=cap)
    faulted = res.faults != 0
    assert (faulted == (max_rounds_o > cap)).all() and 0 < faulted.sum() < len(faulted)
    assert (res.faults[faulted] == TRACE_OVERFLOW).all()
    check_tables(res, jumps_oracle, clean=~faulted)
    tables, max_rounds, _ = res.round_tables()
    assert (max_rounds == max_rounds_o).all() and tables.shape[1] == int(max_rounds_o.max())
    assert (tables[:, :cap] == tables_o[:, :cap]).all() and (tables[faulted][:, cap:] == ref.EMPTY).all()  # a faulted instance keeps `cap` rows
    fam, stay, _, stats = check_histograms(res, jumps_oracle, JUMPS["max_clock"], [(None, None), (10, 20)])
    everyone = ref.samples(tables_o, max_rounds_o, None, None, 1)
    assert len(everyone[0][ref.STAY]) > len(fam[0][ref.STAY]) == stats[0, 0]  # (the faulted instances do hold cells: the rule matters)
    sim.close()


# ---- case 7: lifecycle ----
def arrays(res):
    return list(res.round_tables()) + list(res.round_histogram()) + list(res.round_histogram(9, 30))


def test_reset_steps_and_checkpoint_give_the_same_arrays(amd, jumps, tmp_path):
    from librabft_simulator_amd import _lib
    sim, res = jumps
    mc, trace = JUMPS["max_clock"], JUMPS["max_clock"] + 64
    want = arrays(res)
    assert same(want, arrays(res))  # two calls: identical arrays
    again = jumps_batch(amd)
    r1 = again.loop_until(mc, round_trace=trace)
    assert same(want, arrays(r1))
    again.reset()
    assert same(want, arrays(again.loop_until(mc, round_trace=trace)))
    again.close()
    a = jumps_batch(amd)
    _lib.check(_lib.lib().lbft_batch_enable_round_trace(a._h, trace))
    left, _ = a.run_steps(mc, 200)
    assert left > 0
    with pytest.raises(amd.LbftError) as e:  # (an unfinished run is no finished run)
        amd.BatchResult(a).round_histogram()
    assert e.value.code == _lib.LBFT_ERR_STATE
    a.save_checkpoint(str(tmp_path / "ck.bin"))
    a.close()
    b = jumps_batch(amd)
    b.load_checkpoint(str(tmp_path / "ck.bin"))
    done = None
    for _ in range(10000):
        left, done = b.run_steps(mc, 200)
        if left == 0:
            break
    assert done is not None and same(want, arrays(done))
    b.close()


# ---- case 8: refusals ----
def test_refusals(amd, jumps):
    from librabft_simulator_amd import _lib
    calls = (lambda r: r.round_histogram(), lambda r: r.round_tables(), lambda r: r.round_tables(4), lambda r: r.rounds_by_param_set())
    untraced = jumps_batch(amd)
    for call in calls:  # before the run
        with pytest.raises(amd.LbftError) as e:
            call(amd.BatchResult(untraced))
        assert e.value.code == _lib.LBFT_ERR_STATE
    ru = untraced.loop_until(300)
    for call in calls:  # a batch without the trace
        with pytest.raises(amd.LbftError) as e:
            call(ru)
        assert e.value.code == _lib.LBFT_ERR_STATE
    untraced.close()
    sim, res = jumps
    L = _lib.lib()
    stay, skew, stats = np.full(8, 7, dtype=np.uint64), np.full(8, 7, dtype=np.uint64), np.full(16, 7, dtype=np.uint64)
    p = [a.ctypes.data for a in (stay, skew, stats)]
    assert L.lbft_batch_round_stats(sim._h, 1, 0, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_round_stats(sim._h, 0, 8, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_round_stats(sim._h, 1, 2 ** 31 + 1, *p) == _lib.LBFT_ERR_INVALID  # groups x bins > 2^31
    assert L.lbft_batch_round_stats(sim._h, 1, 8, p[0], None, p[2]) == _lib.LBFT_ERR_INVALID
    assert (stay == 7).all() and (skew == 7).all() and (stats == 7).all()
    with pytest.raises(ValueError):
        res.round_histogram(bins=0)


# ---- case 9: the grid tool ----
def test_grid_cli_rounds(amd):
    args = ["--nodes", "4", "--delta", "10,20", "--lambda", "0.25,0.75", "--seeds-per-point", "16", "--max-clock", "500", "--assign", "interleaved"]
    out = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid", "--rounds"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.strip()]
    assert [(l["delta"], l["lambda"]) for l in lines] == [(10, 0.25), (10, 0.75), (20, 0.25), (20, 0.75)]
    from librabft_simulator_amd import grid
    sets = [amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, d, 2.0, lam)) for d in (10, 20) for lam in (0.25, 0.75)]
    set_of, seed_index = grid.set_assignment(4, 16, "interleaved")
    sim = amd.BatchSimulator.with_param_sets((1 + seed_index).astype(np.uint64), 4, sets, set_of)
    res = sim.loop_until(500, allow_faults=True, round_trace=grid.round_trace_capacity(500, None))
    _, _, stats = res.round_histogram()
    for k, l in enumerate(lines):
        assert set(l["round_stats"]) == {"set", "stay", "skipped", "skew", "reach"} and l["faulted"] == 0
        assert [l["round_stats"][name]["samples"] for name in ("stay", "skipped", "skew", "reach")] == stats[k, 0::4].tolist()
        assert l["round_stats"]["stay"]["samples"] > 0 and l["round_stats"]["reach"]["samples"] > 0
    assert [l["round_stats"] for l in lines] == json.loads(json.dumps(res.rounds_by_param_set()))
    # the summary is one more key: the line's other fields, the final active round's "rounds" among them, are what they are without it
    assert [l["rounds"] for l in lines] == json.loads(json.dumps([row["rounds"] for row in res.by_param_set()]))
    assert all(set(l["rounds"]) == {"mean", "min", "max"} for l in lines)
    bare = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bare.returncode == 0, bare.stderr[-2000:]
    assert [{k: v for k, v in l.items() if k != "round_stats"} for l in lines] == [json.loads(l) for l in bare.stdout.splitlines() if l.strip()]
    sim.close()
