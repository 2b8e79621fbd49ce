"""Chain statistics on the device (BatchResult.chain_stats / chain_by_param_set, lbft_k_cs_chain) against the oracle: in every case the
device's arrays equal the numpy reference of the definitions (tests/chain_stats_reference.py) evaluated on the ORACLE's histories, commit
counts and startup times -- fault words come from the device only where a case provokes a capacity fault.  The shapes are the smallest
that reach each mechanism: chains of three 64-entry chunks, of less than one and of none at all on instance-major class-0 rows, the
headline batch shape, 64-wide tiles with a partial tile, networks of 33 and 65 nodes (the node pass's second round), weighted rights and
epoch changes, parameter sets with an unused set and instances that overflowed their logs, timed and traced batches, the binnings' edges,
repeated calls, reset, stepping and checkpoints, the refusals and the grid tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_stats_reference as ref
from support import amd, oracle_cfg, plain, same  # noqa: F401
from support import check_chain_stats as check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
LOG_OVERFLOW = 1 << 3  # LBFT_FAULT_LOG_OVERFLOW


def arrays(res):
    return list(res.chain_stats()) + list(res.chain_stats(7, 30))


# ---- class 0, instance-major rows ----
SMALL = dict(n=4, seeds=np.arange(1, 97, dtype=np.uint64))


@pytest.mark.parametrize("max_clock", [4000, 300, 0, 20])
def test_class_0_chains_of_three_chunks_of_less_than_one_and_of_none(amd, oracle, max_clock):
    ps = amd.ParamSet()
    want = ref.oracle_batch(oracle, oracle_cfg(oracle, SMALL["n"], ps), SMALL["seeds"], max_clock)
    sim = plain(amd, SMALL["seeds"], SMALL["n"], ps)
    res = sim.loop_until(max_clock)
    assert sim.layout()["kernel_class"] & 0xff == 0 and (res.faults == 0).all()
    binnings = [(None, None), (1, 5000), (1, 2 * ref.LDS_BINS + 7), (7, None), (1, 1), (None, 10)] if max_clock == 4000 else [(None, None), (7, 5), (1, 1)]
    fam, authors_o, hist, _, stats = check(res, want, max_clock, binnings)
    f = fam[0]
    if max_clock == 4000:  # three chunks: carries and tenure runs across the seams of 64 entries
        assert f[ref.LENGTH].min() > 128 and f[ref.TENURE].max() > 1 and f[ref.LAG].max() > 0
        every = arrays(res)
        assert same(every, arrays(res))  # two calls: identical arrays
        clamp = res.chain_stats(7, 5)[0]
        assert clamp[0, -1] == (f[ref.INTERVAL] >= 28).sum() > 0  # the last bin also counts everything above it
        one = res.chain_stats(1, 1)
        assert one[0][0, 0] == len(f[ref.INTERVAL]) and (one[2] == stats).all()  # the binning leaves the statistics as they are
    elif max_clock == 300:
        assert 0 < f[ref.LENGTH].min() and f[ref.LENGTH].max() < 64
    else:  # no commit anywhere: L = 0, one length and n lag samples per instance, no interval, no tenure
        assert stats[0].tolist() == [0, 0, 0, 0, 96, 0, 0, 0, 96 * 4, 0, 0, 0, 0, 0, 0, 0, 96, 0, 0, 0, 96, 0, 0, 0]
        assert not hist.any() and res.chain_by_param_set()[0]["author_share"] is None
    sim.close()


def test_headline_batch_shape(amd, oracle):
    n, max_clock, seeds = 4, 1000, np.arange(1, 1025, dtype=np.uint64)
    ps = amd.ParamSet()
    want = ref.oracle_batch(oracle, oracle_cfg(oracle, n, ps), seeds, max_clock)
    sim = plain(amd, seeds, n, ps)
    res = sim.loop_until(max_clock)
    assert sim.layout()["kernel_class"] & 0xff == 0 and (res.faults == 0).all()
    check(res, want, max_clock)
    sim.close()


# ---- class 1, 64-wide tiles: one full tile and a partial one ----
def test_mid_class_tiles_with_equivocators_and_loss(amd, oracle):
    n, max_clock, seeds = 7, 1000, np.arange(1, 71, dtype=np.uint64)
    ps = amd.ParamSet(drop_per_million=50000)
    want = ref.oracle_batch(oracle, oracle_cfg(oracle, n, ps, quirks=3, equivocate_every=3), seeds, max_clock)
    sim = plain(amd, seeds, n, ps, quirks=3, equivocate_every=3)
    res = sim.loop_until(max_clock)
    assert sim.layout()["kernel_class"] & 0xff == 1 and (res.faults == 0).all()
    fam, authors_o, _, _, _ = check(res, want, max_clock, [(None, None), (3, 40)])
    assert authors_o[0, [0, 3, 6]].sum() * 10 < authors_o[0].sum()  # whose blocks end up in the chain: hardly the equivocators'
    sim.close()


# ---- large networks, tile width 1 ----
@pytest.mark.parametrize("n,max_clock,quirks", [(33, 400, 0), (33, 400, 3), (65, 300, 0), (65, 300, 3)])
def test_large_networks(amd, oracle, n, max_clock, quirks):
    seeds = np.arange(1, 3, dtype=np.uint64)
    ps = amd.ParamSet()
    want = ref.oracle_batch(oracle, oracle_cfg(oracle, n, ps, quirks=quirks), seeds, max_clock, threads=2)
    sim = plain(amd, seeds, n, ps, quirks=quirks)
    res = sim.loop_until(max_clock)
    assert sim.layout()["kernel_class"] & 0xff == 2 and (res.faults == 0).all()
    fam, _, _, _, stats = check(res, want, max_clock, [(None, None), (2, 5)])
    assert stats[0, 4 * ref.LAG] == 2 * n and fam[0][ref.LENGTH].min() > 0
    sim.close()


# ---- weighted rights and epochs ----
@pytest.mark.parametrize("max_clock,kw", [(1000, {}), (1500, dict(commands_per_epoch=3, rights_rotation=1, quirks=3))])
def test_weighted_rights_and_epoch_changes(amd, oracle, max_clock, kw):
    n, seeds, rights = 5, np.arange(1, 9, dtype=np.uint64), [5, 1, 1, 1, 1]
    ps = amd.ParamSet()
    want = ref.oracle_batch(oracle, oracle_cfg(oracle, n, ps, voting_rights=rights, **kw), seeds, max_clock)
    sim = plain(amd, seeds, n, ps, voting_rights=rights, **kw)
    res = sim.loop_until(max_clock)
    assert (res.faults == 0).all()
    _, authors_o, _, authors, _ = check(res, want, max_clock)
    if not kw:  # the node with five of nine votes leads, and authors, most
        assert authors[0, 0] > authors[0, 1:].max()
        share = res.chain_by_param_set()[0]["author_share"]
        assert share == [int(v) / int(authors[0].sum()) for v in authors[0]] and abs(sum(share) - 1) < 1e-12
    sim.close()


# ---- parameter sets: unequal sizes, a set nobody uses, instances that overflowed their logs ----
def param_set_case(amd):
    sets = [amd.ParamSet(), amd.ParamSet(amd.RandomDelay.new(20.0, 9.0)), amd.ParamSet(amd.RandomDelay.new(3.0, 1.0)), amd.ParamSet(drop_per_million=10000)]
    set_of = np.array([0, 2, 1, 0, 2, 0, 1, 2, 0, 1, 2, 0, 0], dtype=np.uint32)  # 6, 3 and 4 instances; set 3 is unused
    seeds = np.arange(1, len(set_of) + 1, dtype=np.uint64)
    return sets, set_of, seeds


def test_parameter_sets_with_an_unused_set_and_log_overflows(amd, oracle):
    n, max_clock, lcap = 4, 1000, 64
    sets, set_of, seeds = param_set_case(amd)
    parts, order = [], []
    for k, ps in enumerate(sets):
        idx = np.nonzero(set_of == k)[0]
        if len(idx):
            parts.append(ref.oracle_batch(oracle, oracle_cfg(oracle, n, ps), seeds[idx], max_clock))
            order.append(idx)
    back = np.argsort(np.concatenate(order))
    want = tuple(a[back] for a in ref.concat(parts))
    counts = want[1]
    outgrown = counts.max(axis=1) > lcap  # only the fast set's instances outgrow a log of 64 entries
    assert (outgrown == (set_of == 2)).all() and counts[~outgrown].max() <= lcap
    # on the CPU first: with those fault words the reference is defined (it never looks at a skipped instance's rows past the capacity)
    expected_faults = np.where(outgrown, LOG_OVERFLOW, 0).astype(np.uint32)
    ref.chain_stats(*want, expected_faults, set_of, len(sets), 1, max_clock + 1, log_capacity=lcap)
    sim = amd.BatchSimulator.with_param_sets(seeds, n, sets, set_of, log_capacity=lcap)
    from librabft_simulator_amd import _lib
    with pytest.raises(amd.LbftError) as e:  # the run reports the faults
        sim.loop_until(max_clock)
    assert e.value.code == _lib.LBFT_ERR_FAULT
    res = amd.BatchResult(sim)
    assert (res.faults == expected_faults).all(), res.faults
    fam, _, hist, authors, stats = check(res, want, max_clock, [(None, None), (5, 20)], set_of, len(sets), faults=res.faults, log_capacity=lcap)
    assert not stats[2].any() and not stats[3].any() and not authors[2:].any() and not hist[2:].any()  # all faulted; unused
    assert stats[0, 4 * ref.LENGTH] == 6 and stats[1, 4 * ref.LENGTH] == 3 and stats[1, 1] / stats[1, 0] > stats[0, 1] / stats[0, 0]
    rows = res.chain_by_param_set((0.0, 0.5, 1.0))
    assert [r["set"] for r in rows] == [0, 1, 2, 3] and rows[3]["author_share"] is None and rows[3]["interval"]["mean"] is None
    for k in (0, 1):  # every group row is the plain batch of that set
        p = plain(amd, seeds[set_of == k], n, sets[k])
        pr = p.loop_until(max_clock)
        assert same([a[0] for a in pr.chain_stats()], [a[k] for a in res.chain_stats()])
        assert pr.chain_by_param_set((0.0, 0.5, 1.0))[0] == dict(rows[k], set=0)
        p.close()
        for f, (name, key) in enumerate((("interval", "samples"), ("length", "instances"), ("lag", "nodes"), ("tenure", "runs"),
                                         ("differing", "instances"), ("inversions", "instances"))):
            s = fam[k][f]
            assert rows[k][name][key] == len(s) and rows[k][name]["min"] == s.min() and rows[k][name]["max"] == s.max()
            assert rows[k][name]["mean"] == pytest.approx(s.mean(), rel=1e-12)
        for q in (0.0, 0.5, 1.0):
            assert rows[k]["interval"]["quantiles"][str(q)] == int(np.quantile(fam[k][ref.INTERVAL], q, method="inverted_cdf")), (k, q)
        assert rows[k]["authors"] == authors[k].tolist()
    sim.close()


# ---- timed and traced batches ----
def test_timed_and_traced_batches_give_the_plain_batch_statistics(amd, oracle):
    n, max_clock, seeds = 4, 600, np.arange(1, 33, dtype=np.uint64)
    ps = amd.ParamSet(partition=(1, 200, 400))
    want = ref.oracle_batch(oracle, oracle_cfg(oracle, n, ps, quirks=3), seeds, max_clock)
    base = plain(amd, seeds, n, ps, quirks=3)
    res = base.loop_until(max_clock)
    check(res, want, max_clock)
    mine = arrays(res)
    timed = plain(amd, seeds, n, ps, quirks=3, commit_times=True)
    rt = timed.loop_until(max_clock)
    assert timed.layout()["kernel_class"] & (1 << 17) and same(mine, arrays(rt))
    rt.latency_histogram()  # the other statistics of the batch are untouched by the call, and the other way round
    assert same(mine, arrays(rt))
    traced = plain(amd, seeds, n, ps, quirks=3)
    assert same(mine, arrays(traced.loop_until(max_clock, round_trace=256)))
    for s in (base, timed, traced):
        s.close()


# ---- lifecycle: reset, steps, checkpoint, a node-level session ----
def test_reset_steps_checkpoint_and_manual_sessions(amd, tmp_path):
    from librabft_simulator_amd import _lib
    n, max_clock, seeds = 4, 500, np.arange(1, 17, dtype=np.uint64)
    ps = amd.ParamSet()
    sim = plain(amd, seeds, n, ps)
    for call in (lambda r: r.chain_stats(), lambda r: r.chain_by_param_set()):  # before the run
        with pytest.raises(amd.LbftError) as e:
            call(amd.BatchResult(sim))
        assert e.value.code == _lib.LBFT_ERR_STATE
    res = sim.loop_until(max_clock)
    want = arrays(res)
    counts = res.commit_counts.copy()
    assert same(want, arrays(res)) and (res.commit_counts == counts).all()  # the call changes no state: the caches stay valid
    sim.reset()
    with pytest.raises(amd.LbftError) as e:  # between reset() and the next run
        amd.BatchResult(sim).chain_stats()
    assert e.value.code == _lib.LBFT_ERR_STATE
    assert same(want, arrays(sim.loop_until(max_clock)))
    sim.close()
    a = plain(amd, seeds, n, ps)
    left, _ = a.run_steps(max_clock, 150)
    assert left > 0
    with pytest.raises(amd.LbftError) as e:  # (an unfinished run is no finished run)
        amd.BatchResult(a).chain_stats()
    assert e.value.code == _lib.LBFT_ERR_STATE
    a.save_checkpoint(str(tmp_path / "ck.bin"))
    a.close()
    b = plain(amd, seeds, n, ps)
    b.load_checkpoint(str(tmp_path / "ck.bin"))
    done = None
    for _ in range(10000):
        left, done = b.run_steps(max_clock, 150)
        if left == 0:
            break
    assert done is not None and same(want, arrays(done))
    b.close()
    # a node-level session: legal after manual_finalize, as lbft_batch_commit_counts is; nothing was committed
    c = plain(amd, seeds[:2], n, ps)
    c.manual(max_clock)
    with pytest.raises(amd.LbftError) as e:
        amd.BatchResult(c).chain_stats()
    assert e.value.code == _lib.LBFT_ERR_STATE
    hist, authors, stats = c.manual_finalize().chain_stats()
    assert not hist.any() and not authors.any() and stats[0, 0::4].tolist() == [0, 2, 2 * n, 0, 2, 2] and not stats[0, 1::4].any()
    c.close()


# ---- refusals ----
def test_refusals(amd):
    from librabft_simulator_amd import _lib
    sim = plain(amd, np.arange(1, 5, dtype=np.uint64), 4, amd.ParamSet())
    res = sim.loop_until(200)
    L = _lib.lib()
    hist, authors, stats = np.full(8, 7, dtype=np.uint64), np.full(4, 7, dtype=np.uint64), np.full(24, 7, dtype=np.uint64)
    p = [a.ctypes.data for a in (hist, authors, stats)]
    assert L.lbft_batch_chain_stats(sim._h, 1, 0, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_chain_stats(sim._h, 0, 8, *p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_chain_stats(sim._h, 1, 2 ** 31 + 1, *p) == _lib.LBFT_ERR_INVALID  # groups x bins > 2^31
    for k in range(3):
        q = list(p)
        q[k] = None
        assert L.lbft_batch_chain_stats(sim._h, 1, 8, *q) == _lib.LBFT_ERR_INVALID
    assert (hist == 7).all() and (authors == 7).all() and (stats == 7).all()
    assert L.lbft_batch_chain_stats(sim._h, 1, 8, *p) == _lib.LBFT_OK and hist.sum() == stats[0] and authors.sum() == stats[5]
    with pytest.raises(ValueError):
        res.chain_stats(bins=0)
    sim.close()


# ---- the grid tool ----
def test_grid_cli_chain(amd):
    args = ["--nodes", "4", "--delta", "10,20", "--seeds-per-point", "8", "--max-clock", "300", "--assign", "interleaved"]
    out = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid", "--chain"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.strip()]
    assert [l["delta"] for l in lines] == [10, 20]
    from librabft_simulator_amd import grid
    sets = [amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, d, 2.0, 0.5)) for d in (10, 20)]
    set_of, seed_index = grid.set_assignment(2, 8, "interleaved")
    sim = amd.BatchSimulator.with_param_sets((1 + seed_index).astype(np.uint64), 4, sets, set_of)
    res = sim.loop_until(300, allow_faults=True)
    _, authors, stats = res.chain_stats()
    names = ("interval", "length", "lag", "tenure", "differing", "inversions")
    for k, l in enumerate(lines):
        assert set(l["chain"]) == {"set", "authors", "author_share", "agreement", *names} and l["faulted"] == 0
        assert [next(v for key, v in l["chain"][name].items() if key in ("samples", "instances", "nodes", "runs")) for name in names] == stats[k, 0::4].tolist()
        assert l["chain"]["authors"] == authors[k].tolist() and l["chain"]["agreement"] is True and l["chain"]["length"]["instances"] == 8
    assert [l["chain"] for l in lines] == json.loads(json.dumps(res.chain_by_param_set()))
    bare = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bare.returncode == 0, bare.stderr[-2000:]
    assert [{k: v for k, v in l.items() if k != "chain"} for l in lines] == [json.loads(l) for l in bare.stdout.splitlines() if l.strip()]
    sim.close()
