"""Record hashes of whole batches on the device (BatchResult.chain_record_hashes / chain_heads, lbft_k_rh_chain).  In every case
entries[i, :count] equals committed_record_hashes(i, node) -- the single-lane kernel -- for EVERY node of every instance, heads is the
last entry and node_prefix equals commit_counts; for the listed seeds the entries also equal the oracle's own records.  The shapes are the
smallest at which the mapping can go wrong: segments of 4, 8 and 64 lanes, more segments than two wavefronts hold, an idle lane per
segment, block seams every four entries and the 64-entry seam, one to four voter words, two voter rounds, 64-wide tiles, parameter sets,
empty chains, a capacity below the chains, heads alone, checkpoints, reset, the refusals, and 4 096 instances."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from support import amd  # noqa: F401

pytestmark = pytest.mark.gpu
FIELDS = ("block_hash", "state", "qc_hash", "num_votes")


def make(amd, kw, seeds, **sim_kw):
    kw = dict(kw)
    n = kw.pop("num_nodes")
    delay = amd.RandomDelay.new(kw.get("mean", 10.0), kw.get("variance", 4.0))
    nc = amd.NodeConfig(kw.get("target_commit_interval", 100000), kw.get("delta", 20), kw.get("gamma", 2.0), kw.get("lambda_", 0.5))
    return amd.BatchSimulator.new(np.asarray(seeds, dtype=np.uint64), n, delay, nc, commands_per_epoch=kw.get("commands_per_epoch", 30000),
                                  voting_rights=kw.get("voting_rights"), equivocate_every=kw.get("equivocate_every", 0),
                                  drop_per_million=kw.get("drop_per_million", 0), quirks=kw.get("quirks", 0),
                                  rights_rotation=kw.get("rights_rotation", 0), **sim_kw)


def check_nodes(res, instances=None, cap=None):
    """chain_record_hashes() against the per-node call for every node of `instances` (default: all); returns its three arrays."""
    from librabft_simulator_amd import _lib
    entries, heads, prefix = res.chain_record_hashes(cap)
    counts = res.commit_counts
    m, n = counts.shape
    assert entries.dtype == _lib.RECORD_HASH_DTYPE and heads.dtype == _lib.CHAIN_HEAD_DTYPE and prefix.dtype == np.uint32
    assert entries.shape == (m, max(int(counts.max()), 1) if cap is None else cap) and heads.shape == (m,) and prefix.shape == (m, n)
    assert not res.faults.any()
    assert (prefix == counts).all()  # every history is a prefix of its chain
    assert (heads["length"] == counts.max(axis=1)).all() and (heads["ref_node"] == counts.argmax(axis=1)).all()
    width = entries.shape[1]
    for i in (range(m) if instances is None else instances):
        length = int(heads["length"][i])
        assert not entries[i, length:].tobytes().strip(b"\0")
        if length == 0:
            assert not heads[i].tobytes().strip(b"\0")
        elif length <= width:
            last = entries[i, length - 1]
            assert all(heads[f][i] == last[f] for f in FIELDS + ("flags",)), (i, heads[i], last)
        for node in range(n):
            mine = res.committed_record_hashes(i, node)
            assert len(mine) == counts[i, node]
            k = min(len(mine), width)
            assert entries[i, :k].tobytes() == mine[:k].tobytes(), (i, node)
            if node == heads["ref_node"][i] and length:
                assert all(heads[f][i] == mine[-1][f] for f in FIELDS + ("flags",))
                assert int(heads["state"][i]) == int(res.last_committed_states[i, node])
    return entries, heads, prefix


def oracle_runs(oracle, cfg, seeds, max_clock):
    """One finished OracleSim per seed (the oracle's calls leave the interpreter lock: the runs go side by side)."""
    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(lambda seed: oracle.OracleSim(cfg, int(seed)).run_until(max_clock), seeds))


def check_oracle(oracle, kw, seeds, max_clock, entries, heads, min_length=1):
    cfg = oracle.make_config(math_mode=1, **kw)
    for i, sim in enumerate(oracle_runs(oracle, cfg, seeds, max_clock)):
        counts = sim.commit_counts()
        assert max(counts) >= min_length  # (asserted on the oracle: the case reaches what it is there for)
        for node in range(kw["num_nodes"]):
            ref = sim.committed_record_hashes(node)
            assert len(ref) == counts[node] <= heads["length"][i]
            for f in FIELDS:
                assert (entries[f][i, :len(ref)] == ref[f]).all(), (i, node, f)
            assert ref["has_qc"].all() and not entries["flags"][i, :len(ref)].any()
        sim.close()


# name: (configuration, clock, instances, kernel class or None, shortest chain the oracle must reach, creation keywords)
CASES = {
    # W = 4: two full wavefronts' worth of segments and five more, a block seam every four entries; class 0, instance-major rows
    "n4_37_instances": (dict(num_nodes=4), 1000, 37, 0, 20),
    "n3_idle_lane": (dict(num_nodes=3), 1000, 5, 0, 20),  # W = 4 with an idle lane per segment
    # W = 8, the epoch-id hash at every epoch change
    "n7_weighted_epochs_q2": (dict(num_nodes=7, voting_rights=[2, 1, 1, 3, 1, 2, 1], commands_per_epoch=9, quirks=2), 2000, 9, None, 10),
    "n7_equivocators": (dict(num_nodes=7, equivocate_every=3), 1000, 9, None, 10),
    "n40_long_tail": (dict(num_nodes=40, mean=10.0, variance=400.0), 300, 3, 2, 1),  # W = 64, two voter words
    "n33_past_the_64_entry_seam": (dict(num_nodes=33), 2300, 2, 2, 65),  # W = 64: a second block of entries
    # two rounds of voter lanes, four voter words
    "n100_weighted": (dict(num_nodes=100, voting_rights=[1 + (i % 3) for i in range(100)]), 300, 2, 2, 1),
    "n8_lossy_tiles": (dict(num_nodes=8, drop_per_million=30000, quirks=3), 1000, 70, 1, 10),  # class 1: 64-wide tiles, a partial tile
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_chains_equal_every_node_and_the_oracle(amd, oracle, name):
    kw, max_clock, m, cls, min_length = CASES[name]
    seeds = np.arange(1, m + 1, dtype=np.uint64)
    seeds[:3] = [52, 7, 1234567][:min(3, m)]
    sim = make(amd, kw, seeds)
    res = sim.loop_until(max_clock)
    if cls is not None:
        assert sim.layout()["kernel_class"] & 0xff == cls
    entries, heads, _ = check_nodes(res)
    listed = min(m, 3)
    check_oracle(oracle, kw, seeds[:listed], max_clock, entries, heads, min_length)
    assert (res.chain_heads() == heads).all()
    if kw["num_nodes"] > 64:  # voters of the second round of lanes were hashed
        assert entries["num_votes"].max() > 64
    sim.close()


def test_parameter_set_batch(amd, oracle):
    n, max_clock = 4, 800
    sets = [amd.ParamSet(), amd.ParamSet(amd.RandomDelay.new(20.0, 9.0))]
    set_of = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1], dtype=np.uint32)
    seeds = np.arange(1, len(set_of) + 1, dtype=np.uint64)
    sim = amd.BatchSimulator.with_param_sets(seeds, n, sets, set_of)
    res = sim.loop_until(max_clock)
    entries, heads, _ = check_nodes(res)
    for k, (mean, variance) in enumerate(((10.0, 4.0), (20.0, 9.0))):
        idx = np.nonzero(set_of == k)[0]
        check_oracle(oracle, dict(num_nodes=n, mean=mean, variance=variance), seeds[idx], max_clock, entries[idx], heads[idx])
    assert heads["length"][set_of == 0].mean() > heads["length"][set_of == 1].mean()
    sim.close()


def test_empty_chains(amd, oracle):
    kw, max_clock, seeds = dict(num_nodes=4), 5, np.arange(1, 38, dtype=np.uint64)
    ref = oracle.run_batch(oracle.make_config(math_mode=1, **kw), seeds, max_clock)
    assert not ref["commit_counts"].any()  # (on the oracle first: no chain has an entry)
    sim = make(amd, kw, seeds)
    res = sim.loop_until(max_clock)
    entries, heads, prefix = check_nodes(res)
    assert entries.shape == (37, 1) and not entries.tobytes().strip(b"\0") and not heads.tobytes().strip(b"\0") and not prefix.any()
    assert not res.chain_heads().tobytes().strip(b"\0")
    sim.close()


def test_truncation_and_heads_alone(amd):
    from librabft_simulator_amd import _lib
    kw, seeds = dict(num_nodes=4), np.arange(1, 20, dtype=np.uint64)
    sim = make(amd, kw, seeds)
    res = sim.loop_until(1000)
    full, heads, prefix = check_nodes(res)
    assert heads["length"].min() > 7
    for cap in (1, 7, full.shape[1] + 9, 3 * full.shape[1]):  # below the chains, a seam's neighbour, above the chains
        cut, heads_cut, prefix_cut = res.chain_record_hashes(cap)
        k = min(cap, full.shape[1])
        assert cut.shape == (len(seeds), cap) and cut[:, :k].tobytes() == np.ascontiguousarray(full[:, :k]).tobytes()
        assert not cut[:, k:].tobytes().strip(b"\0")
        assert (heads_cut == heads).all() and (prefix_cut == prefix).all()  # the heads are unaffected
    assert (res.chain_heads() == heads).all()
    # a capacity above the log capacity: the rows past it are zeroed by the call
    L = _lib.lib()
    lcap = 4096
    big = np.full((len(seeds), lcap), 7, dtype=_lib.RECORD_HASH_DTYPE)
    h = np.zeros(len(seeds), dtype=_lib.CHAIN_HEAD_DTYPE)
    assert L.lbft_batch_chain_record_hashes(sim._h, big.ctypes.data, lcap, h.ctypes.data, None) == _lib.LBFT_OK
    assert (h == heads).all() and big[:, :full.shape[1]].tobytes() == full.tobytes() and not big[:, full.shape[1]:].tobytes().strip(b"\0")
    sim.close()


def test_checkpoint_reset_and_rerun(amd, tmp_path):
    from librabft_simulator_amd import _lib
    kw, max_clock, seeds = dict(num_nodes=4), 500, np.arange(1, 17, dtype=np.uint64)
    sim = make(amd, kw, seeds)
    with pytest.raises(amd.LbftError) as e:  # before the run
        amd.BatchResult(sim).chain_heads()
    assert e.value.code == _lib.LBFT_ERR_STATE
    res = sim.loop_until(max_clock)
    want = [a.copy() for a in check_nodes(res)]
    counts = res.commit_counts.copy()
    again = res.chain_record_hashes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(want, again)) and (res.commit_counts == counts).all()  # the call changes no state
    sim.reset()
    with pytest.raises(amd.LbftError) as e:  # between reset() and the next run
        amd.BatchResult(sim).chain_record_hashes(4)
    assert e.value.code == _lib.LBFT_ERR_STATE
    rerun = sim.loop_until(max_clock).chain_record_hashes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(want, rerun))
    sim.close()
    a = make(amd, kw, seeds)
    left, _ = a.run_steps(max_clock, 150)
    assert left > 0
    with pytest.raises(amd.LbftError) as e:  # (an unfinished run is no finished run)
        amd.BatchResult(a).chain_heads()
    assert e.value.code == _lib.LBFT_ERR_STATE
    a.save_checkpoint(str(tmp_path / "ck.bin"))
    a.close()
    b = make(amd, kw, seeds)
    b.load_checkpoint(str(tmp_path / "ck.bin"))
    done = None
    for _ in range(10000):
        left, done = b.run_steps(max_clock, 150)
        if left == 0:
            break
    assert done is not None
    loaded = done.chain_record_hashes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(want, loaded))
    b.close()


def test_refusals(amd):
    from librabft_simulator_amd import _lib
    L = _lib.lib()
    sim = make(amd, dict(num_nodes=4), np.arange(1, 5, dtype=np.uint64))
    out = np.full((4, 8), 7, dtype=_lib.RECORD_HASH_DTYPE)
    heads = np.full(4, 7, dtype=_lib.CHAIN_HEAD_DTYPE)
    prefix = np.full((4, 4), 7, dtype=np.uint32)
    o, h, p = out.ctypes.data, heads.ctypes.data, prefix.ctypes.data
    assert L.lbft_batch_chain_record_hashes(sim._h, o, 8, h, p) == _lib.LBFT_ERR_STATE  # before the run
    res = sim.loop_until(200)
    assert L.lbft_batch_chain_record_hashes(sim._h, o, 8, None, p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_chain_record_hashes(sim._h, o, 0, h, p) == _lib.LBFT_ERR_INVALID
    assert L.lbft_batch_chain_record_hashes(None, o, 8, h, p) == _lib.LBFT_ERR_INVALID
    untouched = np.full(1, 7, dtype=_lib.RECORD_HASH_DTYPE).tobytes()
    assert out.tobytes() == untouched * 32 and (prefix == 7).all() and heads.tobytes() == np.full(4, 7, dtype=_lib.CHAIN_HEAD_DTYPE).tobytes()
    assert L.lbft_batch_chain_record_hashes(sim._h, o, 8, h, p) == _lib.LBFT_OK
    assert (prefix == res.commit_counts).all() and (heads["length"] == res.commit_counts.max(axis=1)).all()
    with pytest.raises(ValueError):
        res.chain_record_hashes(0)
    sim.close()


def test_4096_instances(amd, oracle):
    kw, max_clock, m = dict(num_nodes=4), 1000, 4096
    seeds = np.arange(1, m + 1, dtype=np.uint64)
    sim = make(amd, kw, seeds)
    res = sim.loop_until(max_clock)
    assert sim.layout()["kernel_class"] & 0xff == 0 and not res.faults.any()
    entries, heads, prefix = check_nodes(res, instances=range(5, m, 128))  # 32 strided instances against the per-node call
    counts = res.commit_counts
    assert (heads["length"] > 0).all()
    assert (heads["state"] == res.last_committed_states[np.arange(m), heads["ref_node"]]).all()
    assert (entries["qc_hash"][np.arange(m), heads["length"] - 1] == heads["qc_hash"]).all()
    assert (res.chain_heads() == heads).all()
    cfg = oracle.make_config(math_mode=1, **kw)
    for i, o in enumerate(oracle_runs(oracle, cfg, seeds[:1024], max_clock)):  # the oracle's last records for the first 1 024 seeds
        ref = o.committed_record_hashes(int(heads["ref_node"][i]))
        assert len(ref) == heads["length"][i] == max(o.commit_counts())
        assert all(heads[f][i] == ref[f][-1] for f in FIELDS), i
        o.close()
    sim.close()
