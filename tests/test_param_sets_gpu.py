"""Parameter-set batches on the device (lbft_batch_create_param_sets, liblbft_paramsets.so): every instance equals the oracle for its own
set's configuration and seed, and equals a plain batch of that set -- under both assignments of sets to instances, on both kernel classes,
through run_steps / checkpoints and save_node."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from support import amd, oracle_cfg, plain  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_THREADS = min(os.cpu_count() or 8, 32)
MAX_CLOCK = 1000


def small_grid(amd):
    """16 sets of the small class: delay mean x delta x lambda x target_commit_interval."""
    sets = []
    for mean in (5.0, 10.0):
        for delta in (10, 40):
            for lam in (0.25, 0.75):
                for tci in (100000, 40):
                    sets.append(amd.ParamSet(amd.RandomDelay.new(mean, mean / 2), amd.NodeConfig(tci, delta, 1.5 + lam, lam)))
    return sets


def assignment(n_sets, per_set, how):
    k = np.arange(n_sets * per_set)
    return (k // per_set if how == "blocked" else k % n_sets).astype(np.uint32)


@pytest.mark.parametrize("how", ["blocked", "interleaved"])
def test_sixteen_sets_equal_the_oracle_and_plain_batches(amd, oracle, how):
    sets = small_grid(amd)
    set_of = assignment(len(sets), 256, how)
    seeds = (np.arange(len(set_of)) * 7919 + 3).astype(np.uint64)
    sim = amd.BatchSimulator.with_param_sets(seeds, 4, sets, set_of)
    res = sim.loop_until(MAX_CLOCK)
    assert sim.layout()["kernel_class"] & 65536 and sim.layout()["kernel_class"] & 255 == 0, sim.layout()
    assert (res.faults == 0).all()
    cc, states, hist, starts = res.commit_counts, res.last_committed_states, res.committed_histories(64), res.startup_times
    for k, ps in enumerate(sets):
        idx = np.nonzero(set_of == k)[0]
        ref = oracle.run_batch(oracle_cfg(oracle, 4, ps), seeds[idx], MAX_CLOCK, threads=HOST_THREADS, history_cap=64)
        assert (cc[idx] == ref["commit_counts"]).all(), k
        assert (states[idx] == ref["last_states"]).all(), k
        assert (hist[idx] == ref["histories"]).all(), k
        assert (res.active_rounds[idx] == ref["active_rounds"]).all(), k
        for i in idx[:: max(1, len(idx) // 4)]:  # startup times and record hashes of a sample, against the oracle's single runs
            o = oracle.OracleSim(oracle_cfg(oracle, 4, ps), int(seeds[i])).run_until(MAX_CLOCK)
            assert list(starts[i]) == o.startup_times(), (k, i)
            for node in range(4):
                mine = res.committed_record_hashes(int(i), node)
                theirs = o.committed_record_hashes(node)
                assert [(int(r["block_hash"]), int(r["state"]), int(r["qc_hash"])) for r in mine] == \
                       [(int(r["block_hash"]), int(r["state"]), int(r["qc_hash"])) for r in theirs], (k, i, node)
        # device against device: a plain batch of this set on these seeds
        p = plain(amd, seeds[idx], 4, ps)
        pr = p.loop_until(MAX_CLOCK)
        assert (pr.commit_counts == cc[idx]).all() and (pr.last_committed_states == states[idx]).all(), k
        assert (pr.committed_histories(64) == hist[idx]).all() and (pr.startup_times == starts[idx]).all(), k
        p.close()
    sim.close()


def test_mid_class_with_loss_partition_and_round_trace_equals_the_oracle(amd, oracle):
    n = 20
    sets = [amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, 20, 2.0, 0.5)),
            amd.ParamSet(amd.RandomDelay.new(8.0, 9.0), amd.NodeConfig(100000, 30, 1.5, 0.75), drop_per_million=50000),
            amd.ParamSet(amd.RandomDelay.new(12.0, 2.0), amd.NodeConfig(60, 15, 2.0, 0.25), partition=(7, 100, 400)),
            amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, 25, 2.0, 0.5), drop_per_million=20000, partition=(10, 300, 600))]
    per = 24
    set_of = assignment(len(sets), per, "interleaved")
    seeds = (np.arange(len(set_of)) + 11).astype(np.uint64)
    sim = amd.BatchSimulator.with_param_sets(seeds, n, sets, set_of)
    res = sim.loop_until(MAX_CLOCK, round_trace=512)
    assert sim.layout()["kernel_class"] & 255 == 1 and sim.layout()["kernel_class"] & 65536, sim.layout()
    assert (res.faults == 0).all()
    for k, ps in enumerate(sets):
        idx = np.nonzero(set_of == k)[0]
        ref = oracle.run_batch(oracle_cfg(oracle, n, ps), seeds[idx], MAX_CLOCK, threads=HOST_THREADS, history_cap=64)
        assert (res.commit_counts[idx] == ref["commit_counts"]).all(), k
        assert (res.last_committed_states[idx] == ref["last_states"]).all(), k
        assert (res.committed_histories(64)[idx] == ref["histories"]).all(), k
        for i in idx[:3]:
            o = oracle.OracleSim(oracle_cfg(oracle, n, ps), int(seeds[i])).enable_data_writer().run_until(MAX_CLOCK)
            assert res.round_switches(int(i)) == o.round_switches(), (k, i)
    sim.close()


def test_one_set_equal_to_the_base_config_equals_the_plain_batch(amd):
    seeds = np.arange(1, 257, dtype=np.uint64)
    ps = amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig())
    a = amd.BatchSimulator.with_param_sets(seeds, 4, [ps], np.zeros(256, dtype=np.uint32))
    b = amd.BatchSimulator.new(seeds, 4, amd.RandomDelay.new(10.0, 4.0))
    ra, rb = a.loop_until(MAX_CLOCK), b.loop_until(MAX_CLOCK)
    for name in ("commit_counts", "active_rounds", "last_committed_states", "startup_times", "epochs", "faults"):
        assert (getattr(ra, name) == getattr(rb, name)).all(), name
    assert (ra.committed_histories(64) == rb.committed_histories(64)).all()
    ca, cb = ra.counters, rb.counters
    for name in ("events", "rng_draws", "rounds", "commits", "events_scheduled", "faulted_instances", "max_queue", "max_snapshots", "max_blocks"):
        assert ca[name] == cb[name], name
    for node in range(4):
        assert ra.save_node(5, node) == rb.save_node(5, node)
    a.close()
    b.close()


def test_steps_and_checkpoint_equal_a_straight_run(amd, tmp_path):
    sets = small_grid(amd)[:4] + [amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, 20, 2.0, 0.5), drop_per_million=30000)]
    set_of = assignment(len(sets), 32, "interleaved")
    seeds = np.arange(1, len(set_of) + 1, dtype=np.uint64)
    straight = amd.BatchSimulator.with_param_sets(seeds, 4, sets, set_of).loop_until(MAX_CLOCK)
    a = amd.BatchSimulator.with_param_sets(seeds, 4, sets, set_of)
    left, _ = a.run_steps(MAX_CLOCK, 40)
    assert left > 0
    a.save_checkpoint(str(tmp_path / "ck.bin"))
    b = amd.BatchSimulator.with_param_sets(seeds, 4, sets, set_of)
    b.load_checkpoint(str(tmp_path / "ck.bin"))
    res = None
    for _ in range(10000):
        left, res = b.run_steps(MAX_CLOCK, 40)
        if left == 0:
            break
    assert res is not None
    assert (res.commit_counts == straight.commit_counts).all()
    assert (res.last_committed_states == straight.last_committed_states).all()
    assert (res.committed_histories(64) == straight.committed_histories(64)).all()
    # a checkpoint of another grid is refused
    other = amd.BatchSimulator.with_param_sets(seeds, 4, sets[::-1], set_of)
    with pytest.raises(amd.LbftError):
        other.load_checkpoint(str(tmp_path / "ck.bin"))
    for s in (a, b, other):
        s.close()


def test_save_node_uses_the_instance_own_node_config(amd):
    sets = [amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, 20, 2.0, 0.5)),
            amd.ParamSet(amd.RandomDelay.new(6.0, 3.0), amd.NodeConfig(500, 35, 1.25, 0.75))]
    seeds = np.arange(1, 65, dtype=np.uint64)
    set_of = assignment(2, 32, "interleaved")
    sim = amd.BatchSimulator.with_param_sets(seeds, 4, sets, set_of)
    res = sim.loop_until(MAX_CLOCK)
    for inst in (0, 1, 6, 7):
        ps = sets[set_of[inst]]
        p = plain(amd, seeds[inst:inst + 1], 4, ps)
        pr = p.loop_until(MAX_CLOCK)
        for node in range(4):
            assert res.save_node(inst, node) == pr.save_node(0, node), (inst, node)
        p.close()
    sim.close()


def test_node_level_interface_is_refused(amd):
    sim = amd.BatchSimulator.with_param_sets(np.arange(1, 5, dtype=np.uint64), 4, small_grid(amd)[:2], np.array([0, 1, 0, 1], dtype=np.uint32))
    with pytest.raises(amd.LbftError) as e:
        sim.manual(1000)
    assert e.value.code == -3
    sim.close()


def test_grid_cli_prints_one_line_per_point(amd):
    out = subprocess.run([sys.executable, "-m", "librabft_simulator_amd.grid", "--nodes", "4", "--mean", "5,10", "--delta", "10,40",
                          "--lambda", "0.25,0.5,1.0", "--seeds-per-point", "16", "--max-clock", "500", "--assign", "interleaved"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 12
    assert {(l["mean"], l["delta"], l["lambda"]) for l in lines} == {(m, d, x) for m in (5.0, 10.0) for d in (10, 40) for x in (0.25, 0.5, 1.0)}
    assert all(l["instances"] == 16 and l["faulted"] == 0 and l["commits"]["max"] >= l["commits"]["min"] for l in lines)
