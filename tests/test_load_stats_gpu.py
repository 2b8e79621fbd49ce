"""The run load on the device (lbft_batch_load_stats, lbft_batch_instance_load; lbft_k_ps_load): every instance's sixteen words against
the oracle (one simulator per seed), against the batch's own read-backs and counters and against the host model's high-water marks;
the grouped statistics, histogram and fault census against numpy over the rows (tests/load_stats_reference.py); the shapes at which a
wavefront's four segments run partly empty or make a second trip; networks of 3 to 66 nodes; a batch whose calendar runs out of
chunks; and every kind of batch a finished run can come from."""
import numpy as np
import pytest

import load_stats_reference as ref
import queue_exhaustion as qx
from strided_shapes import gs_workgroups, trips
from support import amd, oracle_cfg, plain, run_to_end  # noqa: F401

pytestmark = pytest.mark.gpu
F = ref.F
PER_STEP = 16  # instances a workgroup of lbft_k_ps_load takes at a time (LD_BLOCK / LD_SEGMENT)


def four_sets(amd):
    return [amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(100000, 20, 2.0, 0.5)),
            amd.ParamSet(amd.RandomDelay.new(5.0, 2.5), amd.NodeConfig(40, 40, 1.75, 0.25)),
            amd.ParamSet(amd.RandomDelay.new(20.0, 9.0), amd.NodeConfig(100000, 10, 2.0, 1.0), drop_per_million=20000),
            amd.ParamSet(amd.RandomDelay.new(3.0, 1.0), amd.NodeConfig(100000, 20, 2.0, 0.75), partition=(1, 100, 250))]


def oracle_of_sets(oracle, n, sets, set_of, seeds, max_clock, **kw):
    want = np.full((len(seeds), 16), -1, dtype=np.int64)
    for g, ps in enumerate(sets):
        idx = np.flatnonzero(np.asarray(set_of) == g)
        if len(idx):
            want[idx] = ref.oracle_rows(oracle, oracle_cfg(oracle, n, ps, **kw), np.asarray(seeds)[idx], max_clock)[0]
    return want


def check_rows(res, want=None, idx=slice(None)):
    """instance_load(): the oracle's counters where it has them (`want`, for the instances `idx`), the batch's own read-backs in
    families 13 to 15, the message sum, and the batch counters word for word.  -> the rows."""
    rows = res.instance_load()
    assert rows.dtype == np.uint32 and rows.shape == (res._sim.num_instances, 16)
    if want is not None:
        for f in ref.ORACLE_FAMILIES:
            assert (rows[idx, f] == want[:, f]).all(), (ref.FAMILIES[f], rows[idx, f], want[:, f])
    assert (rows[:, F["log"]] == res.commit_counts.max(axis=1)).all() and (rows[:, F["commits"]] == res.commit_counts.min(axis=1)).all()
    assert (rows[:, F["rounds"]] == res.active_rounds.min(axis=1)).all()
    assert (rows[:, F["messages"]] == rows[:, 0] + rows[:, 1] + rows[:, 2]).all()
    c, total, top = res.counters, rows.sum(axis=0, dtype=np.uint64), rows.max(axis=0)
    print("counters", c)
    assert c["events"] == [int(v) for v in total[:4]]
    for key, name in (("events_scheduled", "scheduled"), ("rng_draws", "draws"), ("timers_folded", "folded"), ("node_updates", "updates"),
                      ("commits", "commits"), ("rounds", "rounds")):
        assert c[key] == int(total[F[name]]), key
    for key, name in (("max_queue", "queue"), ("max_snapshots", "snapshots"), ("max_blocks", "blocks")):
        assert c[key] == int(top[F[name]]), key
    assert c["faulted_instances"] == int(np.count_nonzero(res.faults))
    return rows


def check_grouped(res, rows, set_of=None, groups=1, families=range(16), binnings=((None, None),)):
    """load_stats() for the given families and binnings (None = the default) equals numpy over the rows.  -> caps."""
    faults = res.faults
    want_census, want_stats = ref.census(faults, set_of, groups), ref.stats(rows, faults, set_of, groups)
    for f in families:
        for width, bins in binnings:
            hist, census, stats, caps = res.load_stats(ref.FAMILIES[f] if f % 2 else f, width, bins)
            w = 1 if width is None else width
            b = ref.default_bins(rows, faults, f, w) if bins is None else bins
            assert hist.shape == (groups, b) and census.shape == (groups, 32) and stats.shape == (groups, 64) and caps.shape == (5,), (f, width, bins)
            assert hist.dtype == census.dtype == stats.dtype == np.uint64 and caps.dtype == np.uint32
            assert (stats == want_stats).all(), (f, stats, want_stats)
            assert (census == want_census).all(), (f, census, want_census)
            assert (hist == ref.hist(rows, faults, f, w, b, set_of, groups)).all(), (f, width, bins)
            assert (hist.sum(axis=1) == stats[:, 0]).all()
    return caps


# ---- 1, 2: the parameter-set batch of 4 sets x 24 seeds x 4 nodes, and the lossy 7-node batch of 70 ----
M1, N1, T1 = 96, 4, 400


@pytest.fixture(scope="module")
def batch1(amd, oracle):
    sets = four_sets(amd)
    set_of = np.random.default_rng(4).permutation(np.repeat(np.arange(4), M1 // 4)).astype(np.uint32)
    seeds = np.arange(1, M1 + 1, dtype=np.uint64) * 7919 + 3
    sim = amd.BatchSimulator.with_param_sets(seeds, N1, sets, set_of)
    res = sim.loop_until(T1)
    yield sim, res, sets, set_of, seeds
    sim.close()


def test_rows_and_statistics_of_a_parameter_set_batch_equal_the_oracle(batch1, oracle):
    sim, res, sets, set_of, seeds = batch1
    assert not res.faults.any()
    rows = check_rows(res, oracle_of_sets(oracle, N1, sets, set_of, seeds, T1))
    caps = check_grouped(res, rows, set_of, 4)
    check_grouped(res, rows, set_of, 4, families=(F["queue"], F["messages"]), binnings=((1, 3), (7, None), (5, 9000), (1, 20000)))  # (three LDS passes)
    assert caps[1] == 0 and (rows[:, F["chunks"]] == 0).all()  # (four nodes run no calendar)
    assert (rows[:, F["queue"]] <= caps[0]).all() and (rows[:, F["snapshots"]] <= caps[2]).all() and (rows[:, F["blocks"]] <= caps[3]).all()
    by_set = res.load_by_param_set()
    for g, row in enumerate(by_set):
        sel = rows[set_of == g].astype(np.float64)
        assert row["instances"] == row["clean"] == 24 and row["faults"] == {}
        assert row["messages"] == {"mean": sel[:, F["messages"]].mean(), "min": int(sel[:, F["messages"]].min()), "max": int(sel[:, F["messages"]].max())}
        assert row["messages_per_commit"] == sel[:, F["messages"]].sum() / sel[:, F["commits"]].sum()
        assert row["headroom"]["queue"] == sel[:, F["queue"]].max() / int(caps[0]) and row["headroom"]["chunks"] is None
        assert row["queue_quantiles"]["0.5"] == int(np.quantile(sel[:, F["queue"]], 0.5, method="inverted_cdf"))
        assert row["worst_seed"]["queue"] == int(seeds[set_of == g][np.argmax(sel[:, F["queue"]])])
    assert res.by_param_set()[0]["commits"]["max"] == by_set[0]["commits"]["max"]


def test_refusals_come_in_the_stated_order(amd):
    from librabft_simulator_amd import _lib
    L = _lib.lib()
    sim = amd.BatchSimulator.new(np.arange(1, 4, dtype=np.uint64), 4, amd.RandomDelay.new(10.0, 4.0))
    hist, faults, stats, rows = np.zeros(8, np.uint64), np.zeros(32, np.uint64), np.zeros(64, np.uint64), np.zeros(48, np.uint32)
    p = [a.ctypes.data for a in (hist, faults, stats)]
    for family, width, bins in ((9, 1, 8), (16, 1, 8), (9, 0, 8), (9, 1, 0)):  # before a run: the state comes before the arguments
        assert L.lbft_batch_load_stats(sim._h, family, width, bins, *p, None) == _lib.LBFT_ERR_STATE
    assert L.lbft_batch_load_stats(sim._h, 16, 0, 0, None, *p[1:], None) == _lib.LBFT_ERR_INVALID  # ... and a NULL before the state
    assert L.lbft_batch_instance_load(sim._h, rows.ctypes.data) == _lib.LBFT_ERR_STATE
    assert L.lbft_batch_instance_load(sim._h, None) == _lib.LBFT_ERR_INVALID
    sim.loop_until(100)
    for family, width, bins in ((16, 1, 8), (9, 0, 8), (9, 1, 0), (9, 1, (1 << 31) + 1)):
        assert L.lbft_batch_load_stats(sim._h, family, width, bins, *p, None) == _lib.LBFT_ERR_INVALID
    assert not hist.any() and not faults.any() and not stats.any() and not rows.any()
    assert L.lbft_batch_load_stats(sim._h, 15, 1, 8, *p, None) == 0 and stats[0] == 3 and L.lbft_batch_instance_load(sim._h, rows.ctypes.data) == 0
    sim.close()


def host_model_marks(oracle, cfg, seeds, max_clock, caps):
    hm = oracle.hostmodel_run_batch(cfg, seeds, max_clock, threads=8, **caps)
    assert not hm["faults"].any()
    return hm["maxq"], hm["maxsnap"]


def test_high_water_marks_equal_the_host_models(batch1, amd, oracle):
    sim, res, sets, set_of, seeds = batch1
    rows = res.instance_load()
    caps = qx.planned_caps(oracle, dict(num_nodes=N1), M1, T1, param_sets=4)
    for g, ps in enumerate(sets):
        idx = np.flatnonzero(set_of == g)
        maxq, maxsnap = host_model_marks(oracle, oracle_cfg(oracle, N1, ps), seeds[idx], T1, caps)
        assert (rows[idx, F["queue"]] == maxq).all() and (rows[idx, F["snapshots"]] == maxsnap).all(), g
    # 70 instances of 7 nodes with 2 % loss: kernel class 1, rows in 64-instance tiles, the second tile partly filled
    ps = amd.ParamSet(amd.RandomDelay.new(10.0, 4.0), amd.NodeConfig(), drop_per_million=20000)
    seeds7 = np.arange(1, 71, dtype=np.uint64) * 104729 + 17
    sim7 = plain(amd, seeds7, 7, ps)
    res7 = sim7.loop_until(T1)
    assert sim7.layout()["kernel_class"] & 255 == 1 and not res7.faults.any()
    cfg7 = oracle_cfg(oracle, 7, ps)
    rows7 = check_rows(res7, ref.oracle_rows(oracle, cfg7, seeds7, T1)[0])
    check_grouped(res7, rows7, families=(F["queue"], F["snapshots"], F["rounds"]))
    plan = oracle.plan(cfg7, 70, T1)
    assert plan["tw"] == 64
    maxq, maxsnap = host_model_marks(oracle, cfg7, seeds7, T1, {k: plan[k] for k in ("qcap", "scap", "bcap", "lcap", "ql", "qheap", "qcal", "ring", "ring_topup", "tw")})
    assert (rows7[:, F["queue"]] == maxq).all() and (rows7[:, F["snapshots"]] == maxsnap).all()
    sim7.close()


# ---- 3: segments and group shapes ----
GROUPS = 256
SIZES = {3: 0, 20: 1, 41: 3, 77: 4, 100: 5, 150: 16, 201: 17, 230: 70, 255: 0}  # group -> instances; every other group holds k % 3


def test_partly_filled_segments_second_trips_and_scattered_groups(amd, oracle):
    sizes = np.array([SIZES.get(g, g % 3) for g in range(GROUPS)])
    set_of = np.random.default_rng(256).permutation(np.repeat(np.arange(GROUPS), sizes)).astype(np.uint32)
    m, max_clock = len(set_of), 200
    gx = gs_workgroups(1024, GROUPS, (70 + PER_STEP - 1) // PER_STEP, 70)
    assert gx == 4 and max(trips(70, gx, PER_STEP)) == 2 and min(trips(70, gx, PER_STEP)) == 1 and max(trips(17, gx, PER_STEP)) == 1
    kinds = four_sets(amd)
    sets = [kinds[g % 4] for g in range(GROUPS)]
    seeds = np.arange(1, m + 1, dtype=np.uint64)
    sim = amd.BatchSimulator.with_param_sets(seeds, 4, sets, set_of)
    res = sim.loop_until(max_clock)
    assert not res.faults.any()
    rows = check_rows(res, oracle_of_sets(oracle, 4, kinds, set_of % 4, seeds, max_clock))
    check_grouped(res, rows, set_of, GROUPS, families=(F["queue"], F["commits"], F["notifications"]))
    stats = res.load_stats()[2]
    assert [int(stats[g, 0]) for g in sorted(SIZES)] == [SIZES[g] for g in sorted(SIZES)] and not stats[255].any() and not stats[3].any()
    sim.close()


def test_a_batch_of_one_instance(amd, oracle):
    ps = four_sets(amd)[0]
    seeds = np.array([52], dtype=np.uint64)
    sim = plain(amd, seeds, 4, ps)
    res = sim.loop_until(300)
    rows = check_rows(res, ref.oracle_rows(oracle, oracle_cfg(oracle, 4, ps), seeds, 300)[0])
    check_grouped(res, rows)
    sim.close()


def test_a_plain_batch_past_the_grid_makes_a_second_trip(amd, oracle):
    m, max_clock = 16400, 100
    gx = gs_workgroups(1024, 1, (m + PER_STEP - 1) // PER_STEP, m)
    assert gx == 1024 and m > gx * PER_STEP and sum(t == 2 for t in trips(m, gx, PER_STEP)) == m - gx * PER_STEP
    ps = four_sets(amd)[0]
    seeds = np.arange(1, m + 1, dtype=np.uint64)
    sim = plain(amd, seeds, 4, ps)
    res = sim.loop_until(max_clock)
    idx = np.concatenate([np.arange(0, m - 16, (m - 16) // 240)[:240], np.arange(m - 16, m)])
    assert len(idx) == 256 and (idx[-16:] >= gx * PER_STEP).all()  # (the last sixteen are taken on the second trip)
    rows = check_rows(res, ref.oracle_rows(oracle, oracle_cfg(oracle, 4, ps), seeds[idx], max_clock)[0], idx)
    check_grouped(res, rows, families=(F["queue"], F["messages"]))
    sim.close()


# ---- 4: node counts ----
@pytest.mark.parametrize("n,max_clock", ((3, 1000), (33, 150), (66, 150)))  # (the oracle takes under a second for each)
def test_node_counts_against_the_oracle(amd, oracle, n, max_clock):
    ps = four_sets(amd)[0]
    seeds = np.array([11, 22, 33], dtype=np.uint64)
    sim = plain(amd, seeds, n, ps)
    res = sim.loop_until(max_clock)
    assert not res.faults.any()
    rows = check_rows(res, ref.oracle_rows(oracle, oracle_cfg(oracle, n, ps), seeds, max_clock)[0])
    caps = check_grouped(res, rows, families=(F["log"], F["commits"], F["rounds"], F["chunks"]))
    calendar = bool(sim.layout()["kernel_class"] & (1 << 9))
    assert (caps[1] != 0) == calendar and ((rows[:, F["chunks"]] != 0) == calendar).all()
    sim.close()


# ---- 5: faults and the chunk pool ----
def test_exhausted_chunk_pool_census_and_headroom(amd):
    kw, max_clock, queue_capacity, words = qx.MIXED["n20_push_event"]
    seeds = np.asarray(qx.MIXED_SEEDS, dtype=np.uint64)
    delay = amd.RandomDelay.uniform(kw["uniform_lo"], kw["uniform_hi"])
    sim = amd.BatchSimulator.new(seeds, kw["num_nodes"], delay, queue_capacity=queue_capacity)
    res = sim.loop_until(max_clock, allow_faults=True)
    assert sim.layout()["kernel_class"] & (1 << 9)
    faults = res.faults.copy()
    assert ((faults != 0) == (np.asarray(words) != 0)).all() and faults.any() and not faults.all()
    rows = check_rows(res)
    caps = check_grouped(res, rows, families=(F["queue"], F["chunks"]))
    hist, census, stats, _ = res.load_stats("chunks")
    for k in range(32):
        assert census[0, k] == np.count_nonzero(faults & np.uint32(1 << k))
    assert (census[0] == np.bincount(np.flatnonzero((faults[:, None] >> np.arange(32, dtype=np.uint32)) & 1) % 32, minlength=32)).all()
    clean = faults == 0
    assert stats[0, 0] == clean.sum() and stats[0, 4 * F["chunks"] + 3] == rows[clean, F["chunks"]].max()
    queue, chunks = rows[:, F["queue"]].astype(np.int64), rows[:, F["chunks"]].astype(np.int64)
    print("caps", caps.tolist(), "queue", queue.tolist(), "chunks", chunks.tolist(), "faults", faults.tolist())
    assert caps[1] > 0 and (-(-queue[clean] // 31) <= chunks[clean]).all() and (chunks <= caps[1]).all()
    starved = ((faults & qx.F_QUEUE) != 0) & (queue < caps[0])
    assert starved.any() and (chunks[starved] == caps[1]).all()  # the pool really was empty
    by_set = res.load_by_param_set()[0]
    assert by_set["faults"] == {"queue_overflow": int(np.count_nonzero(faults & 1))} and by_set["clean"] == clean.sum() and by_set["instances"] == len(seeds)
    assert by_set["worst_seed"]["chunks"] == int(seeds[np.argmax(chunks)]) and by_set["headroom"]["chunks"] == chunks[clean].max() / int(caps[1])
    again = type(res)(sim)  # the handle survives, and a second call returns the same words
    assert (again.instance_load() == rows).all() and all((a == b).all() for a, b in zip(again.load_stats("chunks"), (hist, census, stats, caps)))
    sim.close()
    heap = amd.BatchSimulator.new(seeds, kw["num_nodes"], delay, queue_capacity=queue_capacity, calendar_queue=False)
    res = heap.loop_until(max_clock)
    assert not heap.layout()["kernel_class"] & (1 << 9) and not res.faults.any()
    rows_heap = check_rows(res)
    assert check_grouped(res, rows_heap, families=(F["chunks"],))[1] == 0 and (rows_heap[:, F["chunks"]] == 0).all()
    assert (rows_heap[clean][:, [0, 1, 2, 3, 5, 6, 14, 15]] == rows[clean][:, [0, 1, 2, 3, 5, 6, 14, 15]]).all()  # (the queue's kind changes no run)
    heap.close()


# ---- 6: every kind of batch ----
KIND_T = 300


@pytest.fixture(scope="module")
def want1024(oracle, amd):
    seeds = np.arange(1, 1025, dtype=np.uint64) * 31 + 5
    return seeds, ref.oracle_rows(oracle, oracle_cfg(oracle, 4, four_sets(amd)[0]), seeds, KIND_T)[0]


@pytest.mark.parametrize("kind", ("run0q", "timed", "reset", "checkpoint"))
def test_every_kind_of_batch_serves_the_load_and_stays_as_it_was(amd, want1024, tmp_path, kind):
    seeds, want = want1024
    ps = four_sets(amd)[0]
    sim = plain(amd, seeds, 4, ps, **(dict(commit_times=True) if kind == "timed" else {}))
    if kind == "reset":
        sim.loop_until(120)
        sim.reset()
    if kind == "checkpoint":
        left, _ = sim.run_steps(KIND_T, 150)
        assert left > 0
        sim.save_checkpoint(str(tmp_path / "ck.bin"))
        sim.close()
        sim = plain(amd, np.zeros(len(seeds), dtype=np.uint64), 4, ps)  # (the seeds live in the state)
        sim.load_checkpoint(str(tmp_path / "ck.bin"))
        res = run_to_end(sim, KIND_T, 200)
    else:
        res = sim.loop_until(KIND_T)
    word = sim.layout()["kernel_class"]
    if kind == "run0q":
        assert word & 16384, word  # lbft_k_run0q ran
    if kind == "timed":
        assert word & 131072, word
    before = res.chain_heads()
    rows = check_rows(res, want)
    check_grouped(res, rows, families=(F["queue"], F["blocks"]))
    assert (res.chain_heads() == before).all() and (type(res)(sim).instance_load() == rows).all()  # nothing was mutated
    sim.close()
