"""CPU-side checks of commit finality: the arithmetic the device kernel shares with the host (csrc/lbft_commit_finality.h), compiled into
a g++ shim (tests/commit_finality_host.cpp) that walks the columns the way the kernel does, equals the numpy reference written from the
definitions (tests/commit_finality_reference.py) -- on drawn data that no run produces (ties, lagging rows, holes, counts past the
capacity, rotating weighted rights), on columns written by hand whose answers are known, and on commit times derived from the oracle.
The reference alone then shows what the feature is for: a node that is cut off moves the all-node finality of the entries it misses, and
the bulk of the quorum's stays where it was."""
import ctypes as C
import os

import numpy as np
import pytest

import chain_stats_reference as chain_ref
import commit_finality_reference as ref
from support import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (1, 5, 64)  # entries side by side in the shim's walk (the kernel: 64)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = build_shim(tmp_path_factory.mktemp("fin_host"), "commit_finality_host.cpp", "libfin_host.so", "-Wall", "-Werror")
    vp = C.c_void_p
    L.fin_host.argtypes = [vp] * 9 + [C.c_uint32, C.c_uint64] + [C.c_uint32] * 10 + [vp] * 4
    L.fin_host.restype = C.c_int
    L.fin_rights_index_host.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
    L.fin_rights_index_host.restype = C.c_uint32
    L.fin_workgroups_host.argtypes = [C.c_uint64] * 5
    L.fin_workgroups_host.restype = C.c_uint64
    return L


def run_shim(L, x, faults, group_of, groups, width, bins, chunk):
    ct = np.ascontiguousarray(x["ctimes"], dtype=np.int32)
    logs = np.ascontiguousarray(x["logs"], dtype=np.uint32)
    m, n, lcap = logs.shape
    assert ct.shape == logs.shape
    commits = np.ascontiguousarray(x["commits"], dtype=np.uint32)
    blk_author = np.ascontiguousarray(x["blk_author"], dtype=np.uint32)
    blk_time = np.ascontiguousarray(x["blk_time"], dtype=np.int32)
    startup = np.ascontiguousarray(x["startup"], dtype=np.int32)
    assert commits.shape == startup.shape == (m, n) and blk_author.shape == blk_time.shape and blk_author.shape[0] == m
    faults = np.ascontiguousarray(faults if faults is not None else np.zeros(m), dtype=np.uint32)
    group = None if group_of is None else np.ascontiguousarray(group_of, dtype=np.uint32)
    rights = None if x.get("rights") is None else np.ascontiguousarray(x["rights"], dtype=np.uint32)
    total, quorum, _ = ref.thresholds([1] * n if rights is None else rights)
    fin = np.zeros((groups, bins), dtype=np.uint64)
    spread = np.zeros((groups, bins), dtype=np.uint64)
    first = np.zeros((groups, n), dtype=np.uint64)
    stats = np.zeros((groups, ref.FINALITY_STATS), dtype=np.uint64)
    rc = L.fin_host(ct.ctypes.data, logs.ctypes.data, commits.ctypes.data, blk_author.ctypes.data, blk_time.ctypes.data, startup.ctypes.data,
                    faults.ctypes.data, None if group is None else group.ctypes.data, None if rights is None else rights.ctypes.data,
                    x.get("rot", 0), x.get("cpe", 30000), total, quorum, m, n, lcap, blk_author.shape[1] - 1, groups, width, bins, chunk,
                    fin.ctypes.data, spread.ctypes.data, first.ctypes.data, stats.ctypes.data)
    assert rc == 0, rc
    return fin, spread, first, stats


def records_of(x, faults=None):
    """The histories the reference reads, from logs of block ids and the pool (a faulted instance's rows are not looked at)."""
    logs, commits = x["logs"], x["commits"]
    m, n, lcap = logs.shape
    hist = np.zeros((m, n, lcap), dtype=chain_ref.COMMIT_DTYPE)
    for i in range(m):
        if faults is not None and faults[i]:
            continue
        for j in range(n):
            for k in range(min(int(commits[i, j]), lcap)):
                b = int(logs[i, j, k])
                hist[i, j, k] = (int(x["blk_author"][i, b]), b, int(x["blk_time"][i, b]))
    return hist


def compare(L, x, faults=None, group_of=None, groups=1, binnings=((1, 600),), histories=None):
    histories = records_of(x, faults) if histories is None else histories
    fam, fc = ref.samples(x["ctimes"], x["commits"], histories, x["startup"], faults, x.get("rights"), x.get("rot", 0), x.get("cpe", 30000),
                          group_of, groups, log_capacity=x["logs"].shape[2])
    for width, bins in binnings:
        want = ref.bin_finality(fam, fc, width, bins)
        for chunk in CHUNKS:
            got = run_shim(L, x, faults, group_of, groups, width, bins, chunk)
            for name, a, b in zip(("finality_hist", "spread_hist", "first_committer", "stats"), got, want):
                assert (a == b).all(), (name, chunk, width, bins, a, b)
    fin, spread, first, stats = want
    assert (fin.sum(axis=1) == stats[:, 4 * ref.QUORUM]).all() and (spread.sum(axis=1) == stats[:, 4 * ref.SPREAD]).all()
    assert (first.sum(axis=1) == stats[:, 4 * ref.FIRST]).all() and (stats[:, 4 * ref.ALL] == stats[:, 4 * ref.SPREAD]).all()
    return fam, want


# ---- drawn data ----
def draw(rng, m, n, lcap, rights=None, rot=0, cpe=30000):
    """Instances no run produces: every entry's times drawn from a handful of values (ties), rows of unequal length, holes inside
    the rows, garbage past the counts, one count past the capacity, one all-empty instance."""
    blocks = lcap
    blk_author = rng.integers(0, n, size=(m, blocks + 1)).astype(np.uint32)
    blk_time = rng.integers(0, 40, size=(m, blocks + 1)).astype(np.int32)
    startup = rng.integers(0, 20, size=(m, n)).astype(np.int32)
    logs = np.stack([np.stack([rng.permutation(blocks) + 1 for _ in range(n)]) for _ in range(m)]).astype(np.uint32)
    commits = rng.integers(0, lcap + 1, size=(m, n)).astype(np.uint32)
    commits[0, rng.integers(0, n)] = 4000000000  # past the capacity: counts as the capacity
    commits[1] = 0  # an all-empty instance
    if m > 3:
        commits[3] = lcap  # every node a committer of every entry but the holes
    ctimes = (60 + 3 * np.arange(lcap)[None, None, :] + rng.integers(0, 4, size=(m, n, lcap))).astype(np.int32)  # >= 60 > any proposal time
    ctimes[rng.random(size=ctimes.shape) < 0.08] = -1  # holes
    past = np.arange(lcap)[None, None, :] >= np.minimum(commits, lcap)[:, :, None]
    ctimes[past] = np.where(rng.random(size=int(past.sum())) < 0.5, 7, -1)  # what lies past a count is not looked at
    return dict(ctimes=ctimes, logs=logs, commits=commits, blk_author=blk_author, blk_time=blk_time, startup=startup, rights=rights, rot=rot, cpe=cpe)


@pytest.mark.parametrize("n,rights,rot,cpe", [(2, None, 0, 30000), (4, None, 0, 30000), (7, [3, 1, 1, 2, 1, 1, 4], 2, 5), (32, None, 0, 30000),
                                              (32, list(range(1, 33)), 31, 1), (5, [5, 1, 1, 1, 1], 1, 3), (4, [0, 1, 2, 0], 1, 2)])
def test_shim_equals_the_reference_on_drawn_data(shim, n, rights, rot, cpe):
    rng = np.random.default_rng(1000 + n + rot)
    m, lcap = 7, 70 if n < 32 else 66  # more than one 64-entry chunk
    x = draw(rng, m, n, lcap, rights, rot, cpe)
    faults = np.array([0, 0, 1 << 3, 0, 0, 0, 0], dtype=np.uint32)  # a faulted instance
    x["logs"][2] = 0xdeadbeef  # ... whose rows are not looked at
    fam, (fin, spread, first, stats) = compare(shim, x, faults, None, 1, ((1, 600), (7, 5), (1, 1), (1, ref.LDS_BINS + 3)))
    f = fam[0]
    assert len(f[ref.OPEN]) == m - 1 and len(f[ref.ALL]) > 0 and len(f[ref.FIRST]) > len(f[ref.QUORUM]) >= len(f[ref.ALL])
    assert f[ref.OPEN].sum() == len(f[ref.FIRST]) - len(f[ref.QUORUM]) > 0
    assert (f[ref.SPREAD] <= 3).all()  # every entry's times are drawn from four values: ties in every column
    group_of = np.array([0, 0, 2, 2, 3, 3, 0])  # group 1 is empty
    _, (fin, _, first, stats) = compare(shim, x, faults, group_of, 4, ((1, 600), (3, 9)))
    assert not stats[1].any() and not fin[1].any() and not first[1].any()
    assert stats[2, 4 * ref.OPEN] == 1 and stats[0, 4 * ref.OPEN] == 3  # the faulted instance gives no `open` sample


def test_the_right_of_a_node_changes_inside_a_chunk(shim):
    """Rights [5, 1, 1, 1, 1] rotating by 1 every 3 entries: total 9, quorum 7, valid 3.  The heavy right sits on node (5 - e) % 5 in
    epoch e.  Every entry is committed by nodes 0 .. 3 at times 100 + j and by node 4 never: the quorum is reached with the heavy node
    and two more, and not at all in the epochs in which node 4 holds the 5."""
    n, lcap, rights = 5, 70, [5, 1, 1, 1, 1]
    for j in range(n):
        for k in range(lcap):
            assert rights[shim.fin_rights_index_host(j, k, 3, 1, n)] == (5 if (j + k // 3) % n == 0 else 1)
    assert shim.fin_rights_index_host(3, 65533, 1, 31, 32) == (3 + 65533 * 31) % 32 and shim.fin_rights_index_host(3, 9, 1 << 40, 31, 32) == 3
    blocks = [(0, 0)] * lcap
    x = dict(logs=np.tile(np.arange(1, lcap + 1, dtype=np.uint32), (1, n, 1)), commits=np.array([[lcap] * 4 + [0]], dtype=np.uint32),
             blk_author=np.zeros((1, len(blocks) + 1), dtype=np.uint32), blk_time=np.zeros((1, len(blocks) + 1), dtype=np.int32),
             startup=np.zeros((1, n), dtype=np.int32), rights=rights, rot=1, cpe=3)
    x["ctimes"] = np.broadcast_to(100 + np.arange(n, dtype=np.int32)[None, :, None], (1, n, lcap)).copy()
    fam, (fin, spread, first, stats) = compare(shim, x)
    heavy = [(n - k // 3) % n for k in range(lcap)]
    want_quorum = [100 + max(h, 2) for h in heavy if h != 4]  # 5 + 1 + 1 = 7: the heavy node and two light ones
    want_valid = [100 + min(h, 2) for h in heavy]  # the heavy node alone, or the first three light ones
    assert fam[0][ref.QUORUM].tolist() == want_quorum and fam[0][ref.VALID].tolist() == want_valid
    assert fam[0][ref.OPEN].tolist() == [sum(1 for h in heavy if h == 4)] and len(fam[0][ref.ALL]) == 0
    assert first[0].tolist() == [lcap, 0, 0, 0, 0] and fam[0][ref.FIRST].tolist() == [100] * lcap
    # the same data under unit rights (quorum 4 of 5, valid 2): reached everywhere, by the fourth and the second committer
    x["rights"], x["rot"] = None, 0
    fam, _ = compare(shim, x)
    assert fam[0][ref.QUORUM].tolist() == [103] * lcap and fam[0][ref.OPEN].tolist() == [0] and fam[0][ref.VALID].tolist() == [101] * lcap


def test_committers_holding_exactly_the_threshold_and_one_less(shim):
    """4 nodes, unit rights: quorum 3, valid 2.  Columns written by hand, one entry each, proposal time 10."""
    n, lcap = 4, 8
    cols = [[50, 50, 50, 50], [50, 40, -1, -1], [50, 40, 60, -1], [-1, -1, -1, 70], [-1, -1, -1, -1], [90, 80, 80, 70], [30, 30, 31, 31], [45, -1, 44, 44]]
    x = dict(ctimes=np.array(cols, dtype=np.int32).T[None].copy(), logs=np.tile(np.arange(1, lcap + 1, dtype=np.uint32), (1, n, 1)),
             commits=np.array([[lcap] * n], dtype=np.uint32), blk_author=np.zeros((1, lcap + 1), dtype=np.uint32),
             blk_time=np.full((1, lcap + 1), 10, dtype=np.int32), startup=np.zeros((1, n), dtype=np.int32))
    fam, (_, _, first, stats) = compare(shim, x)
    f = fam[0]
    assert f[ref.FIRST].tolist() == [40, 30, 30, 60, 60, 20, 34]
    assert f[ref.VALID].tolist() == [40, 40, 40, 70, 20, 34]  # two committers: exactly T; one: T - 1
    assert f[ref.QUORUM].tolist() == [40, 50, 70, 21, 35]  # three committers: exactly T; two: T - 1
    assert f[ref.ALL].tolist() == [40, 80, 21] and f[ref.SPREAD].tolist() == [0, 20, 1]
    assert f[ref.OPEN].tolist() == [2] and first[0].tolist() == [2, 2, 1, 2]  # (entry 4 has no committer: it is not open either)
    # rows of unequal length: the same columns with node 3 at 5 commits -- its entries 5 .. 7 are no commits whatever the buffer holds
    x["commits"][0, 3] = 5
    fam, (_, _, first, _) = compare(shim, x)
    assert fam[0][ref.FIRST].tolist() == [40, 30, 30, 60, 70, 20, 34] and fam[0][ref.QUORUM].tolist() == [40, 50, 80, 21]
    assert fam[0][ref.OPEN].tolist() == [3] and first[0].tolist() == [2, 3, 1, 1] and fam[0][ref.ALL].tolist() == [40]


def test_grid_rule_of_the_launcher(shim):
    src = open(os.path.join(ROOT, "librabft_simulator_amd", "csrc", "lbft_commit_times.hip")).read()
    assert "#define LBFT_FN_WORKGROUPS 1024u" in src and "#define LBFT_FN_BLOCK 256" in src
    assert "#define LBFT_FN_LDS_BINS %d " % ref.LDS_BINS in src
    for groups, max_group, lcap, want in ((1, 65536, 64, 1024), (64, 1024, 64, 16), (256, 1, 64, 1), (1, 7, 64, 2), (256, 1 << 24, 4096, 33)):
        assert shim.fin_workgroups_host(1024, groups, max_group, 4, lcap) == want, (groups, max_group, lcap)


# ---- the oracle's commit times ----
def device_form(histories, counts, ct):
    """Histories of records and commit times as the device holds them (test_chain_stats_host.device_form, plus the int32 buffer)."""
    m, n, cap = histories.shape
    logs = np.zeros((m, n, cap), dtype=np.uint32)
    pools = []
    for i in range(m):
        ids = {}
        for j in range(n):
            for k in range(int(counts[i, j])):
                e = histories[i, j, k]
                logs[i, j, k] = ids.setdefault((int(e["proposer"]), int(e["index"]), int(e["time"])), len(ids) + 1)
        pools.append(sorted(ids, key=ids.get))
    blocks = max(max(len(p) for p in pools), 1)
    blk_author = np.zeros((m, blocks + 1), dtype=np.uint32)
    blk_time = np.zeros((m, blocks + 1), dtype=np.int32)
    for i, pool in enumerate(pools):
        for b, (a, _, t) in enumerate(pool, start=1):
            blk_author[i, b], blk_time[i, b] = a, t
    ctimes = np.full((m, n, cap), -1, dtype=np.int32)
    ctimes[:, :, :min(cap, ct.shape[2])] = ct[:, :, :cap]
    return logs, blk_author, blk_time, ctimes


def oracle_case(oracle, cfg, seeds, max_clock, **kw):
    import commit_times_oracle as cto
    histories, counts, startup = chain_ref.oracle_runs(oracle, cfg, seeds, max_clock)
    ct = cto.commit_times(oracle, cfg, seeds, max_clock, histories.shape[2])
    assert ((ct >= 0).sum(axis=2) == counts).all()
    logs, blk_author, blk_time, ctimes = device_form(histories, counts, ct)
    return dict(ctimes=ctimes, logs=logs, commits=counts, blk_author=blk_author, blk_time=blk_time, startup=startup, **kw), histories


def test_shim_equals_the_reference_on_oracle_commit_times(shim, oracle):
    n, seeds, max_clock = 4, range(1, 17), 300
    x, histories = oracle_case(oracle, oracle.make_config(num_nodes=n), seeds, max_clock)
    fam, (fin, spread, first, stats) = compare(shim, x, binnings=((1, max_clock + 1), (7, 5), (1, 1)), histories=histories)
    f = fam[0]
    assert len(f[ref.FIRST]) == int(x["commits"].max(axis=1).sum()) and (f[ref.QUORUM] <= max_clock).all()
    assert len(f[ref.ALL]) > 0 and (f[ref.FIRST][:1] > 0).all() and (f[ref.OPEN] <= 2).all()
    for s in (f[ref.FIRST], f[ref.VALID], f[ref.QUORUM], f[ref.ALL]):
        assert s.min() >= 20  # a commit needs a 3-chain: two more rounds of proposals and votes at a mean delay of 10


def scenario(oracle, size):
    """The two-set scenario of commit_timeline_reference.scenario_oracle -- a control set and a set with nodes [0, size) of 4 cut off during
    [300, 600), quirks = 3, seeds 1..32 per set, clock 1500 -- with what finality needs besides the commit times: histories and startup
    times.  size = 2 is that scenario itself."""
    import commit_times_oracle as cto
    import commit_timeline_reference as tl
    sc = tl.SCENARIO
    per = sc["seeds_per_set"]
    set_of = np.repeat(np.arange(2), per).astype(np.uint32)
    seeds = np.tile(np.arange(1, per + 1), 2).astype(np.uint64)
    _, start, end = sc["partition"]
    kw = dict(num_nodes=sc["nodes"], mean=sc["mean"], variance=sc["variance"], quirks=sc["quirks"], math_mode=1)
    configs = [oracle.make_config(**kw), oracle.make_config(partition_size=size, partition_start=start, partition_end=end, **kw)]
    histories, counts, startup = chain_ref.concat([chain_ref.oracle_runs(oracle, configs[k], seeds[set_of == k], sc["max_clock"]) for k in range(2)])
    ct = cto.param_set_commit_times(oracle, configs, set_of, seeds, sc["max_clock"], histories.shape[2])
    assert ((ct >= 0).sum(axis=2) == counts).all()
    return ct, counts, histories, startup, set_of


def test_a_partition_moves_the_all_node_finality_and_not_the_quorums(oracle):
    """The reference alone, on oracle-derived commit times.  In commit_timeline_reference's scenario nodes {0, 1} of 4 are cut off: neither
    side holds a quorum (3 of 4), a node of the cut-off side IS needed for it, nobody commits during the partition and the quorum's time
    moves with the all-node time (0.99 quantiles 464 and 465 against the control's 145 and 147).  So the partition here cuts off node 0
    alone, everything else as in that scenario: the other three hold a quorum, node 0 commits what it missed after the partition
    heals.  Observed (control -> partition), quantiles by the inverted-CDF rule:
      all:    0.5: 80 -> 82, 0.9: 130 -> 353, max 176 -> 727       quorum: 0.5: 79 -> 80, 0.9: 128 -> 139, max 173 -> 725
    The all-node finality of one entry in ten grows by the length of the partition while the quorum's 0.9 quantile moves by 11 ticks.
    The quorum's maximum does move: the three connected nodes stall as well for a while (rounds led by the absent node time out, and
    the pacemaker's round durations grow), so some entries proposed before the cut are committed by everybody only after it."""
    ct, counts, histories, startup, set_of = scenario(oracle, 1)
    fam, _ = ref.samples(ct, counts, histories, startup, None, None, 0, 30000, set_of, 2)
    control, cut = fam

    def q(s, p):
        return int(np.quantile(s, p, method="inverted_cdf"))
    print("control:", [ref._stat(s) for s in control], "partition:", [ref._stat(s) for s in cut])
    print("quantiles 0.5 / 0.9 (quorum, all):", [[(q(f[x], 0.5), q(f[x], 0.9)) for x in (ref.QUORUM, ref.ALL)] for f in fam])
    assert cut[ref.ALL].max() > control[ref.ALL].max() + 500 and cut[ref.SPREAD].max() > control[ref.SPREAD].max() + 500
    assert q(cut[ref.ALL], 0.9) > q(control[ref.ALL], 0.9) + 200  # the length of the partition, less what was under way
    assert q(cut[ref.QUORUM], 0.9) <= q(control[ref.QUORUM], 0.9) + 15
    assert abs(q(cut[ref.QUORUM], 0.5) - q(control[ref.QUORUM], 0.5)) <= 2
    assert control[ref.SPREAD].max() < 20 and q(cut[ref.SPREAD], 0.5) <= q(control[ref.SPREAD], 0.5) + 2
    for f in fam:  # what holds by definition
        assert len(f[ref.ALL]) == len(f[ref.SPREAD]) <= len(f[ref.QUORUM]) <= len(f[ref.VALID]) <= len(f[ref.FIRST])
        assert f[ref.OPEN].sum() == len(f[ref.FIRST]) - len(f[ref.QUORUM])


def test_the_entry_index_gives_the_epoch_of_its_block(oracle):
    """e_k = k // commands_per_epoch is the epoch of entry k's block: on the rotation case every node's final epoch is its commit count //
    commands_per_epoch (a chain's blocks of epoch e have depths e * cpe + 1 .. (e + 1) * cpe, commit_block's boundary rule: after c commits
    a node has crossed c // cpe boundaries)."""
    cpe = 3
    cfg = oracle.make_config(num_nodes=5, voting_rights=[5, 1, 1, 1, 1], commands_per_epoch=cpe, rights_rotation=1, quirks=3)
    for seed in range(1, 9):
        sim = oracle.OracleSim(cfg, seed).run_until(1500)
        counts, epochs = np.array(sim.commit_counts(), dtype=np.int64), np.array(sim.epochs(), dtype=np.int64)
        sim.close()
        assert counts.min() > 2 * cpe  # several epoch changes in every run
        assert (epochs == counts // cpe).all(), (seed, epochs, counts)
