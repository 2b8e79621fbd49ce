"""CPU-side checks of the chain statistics: the arithmetic the device kernel shares with the host (csrc/lbft_chain_rules.h), compiled
into a g++ shim (tests/chain_stats_host.cpp) that walks the logs the way the kernel does, equals the numpy reference written from the
definitions (tests/chain_stats_reference.py) -- on the oracle's histories of weighted, equivocating, lossy and partitioned networks, and
on logs written by hand that no run produces: this is where the audit families show that they fire.  The reference itself is pinned to
figures of the oracle that were obtained before any of this code existed."""
import ctypes as C
import os

import numpy as np
import pytest

import chain_stats_reference as ref
from support import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHUNKS = (1, 2, 7, 64)  # entries side by side in the shim's chain walk (the kernel: 64)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = build_shim(tmp_path_factory.mktemp("chn_host"), "chain_stats_host.cpp", "libchn_host.so", "-Wall", "-Werror")
    vp = C.c_void_p
    L.chn_host.argtypes = [vp] * 7 + [C.c_uint32] * 8 + [vp, vp, vp]
    L.chn_host.restype = C.c_int
    L.chn_workgroups_host.argtypes = [C.c_uint64] * 6
    L.chn_workgroups_host.restype = C.c_uint64
    return L


def run_shim(L, logs, commits, blk_author, blk_time, startup, faults, group_of, groups, width, bins, chunk):
    logs = np.ascontiguousarray(logs, dtype=np.uint32)
    m, n, lcap = logs.shape
    commits = np.ascontiguousarray(commits, dtype=np.uint32)
    blk_author = np.ascontiguousarray(blk_author, dtype=np.uint32)
    blk_time = np.ascontiguousarray(blk_time, dtype=np.int32)
    startup = np.ascontiguousarray(startup, dtype=np.int32)
    assert commits.shape == startup.shape == (m, n) and blk_author.shape == blk_time.shape and blk_author.shape[0] == m
    faults = np.ascontiguousarray(faults if faults is not None else np.zeros(m), dtype=np.uint32)
    group = None if group_of is None else np.ascontiguousarray(group_of, dtype=np.uint32)
    hist = np.zeros((groups, bins), dtype=np.uint64)
    authors = np.zeros((groups, n), dtype=np.uint64)
    stats = np.zeros((groups, ref.CHAIN_STATS), dtype=np.uint64)
    rc = L.chn_host(logs.ctypes.data, commits.ctypes.data, blk_author.ctypes.data, blk_time.ctypes.data, startup.ctypes.data, faults.ctypes.data,
                    None if group is None else group.ctypes.data, m, n, lcap, blk_author.shape[1] - 1, groups, width, bins, chunk,
                    hist.ctypes.data, authors.ctypes.data, stats.ctypes.data)
    assert rc == 0, rc
    return hist, authors, stats


def device_form(histories, counts, lcap=None):
    """Histories of records as the device holds them: logs of block ids (1-based, one id per distinct record of an instance, numbered
    in the order met) and the pool's author / time tables."""
    m, n, cap = histories.shape
    lcap = lcap or cap
    logs = np.zeros((m, n, lcap), dtype=np.uint32)
    pools = []
    for i in range(m):
        ids = {}
        for j in range(n):
            for k in range(min(int(counts[i, j]), lcap)):
                e = histories[i, j, k]
                key = (int(e["proposer"]), int(e["index"]), int(e["time"]))
                logs[i, j, k] = ids.setdefault(key, len(ids) + 1)
        pools.append(sorted(ids, key=ids.get))
    blocks = max(max(len(p) for p in pools), 1)
    blk_author = np.zeros((m, blocks + 1), dtype=np.uint32)
    blk_time = np.zeros((m, blocks + 1), dtype=np.int32)
    for i, pool in enumerate(pools):
        for b, (a, _, t) in enumerate(pool, start=1):
            blk_author[i, b], blk_time[i, b] = a, t
    return logs, blk_author, blk_time


def records_of(logs, commits, blk_author, blk_time):
    """The other way round, for logs written by hand: the records the reference compares (index = the block id: one per block)."""
    m, n, lcap = logs.shape
    hist = np.zeros((m, n, lcap), dtype=ref.COMMIT_DTYPE)
    for i in range(m):
        for j in range(n):
            for k in range(min(int(commits[i, j]), lcap)):
                b = int(logs[i, j, k])
                hist[i, j, k] = (int(blk_author[i, b]), b, int(blk_time[i, b]))
    return hist


def compare(L, logs, commits, blk_author, blk_time, startup, faults, group_of, groups, width, bins, histories=None):
    histories = records_of(logs, commits, blk_author, blk_time) if histories is None else histories
    want = ref.chain_stats(histories, commits, startup, faults, group_of, groups, width, bins, log_capacity=logs.shape[2])
    for chunk in CHUNKS:
        got = run_shim(L, logs, commits, blk_author, blk_time, startup, faults, group_of, groups, width, bins, chunk)
        for name, a, b in zip(("interval_hist", "author_blocks", "stats"), got, want):
            assert (a == b).all(), (name, chunk, width, bins, a, b)
    hist, authors, stats = want
    assert (hist.sum(axis=1) == stats[:, 0]).all() and (authors.sum(axis=1) == stats[:, 4 * ref.LENGTH + 1]).all()
    assert (stats[:, 4 * ref.TENURE + 1] == stats[:, 4 * ref.LENGTH + 1]).all()  # the runs of a chain sum to its length
    return want


# ---- the oracle's histories ----
ORACLE_CASES = {
    "anchor": (dict(num_nodes=4), range(1, 17), 1000),
    "weighted": (dict(num_nodes=5, voting_rights=[5, 1, 1, 1, 1]), range(1, 9), 1000),
    "equivocators": (dict(num_nodes=7, quirks=3, drop_per_million=50000, equivocate_every=3), range(1, 9), 1000),
    "partition": (dict(num_nodes=4, quirks=3, partition_size=2, partition_start=300, partition_end=600), range(1, 17), 1500),
    "no_partition": (dict(num_nodes=4, quirks=3), range(1, 17), 1500),
}


@pytest.fixture(scope="module")
def oracle_cases(oracle):
    return {name: ref.oracle_runs(oracle, oracle.make_config(**kw), seeds, clock) for name, (kw, seeds, clock) in ORACLE_CASES.items()}


def test_reference_is_pinned_to_the_oracle_figures(oracle_cases):
    """Figures of the oracle (reference CLI defaults: mean 10, variance 4) that the feature was chosen by, as literals."""
    fam, authors = ref.samples(*oracle_cases["anchor"], None, None, 1)
    f = fam[0]
    assert f[ref.LENGTH].sum() == 526 and authors[0].tolist() == [134, 112, 124, 156]
    assert len(f[ref.TENURE]) == 361 and len(f[ref.TENURE]) - len(f[ref.LENGTH]) == 345  # handovers + one run per chain
    assert f[ref.INTERVAL].min() == 15 and f[ref.INTERVAL].max() == 64 and f[ref.LAG].max() <= 2
    assert f[ref.DIFFERING].sum() == 0 and f[ref.INVERSIONS].sum() == 0
    fam, authors = ref.samples(*oracle_cases["weighted"], None, None, 1)
    assert fam[0][ref.LENGTH].sum() == 290 and authors[0].tolist() == [154, 36, 47, 27, 26]
    fam, authors = ref.samples(*oracle_cases["equivocators"], None, None, 1)
    assert fam[0][ref.LENGTH].sum() == 81 and authors[0, [0, 3, 6]].tolist() == [0, 0, 1]
    assert ref.samples(*oracle_cases["partition"], None, None, 1)[0][0][ref.INTERVAL].max() == 463
    assert ref.samples(*oracle_cases["no_partition"], None, None, 1)[0][0][ref.INTERVAL].max() == 64
    for case in oracle_cases.values():  # agreement: what a BFT simulator is there to show
        fam, _ = ref.samples(*case, None, None, 1)
        assert fam[0][ref.DIFFERING].sum() == 0 and fam[0][ref.INVERSIONS].sum() == 0 and fam[0][ref.INTERVAL].min() >= 14


@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_shim_equals_the_reference_on_oracle_histories(shim, oracle_cases, name):
    histories, counts, startup = oracle_cases[name]
    logs, blk_author, blk_time = device_form(histories, counts)
    m = len(counts)
    group_of = np.arange(m) % 3
    for width, bins in ((1, int(ORACLE_CASES[name][2]) + 1), (7, 5), (1, 1)):
        compare(shim, logs, counts, blk_author, blk_time, startup, None, None, 1, width, bins, histories)
        compare(shim, logs, counts, blk_author, blk_time, startup, None, group_of, 3, width, bins, histories)


# ---- logs written by hand ----
def make(n, lcap, blocks, chains, commits, startup=None):
    """One instance: chains[j] = node j's log (block ids), blocks = [(author, time)] for ids 1 ..; commits[j] may differ from len(chains[j])."""
    logs = np.zeros((1, n, lcap), dtype=np.uint32)
    for j, c in enumerate(chains):
        logs[0, j, :len(c)] = c
    a = np.zeros((1, len(blocks) + 1), dtype=np.uint32)
    t = np.zeros((1, len(blocks) + 1), dtype=np.int32)
    for b, (au, ti) in enumerate(blocks, start=1):
        a[0, b], t[0, b] = au, ti
    return dict(logs=logs, commits=np.array([commits], dtype=np.uint32), blk_author=a, blk_time=t,
                startup=np.array([startup if startup is not None else [0] * n], dtype=np.int32))


def batch(instances):
    """Instances of one shape (n, lcap) with pools of different sizes, as one batch."""
    blocks = max(x["blk_author"].shape[1] for x in instances)
    out = {}
    for key in ("logs", "commits", "startup"):
        out[key] = np.concatenate([x[key] for x in instances])
    for key in ("blk_author", "blk_time"):
        out[key] = np.concatenate([np.pad(x[key], ((0, 0), (0, blocks - x[key].shape[1]))) for x in instances])
    return out


def run(L, x, faults=None, group_of=None, groups=1, width=1, bins=4000):
    return compare(L, x["logs"], x["commits"], x["blk_author"], x["blk_time"], x["startup"], faults, group_of, groups, width, bins)


def line(length, n, period=1, step=20):
    """A pool of `length` blocks proposed `step` apart, the author changing every `period` blocks, and the chain 1 .. length."""
    return [((k // period) % n, 10 + step * k) for k in range(length)], list(range(1, length + 1))


def fam_of(stats, f):
    return stats[0, 4 * f:4 * f + 4].tolist()


def test_one_differing_entry_is_counted_wherever_it_lies(shim):
    n, lcap, length = 4, 200, 130
    blocks, chain = line(length, n)
    blocks.append((3, 5))  # block 131: the stranger
    for node, nc, at in ((1, 130, 0), (2, 100, 99), (3, 130, 63), (1, 130, 64), (2, 129, 128), (3, 65, 64)):  # k = 0, k = nc_j - 1, chunk seams
        chains = [list(chain[:length]) for _ in range(n)]
        commits = [length] * n
        commits[node] = nc
        chains[node] = chains[node][:nc]
        chains[node][at] = length + 1
        _, _, stats = run(shim, make(n, lcap, blocks, chains, commits))
        assert fam_of(stats, ref.DIFFERING) == [1, 1, 1, 1], (node, nc, at)
        assert fam_of(stats, ref.LENGTH) == [1, length, length, length] and fam_of(stats, ref.INVERSIONS) == [1, 0, 0, 0]
    # the stranger past a node's count is not looked at; two nodes differing in three places
    chains = [list(chain) for _ in range(n)]
    chains[1][100] = length + 1
    _, _, stats = run(shim, make(n, lcap, blocks, chains, [length, 100, length, length]))
    assert fam_of(stats, ref.DIFFERING) == [1, 0, 0, 0]
    chains[2][0] = chains[2][129] = chains[3][64] = length + 1
    _, _, stats = run(shim, make(n, lcap, blocks, chains, [length] * n))
    assert fam_of(stats, ref.DIFFERING) == [1, 4, 4, 4]


def test_reference_node_is_the_longest_log_and_ties_go_to_the_lowest(shim):
    n, lcap = 4, 100
    blocks, chain = line(70, n)
    other = [(2, 7 + 20 * k) for k in range(70)]  # a second pool half: ids 71 .. 140, authored by node 2
    x = make(n, lcap, blocks + other, [chain[:10], chain[:60], list(range(71, 141)), chain[:66]], [10, 60, 70, 66])
    _, authors, stats = run(shim, x)  # node 2 is longer than every other: its log is the chain
    assert fam_of(stats, ref.LENGTH) == [1, 70, 70, 70] and authors[0].tolist() == [0, 0, 70, 0]
    assert fam_of(stats, ref.LAG) == [4, 60 + 10 + 0 + 4, 0, 60] and fam_of(stats, ref.DIFFERING) == [1, 136, 136, 136]
    assert fam_of(stats, ref.TENURE) == [1, 70, 70, 70]
    x = make(n, lcap, blocks + other, [chain[:10], chain[:66], list(range(71, 137)), chain[:66]], [10, 66, 66, 66])
    _, authors, stats = run(shim, x)  # a tie of nodes 1, 2, 3: node 1
    assert authors[0].tolist() == [17, 17, 16, 16] and fam_of(stats, ref.DIFFERING) == [1, 66, 66, 66]  # (node 2 alone differs)
    # a commit count past the capacity counts as the capacity
    x = make(n, 64, blocks, [chain[:64], chain[:64], chain[:3], chain[:64]], [64, 900, 3, 65])
    _, _, stats = run(shim, x)
    assert fam_of(stats, ref.LENGTH) == [1, 64, 64, 64] and fam_of(stats, ref.LAG) == [4, 61, 0, 61]


def test_an_inversion_is_counted_and_its_interval_clamped(shim):
    n, lcap = 4, 100
    blocks, chain = line(66, n)
    blocks[40] = (0, 10 + 20 * 39 - 5)  # entry 40 proposed 5 before entry 39
    blocks[64] = (0, 10 + 20 * 63 - 1)  # and one across the chunk seam: entry 64 before entry 63
    hist, _, stats = run(shim, make(n, lcap, blocks, [chain] * n, [66] * n))
    assert fam_of(stats, ref.INVERSIONS) == [1, 2, 2, 2]
    assert fam_of(stats, ref.INTERVAL) == [65, 61 * 20 + 45 + 41, 0, 45] and hist[0, 0] == 2
    # the startup time of the author is part of the proposal time: the same pool, node 1's clock 1000 ahead
    blocks, chain = line(8, n)
    _, _, stats = run(shim, make(n, lcap, blocks, [chain] * n, [8] * n, startup=[0, 1000, 0, 0]), bins=2000)
    # authors 0 1 2 3 0 1 2 3: into node 1 +1020, out of it back 980 (an inversion, interval 0)
    assert fam_of(stats, ref.INVERSIONS) == [1, 2, 2, 2] and fam_of(stats, ref.INTERVAL) == [7, 1020 + 20 + 20 + 1020 + 20, 0, 1020]


@pytest.mark.parametrize("length,period", [(64, 64), (65, 64), (66, 65), (64, 63), (130, 63), (200, 150), (129, 1), (128, 2), (70, 7)])
def test_tenure_runs_around_the_chunk_seams(shim, length, period):
    """Runs that end exactly at, one before and one after the seam of a 64-entry chunk, a run over three chunks, and every entry a run."""
    n, lcap = 4, 256
    blocks, chain = line(length, n, period)
    _, authors, stats = run(shim, make(n, lcap, blocks, [chain] * n, [length] * n))
    runs = [min(period, length - s) for s in range(0, length, period)]
    assert fam_of(stats, ref.TENURE) == [len(runs), length, min(runs), max(runs)]
    assert authors[0].sum() == length


@pytest.mark.parametrize("length", [0, 1, 2, 63, 64, 65, 128, 129])
def test_chain_lengths_around_the_chunk_size(shim, length):
    n, lcap = 3, 130
    blocks, chain = line(max(length, 1), n)
    _, authors, stats = run(shim, make(n, lcap, blocks, [chain[:length]] * n, [length] * n))
    assert fam_of(stats, ref.LENGTH) == [1, length, length, length] and fam_of(stats, ref.LAG) == [3, 0, 0, 0]
    assert fam_of(stats, ref.INTERVAL) == ([length - 1, 20 * (length - 1), 20, 20] if length > 1 else [0, 0, 0, 0])
    assert fam_of(stats, ref.TENURE) == ([length, length, 1, 1] if length else [0, 0, 0, 0])
    assert fam_of(stats, ref.DIFFERING) == [1, 0, 0, 0] and authors[0].sum() == length


def test_faulted_instances_empty_groups_and_binning_edges(shim):
    n, lcap = 4, 140
    blocks, chain = line(130, n, 3)
    good = make(n, lcap, blocks, [chain, chain[:128], chain[:129], chain], [130, 128, 129, 130])
    short = make(n, lcap, blocks, [chain[:5]] * n, [5] * n)
    nothing = make(n, lcap, blocks, [[]] * n, [0] * n)  # all nodes with nc = 0
    garbage = make(n, lcap, blocks, [[7] * 140, [3] * 140, [], [1] * 140], [4000000000, 17, 0, 140])
    garbage["logs"][0, 2] = 0xdeadbeef  # ids that name no block: a faulted instance is not looked at
    x = batch([good, garbage, short, nothing, good])
    faults = np.array([0, 8, 0, 0, 1 << 11], dtype=np.uint32)
    group_of = np.array([0, 0, 2, 2, 3])  # group 1 is empty, group 3 holds one faulted instance alone
    for width, bins in ((1, 100), (1, 1), (1000, 4), (2 ** 32 - 1, 2), (7, 2), (1, ref.LDS_BINS + 1)):
        hist, authors, stats = run(shim, x, faults, group_of, 4, width, bins)
        assert not stats[1].any() and not stats[3].any() and not hist[1].any() and not authors[3].any()
        assert stats[0, 0] == 129 and stats[0, 4 * ref.LENGTH] == 1 and fam_of(stats[2:3], ref.LENGTH) == [2, 5, 0, 5]
        assert fam_of(stats[2:3], ref.LAG) == [8, 0, 0, 0]
        if bins == 1 or width > 20:  # bins = 1, or a width larger than every sample: everything in bin 0
            assert hist[0, 0] == 129 and hist[2, 0] == 4
    hist, _, _ = run(shim, x, faults, group_of, 4, 7, 2)
    assert hist[0].tolist() == [0, 129]  # the last bin also counts everything above it
    run(shim, x, faults, None, 1, 1, 50)  # the plain-batch form: one group, no group array


def test_grid_rule_of_the_launcher(shim):
    """lbft_cs_launch_chain's call of gs_workgroups: about 1024 workgroups in all, never more than the steps of a workgroup's stride, and at
    least one more than (largest group x max(lcap, n)) >> 31, so that no u32 LDS bin can wrap."""
    src = open(os.path.join(ROOT, "librabft_simulator_amd", "csrc", "lbft_chain_stats.hip")).read()
    assert "#define LBFT_CS_WORKGROUPS 1024u" in src and "#define LBFT_CS_BLOCK 256" in src and "#define LBFT_CS_LDS_BINS %d\n" % ref.LDS_BINS in src.replace("  //", "\n//")
    for groups, max_group, lcap, n, want in ((1, 65536, 64, 4, 1024), (64, 1024, 64, 4, 16), (256, 1, 64, 4, 1), (1, 7, 64, 100, 2),
                                             (2048, 5000, 64, 4, 1), (256, 1 << 24, 4096, 4, 33), (1, 1 << 26, 16, 128, 1024), (1, 1 << 26, 65536, 128, 2049)):
        assert shim.chn_workgroups_host(1024, groups, max_group, 4, lcap, n) == want, (groups, max_group, lcap, n)
