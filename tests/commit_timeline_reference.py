"""TEST INFRASTRUCTURE: numpy reference of the commit timelines (include/lbft.h: lbft_batch_commit_series / lbft_batch_commit_stalls),
written from the definitions, row by row, with none of the library's code.

For a node: nc = min(commit count, log capacity), c[0 .. nc) its recorded commit times, its commit instants t_1 < ... < t_r the distinct
values of c, which cut [0, max_clock] into r + 1 intervals.  Instances with a non-zero fault word are skipped."""
import numpy as np

GAPS, FIRST, TAIL, LONGEST = range(4)
LDS_BINS = 8192  # LBFT_HIST_LDS_BINS: the device bins wider histograms in passes of this many bins


def _rows(commit_times, commit_counts, faults, group_of):
    ct = np.asarray(commit_times)
    m, n, cap = ct.shape
    counts = np.minimum(np.asarray(commit_counts).astype(np.int64), cap)
    faults = np.zeros(m, dtype=np.uint32) if faults is None else np.asarray(faults)
    group_of = np.zeros(m, dtype=np.int64) if group_of is None else np.asarray(group_of).astype(np.int64)
    for i in range(m):
        if faults[i] != 0:
            continue
        for j in range(n):
            c = ct[i, j, :counts[i, j]].astype(np.int64)
            assert (c >= 0).all() and (np.diff(c) >= 0).all(), (i, j)
            yield int(group_of[i]), c


def _stat(samples):
    s = np.asarray(samples, dtype=np.int64)
    return (len(s), int(s.sum()), int(s.min()), int(s.max())) if len(s) else (0, 0, 0, 0)


def series(commit_times, commit_counts, faults, group_of, groups, width, bins):
    """[groups, bins] uint64: one sample per committed entry, in bin min(c // width, bins - 1)."""
    ct = np.asarray(commit_times).astype(np.int64)
    m, n, cap = ct.shape
    counts = np.minimum(np.asarray(commit_counts).astype(np.int64), cap)
    entry = np.arange(cap)[None, None, :] < counts[:, :, None]
    if faults is not None:
        entry &= (np.asarray(faults) == 0)[:, None, None]
    group_of = np.zeros(m, dtype=np.int64) if group_of is None else np.asarray(group_of).astype(np.int64)
    g = np.broadcast_to(group_of[:, None, None], ct.shape)[entry]
    c = ct[entry]
    assert (c >= 0).all()
    flat = np.bincount(g * bins + np.minimum(c // width, bins - 1), minlength=groups * bins)
    return flat.reshape(groups, bins).astype(np.uint64)


def samples(commit_times, commit_counts, faults, group_of, groups, since, max_clock):
    """The four sample families per group: samples[g][family] = int64 array."""
    since = [0] * groups if since is None else [int(v) for v in since]
    assert len(since) == groups and all(0 <= v <= max_clock for v in since)
    fam = [[[] for _ in range(4)] for _ in range(groups)]
    for g, c in _rows(commit_times, commit_counts, faults, group_of):
        t = np.unique(c)  # the commit instants, ascending
        gaps = np.diff(t)
        fam[g][GAPS].append(gaps)
        later = t[t >= since[g]]
        if len(later):
            fam[g][FIRST].append(later[:1] - since[g])
        if len(t):
            tail = max_clock - int(t[-1])
            longest = max(int(t[0]), tail, int(gaps.max()) if len(gaps) else 0)
        else:
            tail = longest = max_clock
        fam[g][TAIL].append(np.array([tail]))
        fam[g][LONGEST].append(np.array([longest]))
    return [[np.concatenate(f).astype(np.int64) if f else np.zeros(0, dtype=np.int64) for f in per_group] for per_group in fam]


def bin_stalls(fam, width, bins):
    """(hist [groups, bins] uint64 of the gaps, stats [groups, 16] uint64 = (samples, sum, min, max) of gaps, first, tail, longest) of
    the families `samples` returned."""
    groups = len(fam)
    hist = np.zeros((groups, bins), dtype=np.uint64)
    stats = np.zeros((groups, 16), dtype=np.uint64)
    for g in range(groups):
        gaps = fam[g][GAPS]
        assert (gaps >= 1).all()
        hist[g] = np.bincount(np.minimum(gaps // width, bins - 1), minlength=bins)
        for f in range(4):
            stats[g, 4 * f:4 * f + 4] = _stat(fam[g][f])
    return hist, stats


def stalls(commit_times, commit_counts, faults, group_of, groups, since, width, bins, max_clock):
    return bin_stalls(samples(commit_times, commit_counts, faults, group_of, groups, since, max_clock), width, bins)


# ---- the two-set scenario: a control set and a set with nodes {0, 1} cut off during [300, 600), 4 nodes, log-normal(10, 4), quirks = 3 (with
# the reference's own routing, quirks = 0, the partition never heals), seeds 1..32 per set, clock 1500 ----------------------------------------
SCENARIO = dict(nodes=4, mean=10.0, variance=4.0, quirks=3, partition=(2, 300, 600), seeds_per_set=32, max_clock=1500)
# 260 = the 300-tick window minus the 40 ticks in which commits already under way still land
SCENARIO_SETTLE, SCENARIO_STALL = 340, 260


def scenario_oracle(oracle, threads=8):
    """Commit times of the scenario derived from fresh oracle runs (commit_times_oracle): (commit times [64, 4, cap], commit counts,
    set_of, seeds)."""
    import commit_times_oracle as cto
    sc = SCENARIO
    per = sc["seeds_per_set"]
    set_of = np.repeat(np.arange(2), per).astype(np.uint32)
    seeds = np.tile(np.arange(1, per + 1), 2).astype(np.uint64)
    size, start, end = sc["partition"]
    kw = dict(num_nodes=sc["nodes"], mean=sc["mean"], variance=sc["variance"], quirks=sc["quirks"], math_mode=1)
    configs = [oracle.make_config(**kw), oracle.make_config(partition_size=size, partition_start=start, partition_end=end, **kw)]
    counts = np.zeros((len(seeds), sc["nodes"]), dtype=np.uint32)
    for k, cfg in enumerate(configs):
        counts[set_of == k] = oracle.run_batch(cfg, seeds[set_of == k], sc["max_clock"], threads=threads)["commit_counts"]
    cap = int(counts.max())
    ct = cto.param_set_commit_times(oracle, configs, set_of, seeds, sc["max_clock"], cap, threads)
    assert ((ct >= 0).sum(axis=2) == counts).all()
    return ct, counts, set_of, seeds


def check_scenario(series_, width, stats_since_end):
    """The scenario's own assertions, on a series of bin width `width` (a divisor of 20) and the stall statistics taken with since =
    (0, partition end): no commit of the partition set in [340, 600); every node of it commits again after 600; its every node's longest
    commit-free interval is at least 260 ticks; no node of the control set has one that long."""
    sc = SCENARIO
    assert SCENARIO_SETTLE % width == 0 and sc["partition"][2] % width == 0
    assert series_[1, SCENARIO_SETTLE // width:sc["partition"][2] // width].sum() == 0
    assert series_[0, SCENARIO_SETTLE // width:sc["partition"][2] // width].sum() > 0
    nodes = sc["seeds_per_set"] * sc["nodes"]
    assert stats_since_end[1, 4 * FIRST] == nodes  # every node has a first commit at or after the partition's end
    assert stats_since_end[1, 4 * LONGEST] == nodes and stats_since_end[0, 4 * LONGEST] == nodes
    assert stats_since_end[1, 4 * LONGEST + 2] >= SCENARIO_STALL  # longest.min, partition set
    assert stats_since_end[0, 4 * LONGEST + 3] < SCENARIO_STALL  # longest.max, control set
