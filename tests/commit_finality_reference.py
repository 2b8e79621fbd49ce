"""TEST INFRASTRUCTURE: numpy reference of commit finality (include/lbft.h: lbft_batch_commit_finality), written from the definitions,
entry by entry, with none of the library's code.

Inputs: the commit times [instance, node, k] (-1 = not recorded), the commit counts [instance, node], the committed histories as records
with `proposer` and `time` [instance, node, k], the startup times [instance, node], the fault words, the voting rights with their
rotation and commands_per_epoch, the group of every instance.  nc_j = min(commit count, log capacity); the chain is the history of the
lowest-numbered node with the largest nc_j; entry k's proposal time is startup[proposer] + time; node j is a committer of k if k < nc_j
and its commit time is recorded; its voting right at k is rights[(j + (k // commands_per_epoch) * rotation) % n].  A threshold's time is
found by sorting the committers' distinct times and adding up the rights of the committers at each: the smallest time at which the sum
reaches the threshold.  Instances with a non-zero fault word are skipped."""
import numpy as np

FIRST, VALID, QUORUM, ALL, SPREAD, OPEN = range(6)
FAMILIES = 6
FINALITY_STATS = 24  # LBFT_FINALITY_STATS
LDS_BINS = 4096  # LBFT_FN_LDS_BINS: the device bins wider histograms in passes of this many bins
NAMES = ("first", "valid", "quorum", "all", "spread", "open")


def thresholds(rights):
    """(total, quorum, valid) of a rights table."""
    total = int(sum(int(w) for w in rights))
    quorum = 2 * total // 3 + 1
    return total, quorum, total - quorum + 1


def threshold_time(times, weights, need):
    """The smallest t such that the entries of `times` that are <= t carry `weights` summing to at least `need`; None if all do not."""
    for t in sorted(set(times)):
        if sum(w for c, w in zip(times, weights) if c <= t) >= need:
            return t
    return None


def entry_times(times, weights, n, quorum, valid):
    """(first, valid, quorum, all, first committer) of one entry from its committers' (node, time) pairs, None where undefined."""
    if not times:
        return None, None, None, None, None
    nodes = [j for j, _ in times]
    c = [t for _, t in times]
    first = min(c)
    return (first, threshold_time(c, weights, valid), threshold_time(c, weights, quorum), max(c) if len(c) == n else None,
            min(j for j, t in zip(nodes, c) if t == first))


def samples(commit_times, commit_counts, histories, startup_times, faults, rights, rotation, commands_per_epoch, set_of, groups,
            log_capacity=None):
    """(fam, first_committer): fam[g][family] = int64 array of the family's samples of group g, first_committer[g, j] = entries node j
    committed first."""
    ct = np.asarray(commit_times).astype(np.int64)
    counts = np.asarray(commit_counts).astype(np.int64)
    startup = np.asarray(startup_times).astype(np.int64)
    m, n, cap = ct.shape
    rights = [1] * n if rights is None else [int(w) for w in rights]
    assert len(rights) == n and commands_per_epoch >= 1
    _, quorum, valid = thresholds(rights)
    faults = np.zeros(m, dtype=np.uint32) if faults is None else np.asarray(faults)
    set_of = np.zeros(m, dtype=np.int64) if set_of is None else np.asarray(set_of).astype(np.int64)
    fam = [[[] for _ in range(FAMILIES)] for _ in range(groups)]
    first_committer = np.zeros((groups, n), dtype=np.uint64)
    for i in range(m):
        if faults[i] != 0:
            continue
        g = int(set_of[i])
        nc = counts[i] if log_capacity is None else np.minimum(counts[i], int(log_capacity))
        ref = int(np.argmax(nc))  # (the first of the largest: the lowest-numbered node)
        length = int(nc[ref])
        assert length <= cap and length <= histories.shape[2], (i, length, cap)
        open_ = 0
        for k in range(length):
            e = histories[i, ref, k]
            origin = int(startup[i, int(e["proposer"])]) + int(e["time"])
            shift = (k // int(commands_per_epoch)) * int(rotation)
            times = [(j, int(ct[i, j, k])) for j in range(n) if k < nc[j] and ct[i, j, k] >= 0]
            weights = [rights[(j + shift) % n] for j, _ in times]
            first, t_valid, t_quorum, t_all, who = entry_times(times, weights, n, quorum, valid)
            if first is None:
                continue
            fam[g][FIRST].append(first - origin)
            first_committer[g, who] += 1
            if t_valid is not None:
                fam[g][VALID].append(t_valid - origin)
            if t_quorum is not None:
                fam[g][QUORUM].append(t_quorum - origin)
            else:
                open_ += 1
            if t_all is not None:
                fam[g][ALL].append(t_all - origin)
                fam[g][SPREAD].append(t_all - first)
        fam[g][OPEN].append(open_)
    return [[np.array(f, dtype=np.int64) for f in per_group] for per_group in fam], first_committer


def _stat(s):
    return (len(s), int(s.sum()), int(s.min()), int(s.max())) if len(s) else (0, 0, 0, 0)


def bin_finality(fam, first_committer, width, bins, max_clock=None):
    """(finality_hist, spread_hist, first_committer, stats) as the C ABI returns them, from the sample families.  Every sample is
    non-negative (and at most max_clock, where given): a commit before its entry's proposal would be a finding."""
    groups = len(fam)
    fin = np.zeros((groups, bins), dtype=np.uint64)
    spread = np.zeros((groups, bins), dtype=np.uint64)
    stats = np.zeros((groups, FINALITY_STATS), dtype=np.uint64)
    for g in range(groups):
        assert all((s >= 0).all() for s in fam[g]), [int(s.min()) for s in fam[g] if len(s)]
        assert max_clock is None or all((s <= max_clock).all() for s in fam[g][:OPEN])
        fin[g] = np.bincount(np.minimum(fam[g][QUORUM] // width, bins - 1), minlength=bins)
        spread[g] = np.bincount(np.minimum(fam[g][SPREAD] // width, bins - 1), minlength=bins)
        for f in range(FAMILIES):
            stats[g, 4 * f:4 * f + 4] = _stat(fam[g][f])
    return fin, spread, first_committer.copy(), stats


def finality(commit_times, commit_counts, histories, startup_times, faults, rights, rotation, commands_per_epoch, set_of, groups, width, bins,
             log_capacity=None):
    return bin_finality(*samples(commit_times, commit_counts, histories, startup_times, faults, rights, rotation, commands_per_epoch, set_of,
                                 groups, log_capacity), width, bins)


def of_result(res, rights=None, rotation=0, commands_per_epoch=30000, set_of=None, groups=1, log_capacity=None):
    """The sample families of a BatchResult, from its own read-backs: commit times, histories, startup times, fault words, counts."""
    ct = res.commit_times()
    return samples(ct, res.commit_counts, res.committed_histories(ct.shape[2]), res.startup_times, res.faults, rights, rotation,
                   commands_per_epoch, set_of, groups, log_capacity)
