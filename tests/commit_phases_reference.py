"""TEST INFRASTRUCTURE: numpy reference of the commit phases (include/lbft.h: lbft_batch_commit_phases), written from the definitions,
sample by sample, with none of the library's code.

Inputs as the finality reference's: commit times [instance, node, k] (-1 = not recorded), commit counts [instance, node], committed
histories as records with `proposer` and `time` [instance, node, k], startup times [instance, node], fault words, the voting rights with
their rotation and commands_per_epoch, the group of every instance -- and the edges [group][phases - 1].  The phase of a time t is the
number of the group's edges at or below t.  A latency sample is one recorded entry (k < nc_j, commit time >= 0) of one node: commit time
- (startup[proposer] + time) of the record in the node's OWN history, in the phase of that proposal time.  The finality samples of
entry k of the chain (the history of the lowest-numbered node with the largest nc_j) are first / valid / quorum / all after the
chain record's proposal time and spread = all - first, all in the phase of that proposal time; the times themselves are
commit_finality_reference.entry_times (sorted distinct times, rights added up).  Instances with a non-zero fault word are skipped."""
import numpy as np

import commit_finality_reference as fin_ref

LATENCY, FIRST, VALID, QUORUM, ALL, SPREAD = range(6)
FAMILIES = 6
PHASE_STATS = 24  # LBFT_PHASE_STATS
MAX_PHASES = 8  # LBFT_MAX_PHASES
LDS_BINS = 4096  # LBFT_PH_LDS_BINS: the device bins the phases x bins virtual histograms in passes of this many bins
NAMES = ("latency", "first", "valid", "quorum", "all", "spread")
SAMPLES, SUM, MIN, MAX = range(4)


def phase_of(edges, t):
    """#{q : e_q <= t}."""
    return sum(1 for e in edges if int(e) <= int(t))


def edges_per_group(edges, groups):
    """[groups, phases - 1] int64 from one list for every group or one list per group."""
    e = np.asarray(edges, dtype=np.int64)
    if e.ndim == 1:
        e = np.tile(e, (groups, 1))
    assert e.shape[0] == groups and e.shape[1] < MAX_PHASES and (np.diff(e, axis=1) >= 0).all() and (e >= 0).all()
    return e


def samples(commit_times, commit_counts, histories, startup_times, faults, rights, rotation, commands_per_epoch, set_of, groups, edges,
            log_capacity=None):
    """fam[g][p][family] = int64 array of the family's samples of phase p of group g."""
    ct = np.asarray(commit_times).astype(np.int64)
    counts = np.asarray(commit_counts).astype(np.int64)
    startup = np.asarray(startup_times).astype(np.int64)
    m, n, cap = ct.shape
    edges = edges_per_group(edges, groups)
    phases = edges.shape[1] + 1
    rights = [1] * n if rights is None else [int(w) for w in rights]
    assert len(rights) == n and commands_per_epoch >= 1
    _, quorum, valid = fin_ref.thresholds(rights)
    faults = np.zeros(m, dtype=np.uint32) if faults is None else np.asarray(faults)
    set_of = np.zeros(m, dtype=np.int64) if set_of is None else np.asarray(set_of).astype(np.int64)
    fam = [[[[] for _ in range(FAMILIES)] for _ in range(phases)] for _ in range(groups)]
    for i in range(m):
        if faults[i] != 0:
            continue
        g = int(set_of[i])
        nc = counts[i] if log_capacity is None else np.minimum(counts[i], int(log_capacity))
        for j in range(n):  # the latency: every node's own history
            for k in range(int(nc[j])):
                if ct[i, j, k] < 0:
                    continue
                e = histories[i, j, k]
                origin = int(startup[i, int(e["proposer"])]) + int(e["time"])
                fam[g][phase_of(edges[g], origin)][LATENCY].append(int(ct[i, j, k]) - origin)
        ref = int(np.argmax(nc))  # (the first of the largest: the lowest-numbered node)
        for k in range(int(nc[ref])):  # the finality: the chain
            e = histories[i, ref, k]
            origin = int(startup[i, int(e["proposer"])]) + int(e["time"])
            shift = (k // int(commands_per_epoch)) * int(rotation)
            times = [(j, int(ct[i, j, k])) for j in range(n) if k < nc[j] and ct[i, j, k] >= 0]
            weights = [rights[(j + shift) % n] for j, _ in times]
            first, t_valid, t_quorum, t_all, _ = fin_ref.entry_times(times, weights, n, quorum, valid)
            if first is None:
                continue
            mine = fam[g][phase_of(edges[g], origin)]
            mine[FIRST].append(first - origin)
            if t_valid is not None:
                mine[VALID].append(t_valid - origin)
            if t_quorum is not None:
                mine[QUORUM].append(t_quorum - origin)
            if t_all is not None:
                mine[ALL].append(t_all - origin)
                mine[SPREAD].append(t_all - first)
    return [[[np.array(f, dtype=np.int64) for f in per_phase] for per_phase in per_group] for per_group in fam]


def bin_phases(fam, width, bins, max_clock=None):
    """(latency_hist [g, p, bins], finality_hist [g, p, bins], stats [g, p, 6, 4]) as the C ABI returns them, from the sample families.
    Every sample is non-negative (and at most max_clock, where given): a commit before its entry's proposal would be a finding."""
    groups, phases = len(fam), len(fam[0])
    lat = np.zeros((groups, phases, bins), dtype=np.uint64)
    fin = np.zeros((groups, phases, bins), dtype=np.uint64)
    stats = np.zeros((groups, phases, FAMILIES, 4), dtype=np.uint64)
    for g in range(groups):
        for p in range(phases):
            assert all((s >= 0).all() for s in fam[g][p]) and (max_clock is None or all((s <= max_clock).all() for s in fam[g][p]))
            lat[g, p] = np.bincount(np.minimum(fam[g][p][LATENCY] // width, bins - 1), minlength=bins)
            fin[g, p] = np.bincount(np.minimum(fam[g][p][QUORUM] // width, bins - 1), minlength=bins)
            for f in range(FAMILIES):
                s = fam[g][p][f]
                if len(s):
                    stats[g, p, f] = (len(s), int(s.sum()), int(s.min()), int(s.max()))
    return lat, fin, stats


def of_result(res, edges, rights=None, rotation=0, commands_per_epoch=30000, set_of=None, groups=1, log_capacity=None):
    """The sample families of a BatchResult, from its own read-backs: commit times, histories, startup times, fault words, counts."""
    ct = res.commit_times()
    return samples(ct, res.commit_counts, res.committed_histories(ct.shape[2]), res.startup_times, res.faults, rights, rotation,
                   commands_per_epoch, set_of, groups, edges, log_capacity)


def chain_phases(res, edges, set_of=None, groups=1, log_capacity=None):
    """Per instance of a BatchResult, the phases of its chain's entries in chain order (int64 arrays): what a test's precondition on
    the data looks at -- whether two neighbouring entries lie in different phases."""
    counts = np.asarray(res.commit_counts).astype(np.int64)
    startup = np.asarray(res.startup_times).astype(np.int64)
    edges = edges_per_group(edges, groups)
    nc = counts if log_capacity is None else np.minimum(counts, int(log_capacity))
    histories = res.committed_histories(max(int(nc.max()), 1))
    set_of = np.zeros(len(counts), dtype=np.int64) if set_of is None else np.asarray(set_of).astype(np.int64)
    out = []
    for i in range(len(counts)):
        ref = int(np.argmax(nc[i]))
        h = histories[i, ref, :int(nc[i, ref])]
        origin = startup[i, h["proposer"].astype(np.int64)] + h["time"].astype(np.int64)
        out.append(np.array([phase_of(edges[int(set_of[i])], t) for t in origin], dtype=np.int64))
    return out


def splits_a_chunk(phases, chunk=64):
    """Some entries k and k + 1 of one chunk of the chain lie in different phases."""
    k = np.nonzero(np.diff(phases) != 0)[0]
    return bool(len(k)) and bool((k % chunk != chunk - 1).any())


def pooled(lat, fin, stats):
    """What the phases of every group add up to: (latency_hist [g, bins], finality_hist [g, bins], stats [g, 6, 4]) -- bins, samples
    and sums add, the least minimum and the largest maximum are taken over the phases with samples."""
    out = np.zeros(stats.shape[:1] + stats.shape[2:], dtype=np.uint64)
    out[:, :, SAMPLES] = stats[:, :, :, SAMPLES].sum(axis=1)
    out[:, :, SUM] = stats[:, :, :, SUM].sum(axis=1)
    have = stats[:, :, :, SAMPLES] > 0
    out[:, :, MIN] = np.where(have.any(axis=1), np.where(have, stats[:, :, :, MIN], np.uint64(2 ** 63)).min(axis=1), 0)
    out[:, :, MAX] = np.where(have, stats[:, :, :, MAX], 0).max(axis=1)
    return lat.sum(axis=1), fin.sum(axis=1), out
