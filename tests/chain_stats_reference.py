"""TEST INFRASTRUCTURE: numpy reference of the chain statistics (include/lbft.h: lbft_batch_chain_stats), written from the definitions,
instance by instance, with none of the library's code.

Inputs: the committed histories as (proposer, index, time) records [instance, node, k], the commit counts [instance, node], the startup
times [instance, node], the fault words, the group of every instance and the binning.  nc_j = min(commit count, log capacity); the chain
is the history of the lowest-numbered node with the largest nc_j; an entry's global proposal time is startup[proposer] + time.
Instances with a non-zero fault word are skipped.

Entries are compared as (proposer, index, time) tuples, where the device compares block ids.  That is the same comparison: two different
blocks of an instance never share a tuple, because every block a node proposes takes a fresh command index -- propose_block
(csrc/lbft_core.h) reads NF_NEXT_CMD and increments it for every block, so the two twin blocks of an equivocating leader come from two
fetches and differ in `index` -- and equal ids are one record of the pool the nodes share, hence equal tuples."""
import numpy as np

INTERVAL, LENGTH, LAG, TENURE, DIFFERING, INVERSIONS = range(6)
FAMILIES = 6
CHAIN_STATS = 24  # LBFT_CHAIN_STATS
LDS_BINS = 4096  # LBFT_CS_LDS_BINS: the device bins wider histograms in passes of this many bins
COMMIT_DTYPE = np.dtype([("proposer", "<u8"), ("index", "<u8"), ("time", "<i8")])


def samples(histories, commit_counts, startup_times, faults, set_of, groups, log_capacity=None):
    """(fam, authors): fam[g][family] = int64 array of the family's samples of group g, authors[g, a] = chain entries authored by a."""
    histories = np.asarray(histories)
    counts = np.asarray(commit_counts).astype(np.int64)
    startup = np.asarray(startup_times).astype(np.int64)
    m, n, cap = histories.shape
    faults = np.zeros(m, dtype=np.uint32) if faults is None else np.asarray(faults)
    set_of = np.zeros(m, dtype=np.int64) if set_of is None else np.asarray(set_of).astype(np.int64)
    fam = [[[] for _ in range(FAMILIES)] for _ in range(groups)]
    authors = np.zeros((groups, n), dtype=np.uint64)
    for i in range(m):
        if faults[i] != 0:
            continue
        g = int(set_of[i])
        nc = counts[i] if log_capacity is None else np.minimum(counts[i], int(log_capacity))
        assert nc.max() <= cap, (i, nc, cap)
        ref = int(np.argmax(nc))  # (the first of the largest: the lowest-numbered node)
        length = int(nc[ref])
        chain = histories[i, ref, :length]
        a = chain["proposer"].astype(np.int64)
        t = startup[i, a] + chain["time"].astype(np.int64)
        assert ((t >= 0) & (t < 2 ** 31)).all()
        d = np.diff(t)
        fam[g][INTERVAL].append(np.maximum(d, 0))
        fam[g][LENGTH].append([length])
        fam[g][LAG].append(length - nc)
        if length:
            starts = np.concatenate([[0], np.nonzero(a[1:] != a[:-1])[0] + 1, [length]])
            fam[g][TENURE].append(np.diff(starts))
        fam[g][DIFFERING].append([sum(int((histories[i, j, :int(nc[j])] != chain[:int(nc[j])]).sum()) for j in range(n))])
        fam[g][INVERSIONS].append([int((d < 0).sum())])
        authors[g] += np.bincount(a, minlength=n).astype(np.uint64)
    fam = [[np.concatenate(f).astype(np.int64) if f else np.zeros(0, dtype=np.int64) for f in per_group] for per_group in fam]
    return fam, authors


def _stat(s):
    return (len(s), int(s.sum()), int(s.min()), int(s.max())) if len(s) else (0, 0, 0, 0)


def bin_chain(fam, authors, width, bins):
    """(interval_hist, author_blocks, stats) as the C ABI returns them, from the sample families."""
    groups = len(fam)
    hist = np.zeros((groups, bins), dtype=np.uint64)
    stats = np.zeros((groups, CHAIN_STATS), dtype=np.uint64)
    for g in range(groups):
        assert all((s >= 0).all() for s in fam[g])
        hist[g] = np.bincount(np.minimum(fam[g][INTERVAL] // width, bins - 1), minlength=bins)
        for f in range(FAMILIES):
            stats[g, 4 * f:4 * f + 4] = _stat(fam[g][f])
    return hist, authors.copy(), stats


def chain_stats(histories, commit_counts, startup_times, faults, set_of, groups, width, bins, log_capacity=None):
    return bin_chain(*samples(histories, commit_counts, startup_times, faults, set_of, groups, log_capacity), width, bins)


def oracle_runs(oracle, cfg, seeds, max_clock):
    """(histories [instance, node, k], commit counts, startup times) of the oracle, one run of `cfg` per seed."""
    runs = []
    for seed in seeds:
        sim = oracle.OracleSim(cfg, int(seed)).run_until(int(max_clock))
        runs.append(([sim.committed_history(j) for j in range(cfg.num_nodes)], sim.startup_times()))
        sim.close()
    return stack([h for h, _ in runs], [s for _, s in runs])


def oracle_batch(oracle, cfg, seeds, max_clock, threads=8):
    """The same through the oracle's batch call on `threads` threads, for batches of many instances.  (The startup times are drawn when a
    simulator is created and never change: they are read from simulators that are not run.)"""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    cap = int(max_clock) // 8 + 8  # (a guess that holds for delays of mean 10; the counts say whether it held)
    out = oracle.run_batch(cfg, seeds, int(max_clock), threads=threads, history_cap=cap)
    counts = out["commit_counts"]
    if int(counts.max()) > cap:
        out = oracle.run_batch(cfg, seeds, int(max_clock), threads=threads, history_cap=int(counts.max()))
        assert (out["commit_counts"] == counts).all()
    startup = np.array([oracle.OracleSim(cfg, int(seed)).startup_times() for seed in seeds], dtype=np.int64)
    return out["histories"][:, :, :max(int(counts.max()), 1)].copy(), counts, startup


def stack(histories_of, startup_of):
    """Per instance a list of per-node record arrays and a list of startup times, as (histories, commit counts, startup times)."""
    m, n = len(histories_of), len(histories_of[0]) if histories_of else 0
    counts = np.array([[len(h) for h in inst] for inst in histories_of], dtype=np.uint32).reshape(m, n)
    histories = np.zeros((m, n, max(int(counts.max()) if counts.size else 0, 1)), dtype=COMMIT_DTYPE)
    for i, inst in enumerate(histories_of):
        for j, h in enumerate(inst):
            histories[i, j, :len(h)] = h
    return histories, counts, np.array(startup_of, dtype=np.int64).reshape(m, n)


def concat(parts):
    """Runs of several configurations, one batch: histories padded to the longest."""
    cap = max(p[0].shape[2] for p in parts)
    hist = np.zeros((sum(len(p[0]) for p in parts), parts[0][0].shape[1], cap), dtype=COMMIT_DTYPE)
    at = 0
    for p in parts:
        hist[at:at + len(p[0]), :, :p[0].shape[2]] = p[0]
        at += len(p[0])
    return hist, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
