"""TEST INFRASTRUCTURE: numpy reference of the run load (lbft_batch_load_stats, lbft_batch_instance_load), written from the family
table of include/lbft.h: every instance gives one u32 sample to each of sixteen families; the statistics and the histogram take the
instances with a zero fault word, the census every instance."""
import numpy as np

FAMILIES = ("notifications", "requests", "responses", "timers", "messages", "scheduled", "draws", "folded", "updates", "queue", "chunks",
            "snapshots", "blocks", "log", "commits", "rounds")
F = {name: k for k, name in enumerate(FAMILIES)}
LOAD_STATS = 64
FAULT_BITS = 32
# the words of an instance the families read as they are, in the order the host shim takes them (LoadWord of csrc/lbft_load_stats.h)
WORDS = ("ev0", "ev1", "ev2", "ev3", "stamp", "draws", "nfold", "nupd", "maxq", "cal_bump", "maxsnap", "nblocks")
WORD_OF = {"notifications": "ev0", "requests": "ev1", "responses": "ev2", "timers": "ev3", "scheduled": "stamp", "draws": "draws",
           "folded": "nfold", "updates": "nupd", "queue": "maxq", "chunks": "cal_bump", "snapshots": "maxsnap", "blocks": "nblocks"}


def rows(words, commits, rounds, calendar):
    """words: [m, 12] uint32 in the order of WORDS; commits, rounds: [m, n] -> [m, 16] uint32."""
    words, commits, rounds = (np.asarray(a, dtype=np.uint32) for a in (words, commits, rounds))
    out = np.zeros((len(words), len(FAMILIES)), dtype=np.uint32)
    for name, word in WORD_OF.items():
        out[:, F[name]] = words[:, WORDS.index(word)]
    if not calendar:
        out[:, F["chunks"]] = 0
    out[:, F["messages"]] = (out[:, 0].astype(np.uint64) + out[:, 1] + out[:, 2]).astype(np.uint32)  # (a u32 add: modulo 2^32)
    out[:, F["log"]] = commits.max(axis=1)
    out[:, F["commits"]] = commits.min(axis=1)
    out[:, F["rounds"]] = rounds.min(axis=1)
    return out


def _groups(m, set_of, groups):
    return np.zeros(m, dtype=np.int64) if set_of is None else np.asarray(set_of, dtype=np.int64), groups


def census(faults, set_of=None, groups=1):
    faults = np.asarray(faults, dtype=np.uint32)
    group_of, groups = _groups(len(faults), set_of, groups)
    out = np.zeros((groups, FAULT_BITS), dtype=np.uint64)
    for k in range(FAULT_BITS):
        out[:, k] = np.bincount(group_of[(faults >> np.uint32(k)) & np.uint32(1) == 1], minlength=groups)
    return out


def stats(rows_, faults, set_of=None, groups=1):
    rows_, faults = np.asarray(rows_, dtype=np.uint32), np.asarray(faults)
    group_of, groups = _groups(len(rows_), set_of, groups)
    out = np.zeros((groups, LOAD_STATS), dtype=np.uint64)
    for g in range(groups):
        sel = rows_[(group_of == g) & (faults == 0)].astype(np.uint64)
        if len(sel):
            out[g] = np.stack([np.full(len(FAMILIES), len(sel), dtype=np.uint64), sel.sum(axis=0, dtype=np.uint64), sel.min(axis=0), sel.max(axis=0)],
                              axis=1).reshape(-1)
    return out


def hist(rows_, faults, family, bin_width, bins, set_of=None, groups=1):
    rows_, faults = np.asarray(rows_, dtype=np.uint32), np.asarray(faults)
    group_of, groups = _groups(len(rows_), set_of, groups)
    out = np.zeros((groups, bins), dtype=np.uint64)
    clean = faults == 0
    b = np.minimum(rows_[:, family].astype(np.uint64) // np.uint64(bin_width), np.uint64(bins - 1)).astype(np.int64)
    np.add.at(out, (group_of[clean], b[clean]), 1)
    return out


def default_bins(rows_, faults, family, bin_width=1):
    """BatchResult.load_stats' default: as many bins as the largest clean sample of the family needs."""
    clean = np.asarray(rows_)[np.asarray(faults) == 0, family]
    return (int(clean.max()) if len(clean) else 0) // bin_width + 1


def oracle_rows(oracle, cfg, seeds, max_clock):
    """One oracle simulator per seed -> ([m, 16] int64 rows with -1 where the oracle has no such counter, the families it has)."""
    n = cfg.num_nodes
    out = np.full((len(seeds), len(FAMILIES)), -1, dtype=np.int64)
    for i, seed in enumerate(seeds):
        sim = oracle.OracleSim(cfg, int(seed)).run_until(max_clock)
        c, commits, rounds = sim.counters(), sim.commit_counts(), sim.active_rounds()
        sim.close()
        assert len(commits) == len(rounds) == n
        out[i, 0:4] = c["events"]
        out[i, F["messages"]] = sum(c["events"][:3])
        out[i, F["scheduled"]], out[i, F["draws"]] = c["events_scheduled"], c["rng_draws"]
        out[i, F["log"]], out[i, F["commits"]], out[i, F["rounds"]] = max(commits), min(commits), min(rounds)
    return out, ORACLE_FAMILIES


ORACLE_FAMILIES = (0, 1, 2, 3, 4, 5, 6, 13, 14, 15)
