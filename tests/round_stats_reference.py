"""TEST INFRASTRUCTURE: numpy reference of the round statistics (include/lbft.h: lbft_batch_round_stats), written from the definitions,
table by table, with none of the library's code.

An instance's table T[r][j] has the rows r in [0, R), R = max_rounds[instance] (the largest max_round of its nodes); a cell is a
GlobalTime or EMPTY.  Whatever `tables` holds at or past row R is not part of the table.  Instances with a non-zero fault word are
skipped.  Families: stay / skipped over the consecutive non-empty cells of a node's column, skew / reach over the cells of a row."""
import numpy as np

STAY, SKIPPED, SKEW, REACH = range(4)
EMPTY = np.iinfo(np.int64).min
LDS_BINS = 4096  # LBFT_RS_LDS_BINS: the device bins wider histograms in passes of this many bins


def samples(tables, max_rounds, faults, set_of, groups):
    """The four sample families per group: samples[g][family] = int64 array."""
    tables = np.asarray(tables, dtype=np.int64)
    m = tables.shape[0]
    faults = np.zeros(m, dtype=np.uint32) if faults is None else np.asarray(faults)
    set_of = np.zeros(m, dtype=np.int64) if set_of is None else np.asarray(set_of).astype(np.int64)
    fam = [[[] for _ in range(4)] for _ in range(groups)]
    for i in range(m):
        if faults[i] != 0:
            continue
        g = int(set_of[i])
        rows = int(max_rounds[i])
        assert rows <= tables.shape[1], (i, rows, tables.shape)
        t = tables[i, :rows]  # [round, node]
        for j in range(t.shape[1]):
            r = np.nonzero(t[:, j] != EMPTY)[0]
            fam[g][STAY].append(np.diff(t[r, j]))
            fam[g][SKIPPED].append(np.diff(r) - 1)
        for r in range(rows):
            cells = t[r][t[r] != EMPTY]
            if len(cells) >= 2:
                fam[g][SKEW].append([cells.max() - cells.min()])
            if r >= 1:
                fam[g][REACH].append([len(cells)])
    return [[np.concatenate(f).astype(np.int64) if f else np.zeros(0, dtype=np.int64) for f in per_group] for per_group in fam]


def _stat(s):
    return (len(s), int(s.sum()), int(s.min()), int(s.max())) if len(s) else (0, 0, 0, 0)


def bin_rounds(fam, width, bins):
    """(stay_hist, skew_hist, stats) as the C ABI returns them, from the sample families."""
    groups = len(fam)
    stay = np.zeros((groups, bins), dtype=np.uint64)
    skew = np.zeros((groups, bins), dtype=np.uint64)
    stats = np.zeros((groups, 16), dtype=np.uint64)
    for g in range(groups):
        assert all((s >= 0).all() for s in fam[g])
        stay[g] = np.bincount(np.minimum(fam[g][STAY] // width, bins - 1), minlength=bins)
        skew[g] = np.bincount(np.minimum(fam[g][SKEW] // width, bins - 1), minlength=bins)
        for f in range(4):
            stats[g, 4 * f:4 * f + 4] = _stat(fam[g][f])
    return stay, skew, stats


def round_stats(tables, max_rounds, faults, set_of, groups, width, bins):
    return bin_rounds(samples(tables, max_rounds, faults, set_of, groups), width, bins)


def oracle_tables(oracle, cfg, seeds, max_clock):
    """(tables [instance, round, node], max_rounds, messages) of the oracle's DataWriter for one configuration, one run per seed."""
    runs = [oracle.OracleSim(cfg, int(seed)).enable_data_writer().run_until(max_clock).round_switches() for seed in seeds]
    return stack([rows for rows, _ in runs], cfg.num_nodes) + (np.array([msgs for _, msgs in runs], dtype=np.uint64),)


def stack(rows_of, n):
    """Lists of rows (rows[round][node] = time or None), one per instance, as (tables, max_rounds)."""
    max_rounds = np.array([len(rows) for rows in rows_of], dtype=np.uint64)
    tables = np.full((len(rows_of), max(int(max_rounds.max()) if len(rows_of) else 0, 1), n), EMPTY, dtype=np.int64)
    for i, rows in enumerate(rows_of):
        for r, row in enumerate(rows):
            tables[i, r] = [EMPTY if v is None else v for v in row]
    return tables, max_rounds
