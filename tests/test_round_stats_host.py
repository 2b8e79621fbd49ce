"""CPU-side checks of the round statistics: the arithmetic the device kernel shares with the host (csrc/lbft_round_timeline.h), compiled
into a g++ shim (tests/round_stats_host.cpp) that walks a trace the way the kernel does, equals the numpy reference written from the
definitions (tests/round_stats_reference.py) -- on drawn traces that hit every edge of the definitions, on tables written out by hand,
and on the oracle's own tables of a network with a partition, where nodes do jump rounds."""
import ctypes as C
import os

import numpy as np
import pytest

import round_stats_reference as ref
from support import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NONE = 0xffffffff  # an empty cell as the device stores it
CHUNKS = (1, 64, 32, 5)  # lanes side by side in the shim's node-major walk (the kernel: 64)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = build_shim(tmp_path_factory.mktemp("rtl_host"), "round_stats_host.cpp", "librtl_host.so", "-Wall", "-Werror")
    vp = C.c_void_p
    L.rtl_host.argtypes = [vp, vp, vp, vp] + [C.c_uint32] * 7 + [vp, vp, vp]
    L.rtl_host.restype = C.c_int
    L.gs_workgroups_host.argtypes = [C.c_uint64] * 4
    L.gs_workgroups_host.restype = C.c_uint64
    return L


def run_shim(L, first_time, max_round, faults, group_of, groups, width, bins, chunk):
    first_time = np.ascontiguousarray(first_time, dtype=np.uint32)
    m, n, rcap = first_time.shape
    max_round = np.ascontiguousarray(max_round, dtype=np.uint32)
    faults = np.ascontiguousarray(faults if faults is not None else np.zeros(m), dtype=np.uint32)
    group = None if group_of is None else np.ascontiguousarray(group_of, dtype=np.uint32)
    stay = np.zeros((groups, bins), dtype=np.uint64)
    skew = np.zeros((groups, bins), dtype=np.uint64)
    stats = np.zeros((groups, 16), dtype=np.uint64)
    rc = L.rtl_host(first_time.ctypes.data, max_round.ctypes.data, faults.ctypes.data, None if group is None else group.ctypes.data, m, n, rcap,
                    groups, width, bins, chunk, stay.ctypes.data, skew.ctypes.data, stats.ctypes.data)
    assert rc == 0
    return stay, skew, stats


def tables_of(first_time, max_round):
    """The tables the definitions speak of, from the trace as the device holds it: rows below the largest max_round (and the capacity)."""
    m, n, rcap = first_time.shape
    max_rounds = np.minimum(max_round.max(axis=1), rcap).astype(np.uint64)
    tables = np.full((m, max(int(max_rounds.max()), 1), n), ref.EMPTY, dtype=np.int64)
    for i in range(m):
        rows = int(max_rounds[i])
        t = first_time[i, :, :rows].T.astype(np.int64)
        tables[i, :rows] = np.where(t == NONE, ref.EMPTY, t)
    return tables, max_rounds


def compare(L, first_time, max_round, faults, group_of, groups, width, bins):
    tables, max_rounds = tables_of(first_time, max_round)
    want = ref.round_stats(tables, max_rounds, faults, group_of, groups, width, bins)
    for chunk in CHUNKS:
        got = run_shim(L, first_time, max_round, faults, group_of, groups, width, bins, chunk)
        for name, a, b in zip(("stay_hist", "skew_hist", "stats"), got, want):
            assert (a == b).all(), (name, chunk, width, bins, a, b)
    return want


def draw_instance(rng, n, rows, rcap, max_clock):
    """One instance's trace: the highest round reached is `rows`; every node reaches a round of its own, is recorded in a random subset
    of the rounds below it (jumps of 1 .. 10 rounds and more) and in that round itself -- the cell the device also stores at r = rows."""
    ft = np.full((n, rcap), NONE, dtype=np.uint32)
    mr = np.zeros(n, dtype=np.uint32)
    top = int(rng.integers(0, n))
    for j in range(n):
        mr[j] = rows if j == top else int(rng.integers(0, rows + 1))
        if mr[j] == 0:
            continue
        rounds = [r for r in range(1, int(mr[j])) if rng.random() < 0.7] + [int(mr[j])]
        times = np.sort(rng.integers(0, max_clock + 1, size=len(rounds)))
        if len(times) > 2 and rng.random() < 0.5:
            times[1] = times[0]  # a zero stay
        for r, t in zip(rounds, times):
            if r < rcap:
                ft[j, r] = t
    return ft, mr


def edge_instances(rcap):
    """Hand-made traces of 4 nodes, each with what its table must give written next to it."""
    out = []
    # R = 0: nobody left round 0 (the trace is untouched).  No sample of any family.
    out.append((np.full((4, rcap), NONE, dtype=np.uint32), np.zeros(4, dtype=np.uint32)))
    # R = 1: every node is in round 1, recorded at r = 1 = R: the table is the one empty row 0.  No sample.
    ft = np.full((4, rcap), NONE, dtype=np.uint32)
    ft[:, 1] = (5, 6, 7, 8)
    out.append((ft, np.full(4, 1, dtype=np.uint32)))
    # R = 2: rows 0 and 1; node 3 jumped from nothing to round 2 (its only cell is at r = R: no cell at all in the table).
    # skew of row 1 = 9 - 5, reach of row 1 = 3, no stay (one cell per node below R).
    ft = np.full((4, rcap), NONE, dtype=np.uint32)
    ft[:3, 1] = (5, 9, 7)
    ft[:, 2] = (20, 21, 22, 23)
    out.append((ft, np.full(4, 2, dtype=np.uint32)))
    # R = 14: node 0 walks 1, 2, 13 (a skip of 10) with a zero stay 30 -> 30; node 1's only cell is in row R - 1 = 13; node 2 has max_round
    # 0; node 3 skips 1, 2, ... 10 rounds in turn as far as the rows go: 1, 3, 6, 10.
    ft = np.full((4, rcap), NONE, dtype=np.uint32)
    ft[0, [1, 2, 13, 14]] = (30, 30, 400, 450)
    ft[1, [13, 14]] = (390, 460)
    ft[3, [1, 3, 6, 10]] = (31, 50, 90, 200)
    out.append((ft, np.array([14, 14, 0, 10], dtype=np.uint32)))
    return out


def test_tables_by_hand(shim):
    rcap = 20
    ft, mr = (np.stack(a) for a in zip(*edge_instances(rcap)))
    for chunk in CHUNKS:
        stay, skew, stats = run_shim(shim, ft[:3], mr[:3], None, None, 1, 3, 4, chunk)
        assert stats[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, 4, 4, 4, 1, 3, 3, 3] and not stay.any() and skew.tolist() == [[0, 1, 0, 0]]
        stay, skew, stats = run_shim(shim, ft[3:], mr[3:], None, None, 1, 100, 3, chunk)
        # stays: node 0: 0, 370; node 3: 19, 40, 110.  skipped: 0, 10; 1, 2, 3.  skew: rows 1 (31 - 30) and 13 (400 - 390).
        # reach: rows 1 .. 13 hold 2, 1, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 2 cells.
        assert stats[0].tolist() == [5, 539, 0, 370, 5, 16, 0, 10, 2, 11, 1, 10, 13, 8, 0, 2], stats
        assert stay.tolist() == [[3, 1, 1]] and skew.tolist() == [[2, 0, 0]]  # 370 clamps into the last bin
    want = ref.round_stats(*tables_of(ft, mr), None, None, 1, 100, 3)
    got = run_shim(shim, ft, mr, None, None, 1, 100, 3, 64)
    assert all((a == b).all() for a, b in zip(got, want))


def test_shim_equals_the_numpy_reference_on_drawn_traces(shim):
    rng = np.random.default_rng(20261017)
    n, rcap, groups, max_clock = 5, 70, 3, 3000
    row_counts = [0, 1, 2, 31, 32, 33, 63, 64, 65, 70, 70, 17, 40, 64, 65, 33]  # the chunk seams; rows = rcap: no cell at r = R is stored
    drawn = [draw_instance(rng, n, rows, rcap, max_clock) for rows in row_counts]
    edges = [(np.vstack([ft, np.full((1, 20), NONE, dtype=np.uint32)]), np.append(mr, 0).astype(np.uint32)) for ft, mr in edge_instances(20)]
    edges = [(np.pad(ft, ((0, 0), (0, rcap - 20)), constant_values=NONE), mr) for ft, mr in edges]
    ladder = np.full((n, rcap), NONE, dtype=np.uint32)  # node 0 skips 1, 2, ... 10 rounds in turn; node 1 walks every round
    ladder_rounds = np.cumsum(np.arange(1, 12))  # 1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 66
    ladder[0, ladder_rounds] = 40 * np.arange(11)
    ladder[1, 1:68] = 10 * np.arange(67)
    drawn.append((ladder, np.array([66, 67, 0, 0, 0], dtype=np.uint32)))
    ft = np.stack([a for a, _ in drawn + edges])
    mr = np.stack([b for _, b in drawn + edges])
    m = len(ft)
    # what the draw is meant to contain
    tables, max_rounds = tables_of(ft, mr)
    fam = ref.samples(tables, max_rounds, None, None, 1)[0]
    assert set(range(11)) <= set(fam[ref.SKIPPED].tolist()) and (fam[ref.STAY] == 0).any()
    assert (fam[ref.REACH] == 0).any() and fam[ref.REACH].max() == n
    stored_at_top = [i for i in range(m) if max_rounds[i] < rcap and (ft[i, :, int(max_rounds[i])] != NONE).any()]
    assert len(stored_at_top) >= 10  # cells at r = R that must be ignored (checked below)
    faults = np.zeros(m, dtype=np.uint32)
    faults[[4, 9]] = (1 << 11, 8)  # faulted instances are skipped, whatever their rows hold
    group_of = rng.integers(0, groups, size=m).astype(np.uint32)
    group_of[:3] = (0, 1, 2)
    top = int(max(fam[ref.STAY].max(), fam[ref.SKEW].max()))
    binnings = [(1, top + 1), (1, 1), (7, 1), (top + 5, 3), (2 ** 32 - 1, 2), (3, 50), (7, 5), (1, ref.LDS_BINS), (1, ref.LDS_BINS + 1)]
    for width, bins in binnings:
        stay, skew, stats = compare(shim, ft, mr, faults, group_of, groups, width, bins)
        assert (stay.sum(axis=1) == stats[:, 0]).all() and (skew.sum(axis=1) == stats[:, 8]).all()
        assert (stats[:, 0] == stats[:, 4]).all()  # one skipped sample per stay sample
        if bins == 1 or width > top:
            assert (stay[:, 0] == stats[:, 0]).all() and (skew[:, 0] == stats[:, 8]).all()
        if (width, bins) == (7, 5):
            assert stay[:, -1].sum() > 0 and skew[:, -1].sum() > 0 and top >= 7 * 5  # the last bin also counts everything above it
    compare(shim, ft, mr, None, None, 1, 5, 64)  # the plain-batch form: one group, no group array
    # the cell at r = R is ignored: the same trace with those cells emptied gives the same arrays
    cleared = ft.copy()
    for i in stored_at_top:
        cleared[i, :, int(max_rounds[i])] = NONE
    assert all((a == b).all() for a, b in zip(run_shim(shim, ft, mr, faults, group_of, groups, 3, 50, 64),
                                              run_shim(shim, cleared, mr, faults, group_of, groups, 3, 50, 64)))


def test_grid_rule_equals_the_two_launchers_formulas(shim):
    """gs_workgroups (lbft_group_stats.h), called the way lbft_ct_launch_timeline and lbft_rs_launch_rounds call it, gives the workgroups
    per group that each launcher used to compute for itself (written out below): about 1024 workgroups in all, at least one more than
    the largest group's samples >> 31 (no u32 LDS bin can wrap), at most one per step of a workgroup's stride."""
    target, tl_rows, rs_waves = 1024, 8, 4  # LBFT_TL_WORKGROUPS = LBFT_RS_WORKGROUPS, LBFT_TL_ROWS, LBFT_RS_WAVES
    csrc = os.path.join(ROOT, "librabft_simulator_amd", "csrc")
    ct_src, rs_src = (open(os.path.join(csrc, f)).read() for f in ("lbft_commit_times.hip", "lbft_round_stats.hip"))
    assert "#define LBFT_TL_WORKGROUPS 1024u" in ct_src and "#define LBFT_TL_BLOCK 256" in ct_src and "#define LBFT_TL_SEG 32" in ct_src
    assert "#define LBFT_RS_WORKGROUPS 1024u" in rs_src and "#define LBFT_RS_BLOCK 256" in rs_src

    def timeline_was(n_groups, max_group, n, lcap):
        rows = max_group * n
        steps = (rows + tl_rows - 1) // tl_rows
        gx = target // n_groups if target // n_groups else 1
        least = (rows * lcap >> 31) + 1
        gx = max(gx, least)
        return min(gx, steps)

    def rounds_was(n_groups, max_group, n, rcap):
        steps = (max_group + rs_waves - 1) // rs_waves
        gx = target // n_groups if target // n_groups else 1
        least = (max_group * n * rcap >> 31) + 1
        gx = max(gx, least)
        return min(gx, steps)

    table = [  # (n_groups, max_group, n, lcap or rcap)
        (1, 65536, 4, 64),           # one group: the target binds (1024)
        (256, 1024, 4, 64),          # 256 groups: 4 workgroups each
        (256, 1, 4, 64), (1, 1, 1, 1), (7, 1, 32, 4096),  # a largest group of one instance: one step
        (1, 3, 4, 16), (1, 37, 3, 100), (64, 9, 2, 8),    # fewer steps than the target: the cap binds
        (256, 1 << 20, 32, 4096),    # 2^37 samples: the floor of 65 binds over 1024 / 256 = 4
        (1, 1 << 26, 32, 65534),     # ... and over the target itself (65 535 > 1024)
        (1000, 1 << 22, 16, 2048),   # 1024 / 1000 = 1, floor 65
        (2048, 5000, 4, 64),         # more groups than the target: 1
    ]
    seen = set()
    for n_groups, max_group, n, cap in table:
        rows = max_group * n
        got_tl = shim.gs_workgroups_host(target, n_groups, (rows + tl_rows - 1) // tl_rows, rows * cap)
        got_rs = shim.gs_workgroups_host(target, n_groups, (max_group + rs_waves - 1) // rs_waves, max_group * n * cap)
        assert got_tl == timeline_was(n_groups, max_group, n, cap), (n_groups, max_group, n, cap, got_tl)
        assert got_rs == rounds_was(n_groups, max_group, n, cap), (n_groups, max_group, n, cap, got_rs)
        for gx, steps in ((got_tl, (rows + tl_rows - 1) // tl_rows), (got_rs, (max_group + rs_waves - 1) // rs_waves)):
            floor = (rows * cap >> 31) + 1
            seen.add("steps" if gx == steps else "floor" if gx == floor and floor > max(target // n_groups, 1) else "target")
    assert seen == {"steps", "floor", "target"}, seen


def test_oracle_tables_of_a_partitioned_network(shim, oracle):
    """4 nodes, quirks = 3, node 0 cut off during [300, 600), clock 1000, seeds 1 .. 16: the oracle's DataWriter tables show node 0
    jumping rounds after the partition; the shim on the trace rebuilt from those tables equals the reference on the tables."""
    cfg = oracle.make_config(num_nodes=4, quirks=3, partition_size=1, partition_start=300, partition_end=600, math_mode=1)
    tables, max_rounds, _ = ref.oracle_tables(oracle, cfg, range(1, 17), 1000)
    fam = ref.samples(tables, max_rounds, None, None, 1)[0]
    assert (fam[ref.SKIPPED] > 0).any() and (fam[ref.REACH] < 4).any() and (fam[ref.STAY] == 0).any()
    rcap = tables.shape[1] + 3
    ft = np.full((len(tables), 4, rcap), NONE, dtype=np.uint32)
    ft[:, :, :tables.shape[1]] = np.where(tables == ref.EMPTY, NONE, tables).transpose(0, 2, 1).astype(np.uint32)
    mr = np.repeat(max_rounds[:, None], 4, axis=1).astype(np.uint32)
    stay, skew, stats = compare(shim, ft, mr, None, None, 1, 1, 1001)
    assert stats[0, 0] == len(fam[ref.STAY]) and stats[0, 7] == fam[ref.SKIPPED].max()
