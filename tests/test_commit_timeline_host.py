"""CPU-side checks of the commit timelines: the arithmetic the device kernel shares with the host (csrc/lbft_commit_timeline.h), compiled
into a g++ shim (tests/commit_timeline_host.cpp) that walks rows the way the kernel does, equals the numpy reference written from the
definitions (tests/commit_timeline_reference.py) -- on drawn rows that hit every edge of the definitions, and on commit times derived
from the oracle for a control set and a set with a partition, where the reference alone already shows the stall and the recovery."""
import ctypes as C
import os

import numpy as np
import pytest

import commit_timeline_reference as ref
from support import build_shim

THREADS = min(os.cpu_count() or 8, 16)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = build_shim(tmp_path_factory.mktemp("ctl_host"), "commit_timeline_host.cpp", "libctl_host.so", "-Wall", "-Werror")
    vp = C.c_void_p
    L.ctl_host.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_int64, C.c_uint32, C.c_uint32, C.c_uint32,
                           vp, vp, vp]
    L.ctl_host.restype = C.c_int
    return L


def run_shim(L, ct, counts, faults, group_of, groups, since, max_clock, width, bins, seg):
    ct = np.ascontiguousarray(ct, dtype=np.int64)
    m, n, cap = ct.shape
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    faults = np.ascontiguousarray(faults if faults is not None else np.zeros(m), dtype=np.uint32)
    group_of = np.ascontiguousarray(group_of if group_of is not None else np.zeros(m), dtype=np.uint32)
    since_a = None if since is None else np.ascontiguousarray(since, dtype=np.int64)
    series = np.zeros((groups, bins), dtype=np.uint64)
    hist = np.zeros((groups, bins), dtype=np.uint64)
    stats = np.zeros((groups, 16), dtype=np.uint64)
    rc = L.ctl_host(ct.ctypes.data, counts.ctypes.data, faults.ctypes.data, group_of.ctypes.data, m, n, cap, groups,
                    None if since_a is None else since_a.ctypes.data, max_clock, width, bins, seg, series.ctypes.data, hist.ctypes.data,
                    stats.ctypes.data)
    assert rc == 0
    return series, hist, stats


def compare(L, ct, counts, faults, group_of, groups, since, max_clock, width, bins):
    want_series = ref.series(ct, counts, faults, group_of, groups, width, bins)
    want_hist, want_stats = ref.stalls(ct, counts, faults, group_of, groups, since, width, bins, max_clock)
    for seg in (1, 32, 5):
        series, hist, stats = run_shim(L, ct, counts, faults, group_of, groups, since, max_clock, width, bins, seg)
        assert (series == want_series).all(), (seg, width, bins)
        assert (hist == want_hist).all(), (seg, width, bins)
        assert (stats == want_stats).all(), (seg, width, bins, stats, want_stats)
    return want_series, want_hist, want_stats


def draw_rows(rng, m, n, cap, max_clock):
    """Commit times [m, n, cap] (-1 padded) and counts: rows of random length with repeated times, plus the fixed edge rows."""
    ct = np.full((m, n, cap), -1, dtype=np.int64)
    counts = np.zeros((m, n), dtype=np.uint32)
    for i in range(m):
        for j in range(n):
            nc = int(rng.integers(0, cap + 1))
            distinct = max(1, int(rng.integers(1, nc + 1))) if nc else 0
            t = np.sort(rng.choice(rng.integers(0, max_clock + 1, size=max(distinct, 1)), size=nc)) if nc else np.zeros(0, dtype=np.int64)
            ct[i, j, :nc] = t
            counts[i, j] = nc
    ct[0, 0], counts[0, 0] = -1, 0  # an empty row
    ct[0, 1], counts[0, 1] = -1, 7
    ct[0, 1, :7] = max_clock // 3  # a row of equal times
    ct[0, 2, :] = np.sort(rng.integers(0, max_clock + 1, size=cap))  # a full row ...
    counts[0, 2] = cap + 3  # ... of a node that committed more than the log holds: nc = cap
    ct[1, 0], counts[1, 0] = -1, 2
    ct[1, 0, :2] = (0, max_clock)  # instants at both ends of [0, max_clock]
    return ct, counts


def test_shim_equals_the_numpy_reference_on_drawn_rows(shim):
    rng = np.random.default_rng(20261016)
    m, n, cap, groups = 24, 4, 70, 3  # (rows longer than two segments of 32 lanes: the carry across chunks)
    for max_clock in (1000, 40000):
        ct, counts = draw_rows(rng, m, n, cap, max_clock)
        faults = np.zeros(m, dtype=np.uint32)
        faults[[3, 17]] = (8, 1)  # faulted instances are skipped, whatever their rows hold
        group_of = rng.integers(0, groups, size=m).astype(np.uint32)
        group_of[:3] = (0, 1, 2)
        instant = int(ct[5, 1, counts[5, 1] // 2]) if counts[5, 1] else max_clock // 2
        sinces = (None, [0] * groups, [max_clock] * groups, [instant] * groups, [instant + 1, 0, max_clock // 2])
        binnings = [(1, max_clock + 1), (1, 1), (7, 1), (max_clock + 5, 3), (2 ** 32 - 1, 2), (3, 50), (1, ref.LDS_BINS), (1, ref.LDS_BINS + 1)]
        if max_clock > 2 * ref.LDS_BINS:
            binnings += [(1, 3 * ref.LDS_BINS + 5), (2, 2 * ref.LDS_BINS)]  # more bins than the LDS window, with samples past it
        for since in sinces:
            for width, bins in binnings:
                series, hist, stats = compare(shim, ct, counts, faults, group_of, groups, since, max_clock, width, bins)
                assert series.sum() == counts.clip(max=cap)[faults == 0].sum()
                if bins == 1 or width > max_clock:
                    assert (series[:, 0] == series.sum(axis=1)).all() and (hist[:, 0] == stats[:, 0]).all()
                if max_clock > 2 * ref.LDS_BINS and width == 1 and bins > ref.LDS_BINS:
                    assert hist[:, ref.LDS_BINS:].sum() > 0 and series[:, ref.LDS_BINS:].sum() > 0
        # the plain-batch form: one group, no group array
        compare(shim, ct, counts, faults, None, 1, None, max_clock, 5, 64)
        # since at an instant exactly counts that instant (distance 0); one past it does not
        _, st_at = ref.stalls(ct[5:6], counts[5:6], None, None, 1, [instant], 1, 1, max_clock)
        if counts[5, 1]:
            assert st_at[0, 4 * ref.FIRST + 2] == 0


def test_rows_by_hand(shim):
    """Three rows whose samples are written out: instants 10, 10, 25, 70 / no commit / one commit at 0, horizon 100."""
    ct = np.full((1, 3, 4), -1, dtype=np.int64)
    ct[0, 0] = (10, 10, 25, 70)
    ct[0, 2, 0] = 0
    counts = np.array([[4, 0, 1]], dtype=np.uint32)
    for seg in (1, 2, 32):
        series, hist, stats = run_shim(shim, ct, counts, None, None, 1, [25], 100, 10, 5, seg)
        assert series.tolist() == [[1, 2, 1, 0, 1]]  # 0 | 10, 10 | 25 | - | 70 clamps into the last bin
        assert hist.tolist() == [[0, 1, 0, 0, 1]]  # gaps 15 and 45
        assert stats[0].tolist() == [2, 60, 15, 45,  # gaps
                                     1, 0, 0, 0,  # first: row 0 at 25 exactly; rows 1 and 2 have no instant at or after 25
                                     3, 30 + 100 + 100, 30, 100,  # tail
                                     3, 45 + 100 + 100, 45, 100]  # longest
    want = ref.stalls(ct, counts, None, None, 1, [25], 10, 5, 100)
    assert (want[0] == hist).all() and (want[1] == stats).all()
    assert (ref.series(ct, counts, None, None, 1, 10, 5) == series).all()


def test_oracle_scenario_shows_the_stall_and_the_recovery(shim, oracle):
    ct, counts, set_of, _ = ref.scenario_oracle(oracle, THREADS)
    sc = ref.SCENARIO
    mc, end = sc["max_clock"], sc["partition"][2]
    series, _, stats = compare(shim, ct, counts, None, set_of, 2, [0, end], mc, 20, -(-(mc + 1) // 20))
    ref.check_scenario(series, 20, stats)
    series1, _, _ = compare(shim, ct, counts, None, set_of, 2, None, mc, 1, mc + 1)
    assert series1[1, ref.SCENARIO_SETTLE:end].sum() == 0 and series1[0, ref.SCENARIO_SETTLE:end].sum() > 1000
    # (the figures the oracle gives: per node, the longest interval is 325 .. 524 with the partition and 76 .. 125 without)
    assert stats[1, 4 * ref.LONGEST + 2] == 325 and stats[0, 4 * ref.LONGEST + 3] == 125, stats
