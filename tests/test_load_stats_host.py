"""CPU test of the run load's arithmetic: a host shim (tests/load_stats_host.cpp) compiles the host part of csrc/lbft_load_stats.h --
the code lbft_k_ps_load runs per 16-lane segment -- and is fed hand-made instance words; its samples, its fault census and its
clean / faulted split equal the numpy reference written from the family table (tests/load_stats_reference.py)."""
import ctypes

import numpy as np
import pytest

import load_stats_reference as ref
from strided_shapes import gs_workgroups
from support import build_shim

ONES = 0xffffffff


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = build_shim(tmp_path_factory.mktemp("load_stats"), "load_stats_host.cpp", "libload_stats_host.so")
    vp = ctypes.c_void_p
    L.ld_rows_host.argtypes = [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, vp]
    L.ld_rows_host.restype = ctypes.c_int
    L.ld_group_host.argtypes = [vp, vp, vp] + [ctypes.c_uint32] * 5 + [vp, vp, vp]
    L.ld_group_host.restype = ctypes.c_int
    L.ld_workgroups_host.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    L.ld_workgroups_host.restype = ctypes.c_uint64
    L.ld_constant_host.argtypes = L.ld_word_of_host.argtypes = [ctypes.c_uint32]
    L.ld_constant_host.restype = L.ld_word_of_host.restype = ctypes.c_uint32
    return L


def shim_rows(L, words, commits, rounds, calendar):
    words, commits, rounds = (np.ascontiguousarray(a, dtype=np.uint32) for a in (words, commits, rounds))
    out = np.full((len(words), 16), 0xdeadbeef, dtype=np.uint32)
    assert L.ld_rows_host(words.ctypes.data, commits.ctypes.data, rounds.ctypes.data, len(words), commits.shape[1], int(calendar), out.ctypes.data) == 0
    return out


def shim_groups(L, rows, faults, set_of, groups, family, width, bins):
    rows, faults = np.ascontiguousarray(rows, dtype=np.uint32), np.ascontiguousarray(faults, dtype=np.uint32)
    group_of = None if set_of is None else np.ascontiguousarray(set_of, dtype=np.uint32)
    hist, census, stats = np.zeros((groups, bins), np.uint64), np.zeros((groups, 32), np.uint64), np.zeros((groups, 64), np.uint64)
    assert L.ld_group_host(rows.ctypes.data, faults.ctypes.data, None if group_of is None else group_of.ctypes.data, len(rows), groups, family, width, bins,
                           hist.ctypes.data, census.ctypes.data, stats.ctypes.data) == 0
    return hist, census, stats


def instances(n, rng):
    """Hand-made instances of n nodes: all zeros, all-ones words, a message sum that wraps and one that does not, distinct words, and
    drawn ones; the nodes' words put their extremes at the first node, the last node and a node past the first stride of sixteen."""
    words = [np.zeros(12, np.uint32), np.full(12, ONES, np.uint32), np.arange(1, 13, dtype=np.uint32) * 1000003,
             np.array([ONES, 1, 0] + [7] * 9, np.uint32), np.array([ONES // 2, ONES // 2, 1] + [0] * 9, np.uint32)]
    words += [rng.integers(0, 1 << 32, 12, dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    commits = [np.zeros(n, np.uint32), np.full(n, ONES, np.uint32)]
    for at in (0, n - 1, min(n - 1, 16), n // 2):
        c = np.full(n, 50, np.uint32)
        c[at] = 3
        c[(at + 1) % n] = 900 if n > 1 else 3
        commits.append(c)
    while len(commits) < len(words):
        commits.append(rng.integers(0, 1 << 20, n, dtype=np.uint64).astype(np.uint32))
    rounds = [c[::-1] // 2 + np.uint32(k) for k, c in enumerate(commits)]
    return np.array(words), np.array(commits), np.array(rounds)


def test_the_header_states_the_table_of_the_issue(shim):
    assert [shim.ld_constant_host(k) for k in range(8)] == [16, 64, 16, 32, len(ref.WORDS), 256, 1024, 8192]
    for name, k in ref.F.items():
        word = shim.ld_word_of_host(k)
        assert word == (ref.WORDS.index(ref.WORD_OF[name]) if name in ref.WORD_OF else len(ref.WORDS)), name


@pytest.mark.parametrize("n", (1, 3, 33, 128))
@pytest.mark.parametrize("calendar", (False, True))
def test_samples_equal_the_reference(shim, n, calendar):
    words, commits, rounds = instances(n, np.random.default_rng(100 + n))
    got, want = shim_rows(shim, words, commits, rounds, calendar), ref.rows(words, commits, rounds, calendar)
    assert got.dtype == want.dtype and (got == want).all(), (got, want)
    # the table, spelled out on single instances
    assert (got[0, :13] == 0).all() and (got[1, [0, 1, 2, 3, 5, 6, 7, 8, 9, 11, 12]] == ONES).all()
    assert got[1, ref.F["chunks"]] == (ONES if calendar else 0) and got[2, ref.F["chunks"]] == (10 * 1000003 if calendar else 0)
    assert got[1, ref.F["messages"]] == (3 * ONES) % (1 << 32) and got[3, ref.F["messages"]] == 0 and got[4, ref.F["messages"]] == ONES
    assert got[2, ref.F["messages"]] == 6 * 1000003
    assert (got[:, ref.F["log"]] == commits.max(axis=1)).all() and (got[:, ref.F["commits"]] == commits.min(axis=1)).all()
    assert (got[:, ref.F["rounds"]] == rounds.min(axis=1)).all() and got[1, ref.F["log"]] == ONES  # (unclamped)


def test_census_and_the_clean_faulted_split_equal_the_reference(shim):
    rng = np.random.default_rng(7)
    m, groups = 200, 5
    rows = rng.integers(0, 1 << 32, (m, 16), dtype=np.uint64).astype(np.uint32)
    rows[:, ref.F["queue"]] = rng.integers(0, 300, m)
    faults = np.zeros(m, np.uint32)
    faults[rng.choice(m, 60, replace=False)] = rng.choice(np.array([1, 1 << 12, 1 | 2 | 1 << 12, 1 << 31, ONES, 1 << 3 | 1 << 7], dtype=np.uint32), 60)
    set_of = rng.integers(0, groups - 1, m).astype(np.uint32)  # (the last group stays empty)
    only_faulted = set_of == 2
    faults[only_faulted & (faults == 0)] = 1  # a group without a clean instance
    for group_of, g in ((set_of, groups), (None, 1)):
        want_census, want_stats = ref.census(faults, group_of, g), ref.stats(rows, faults, group_of, g)
        for family, width, bins in ((ref.F["queue"], 1, 300), (ref.F["queue"], 7, 10), (ref.F["messages"], 1 << 20, 5000), (0, 1, 1), (15, ONES, 2)):
            hist, census, stats = shim_groups(shim, rows, faults, group_of, g, family, width, bins)
            assert (census == want_census).all() and (stats == want_stats).all(), (family, width, bins)
            assert (hist == ref.hist(rows, faults, family, width, bins, group_of, g)).all(), (family, width, bins)
            assert (hist.sum(axis=1) == stats[:, 0]).all()
    assert want_census.sum(axis=0)[0] == ((faults & 1) != 0).sum() and want_census[0, 12] == ((faults >> 12) & 1).sum()
    census, stats = shim_groups(shim, rows, faults, set_of, groups, 0, 1, 1)[1:]
    assert not stats[2].any() and census[2].any() and not stats[groups - 1].any() and not census[groups - 1].any()
    assert stats[0, 0] == ((set_of == 0) & (faults == 0)).sum()


def test_grid_rule_is_the_grouped_scheme_with_sixteen_instances_a_step(shim):
    for groups, max_group in ((1, 1), (1, 16), (1, 17), (1, 16400), (256, 70), (256, 3), (4, 24), (1, 1 << 20), (3, (1 << 32) - 1)):
        want = gs_workgroups(1024, groups, (max_group + 15) // 16, max_group)
        assert shim.ld_workgroups_host(groups, max_group) == want, (groups, max_group)
    assert shim.ld_workgroups_host(256, 70) == 4 and shim.ld_workgroups_host(1, 16400) == 1024  # (a second trip in both)
