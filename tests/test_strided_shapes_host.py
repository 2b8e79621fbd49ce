"""The preconditions of tests/test_grouped_stats_stride_gpu.py, stated once on the CPU: at every shape of tests/strided_shapes.py the
launchers' grid rule -- the three host shims compile it as the launchers call it -- leaves a wavefront more than one instance of the
largest group, the Python mirror of the rule equals the shims, the trip counts are the patterns the shapes were chosen for, and the
oracle's runs of the layout have the chains and the mix of faulted and clean instances that the device tests rely on.  An edit of a
shape, of a seed or of a *_WORKGROUPS constant cannot turn the device tests back into single-trip tests without failing here."""
import ctypes as C

import numpy as np
import pytest

import strided_shapes as S
from support import build_shim

LCAP = S.MAX_CLOCK // 10 + 64  # the planner's log capacity of the layout's horizon (csrc/lbft_plan.h: one block per round)
FAST_MEDIAN = 145  # of the oracle's chains of the FAST group, on both 4-node flavours


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("strided_host")
    chn = build_shim(tmp, "chain_stats_host.cpp", "libchn_host.so")
    fin = build_shim(tmp, "commit_finality_host.cpp", "libfin_host.so")
    rtl = build_shim(tmp, "round_stats_host.cpp", "librtl_host.so")
    for fn, args in ((chn.chn_workgroups_host, 6), (fin.fin_workgroups_host, 5), (rtl.gs_workgroups_host, 4)):
        fn.argtypes, fn.restype = [C.c_uint64] * args, C.c_uint64
    return chn, fin, rtl


def grids(shims, groups, max_group, lcap, n, rcap):
    """gridDim.x of the three launchers, (chain, finality, rounds), by the shims."""
    chn, fin, rtl = shims
    return (chn.chn_workgroups_host(S.TARGET, groups, max_group, S.WAVES, lcap, n), fin.fin_workgroups_host(S.TARGET, groups, max_group, S.WAVES, lcap),
            rtl.gs_workgroups_host(S.TARGET, groups, (max_group + S.WAVES - 1) // S.WAVES, max_group * n * rcap))


def mirror(groups, max_group, lcap, n, rcap):
    return (S.grid_x(groups, max_group, max(lcap, n)), S.grid_x(groups, max_group, lcap), S.grid_x(groups, max_group, n * rcap))


# (groups, largest group, log capacity, nodes, trace capacity) of every shape of the device module
SHAPES = {
    "class0": (S.GROUPS, 38, LCAP, 4, S.ROUND_TRACE), "partition": (S.GROUPS, 38, LCAP, 4, S.ROUND_TRACE), "tiles": (S.GROUPS, 38, LCAP, 7, S.ROUND_TRACE),
    "faults": (S.GROUPS, 38, FAST_MEDIAN, 4, S.ROUND_TRACE),
    "plain": (1, S.PLAIN["m"], S.PLAIN["max_clock"] // 10 + 64, S.PLAIN["n"], S.ROUND_TRACE),
    "weighted": (1, S.WEIGHTED["m"], S.WEIGHTED["max_clock"] // 10 + 64, S.WEIGHTED["n"], S.ROUND_TRACE),
}


def test_the_layouts_largest_group_and_the_constants():
    for flavour, f in S.FLAVOURS.items():
        sizes = S.group_sizes(f["background"])
        set_of, seeds = S.assignment(f["background"])
        assert sizes.max() == SHAPES[flavour][1] == 38 and len(sizes) == S.GROUPS and sizes[S.EMPTY_LAST] == 0 and (sizes == 0).sum() > 10
        assert (np.bincount(set_of, minlength=S.GROUPS) == sizes).all() and len(seeds) == sizes.sum() and len(set(seeds.tolist())) == len(seeds)
        for g in S.SPECIAL:  # scattered over the batch: grp_inst is a real gather
            idx = S.members(set_of, g)
            assert (np.diff(idx) > 0).all() and (np.diff(idx) > 1).any() and idx[-1] - idx[0] > 2 * len(idx)
        assert len(S.param_sets(flavour)) == S.GROUPS
    assert sorted(S.SPECIAL.values()) == [16, 17, 33, 38, 38, 38]
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "librabft_simulator_amd", "csrc")
    for name, tag in (("lbft_chain_stats.hip", "CS"), ("lbft_commit_times.hip", "FN"), ("lbft_round_stats.hip", "RS")):
        src = open(os.path.join(csrc, name)).read()
        assert "#define LBFT_%s_WORKGROUPS %du" % (tag, S.TARGET) in src and "#define LBFT_%s_BLOCK %d" % (tag, 64 * S.WAVES) in src, name


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_shape_leaves_a_wavefront_more_than_one_instance(shims, shape):
    groups, max_group, lcap, n, rcap = SHAPES[shape]
    got = grids(shims, groups, max_group, lcap, n, rcap)
    assert got == mirror(groups, max_group, lcap, n, rcap)
    for gx in got:
        assert S.WAVES * gx < max_group and max(S.trips(max_group, gx)) >= 2, (shape, got)
    assert got == ((4, 4, 4) if groups == S.GROUPS else (1024, 1024, 1024))


def test_the_mirror_equals_the_shims_on_the_grid_rules_tables(shims):
    chn, fin, rtl = shims
    # tests/test_chain_stats_host.py's table: (groups, largest group, lcap, n, gridDim.x)
    for groups, max_group, lcap, n, want in ((1, 65536, 64, 4, 1024), (64, 1024, 64, 4, 16), (256, 1, 64, 4, 1), (1, 7, 64, 100, 2), (2048, 5000, 64, 4, 1),
                                             (256, 1 << 24, 4096, 4, 33), (1, 1 << 26, 16, 128, 1024), (1, 1 << 26, 65536, 128, 2049)):
        assert S.grid_x(groups, max_group, max(lcap, n)) == chn.chn_workgroups_host(S.TARGET, groups, max_group, S.WAVES, lcap, n) == want
    # tests/test_commit_finality_host.py's
    for groups, max_group, lcap, want in ((1, 65536, 64, 1024), (64, 1024, 64, 16), (256, 1, 64, 1), (1, 7, 64, 2), (256, 1 << 24, 4096, 33)):
        assert S.grid_x(groups, max_group, lcap) == fin.fin_workgroups_host(S.TARGET, groups, max_group, S.WAVES, lcap) == want
    # tests/test_round_stats_host.py's: (groups, largest group, n, rcap)
    for groups, max_group, n, cap in ((1, 65536, 4, 64), (256, 1024, 4, 64), (256, 1, 4, 64), (1, 1, 1, 1), (7, 1, 32, 4096), (1, 3, 4, 16), (1, 37, 3, 100),
                                      (64, 9, 2, 8), (256, 1 << 20, 32, 4096), (1, 1 << 26, 32, 65534), (1000, 1 << 22, 16, 2048), (2048, 5000, 4, 64)):
        steps = (max_group + S.WAVES - 1) // S.WAVES
        assert S.grid_x(groups, max_group, n * cap) == S.gs_workgroups(S.TARGET, groups, steps, max_group * n * cap) \
            == rtl.gs_workgroups_host(S.TARGET, groups, steps, max_group * n * cap), (groups, max_group, n, cap)


def test_trip_counts_are_the_patterns_the_shapes_were_chosen_for():
    assert S.trips(38, 4) == [3] * 6 + [2] * 10
    assert S.trips(38, 4)[4:8] == [3, 3, 2, 2]  # workgroup 1: its wavefronts leave the loop after different numbers of trips
    assert S.trips(33, 4) == [3] + [2] * 15
    assert S.trips(17, 4) == [2] + [1] * 15
    assert S.trips(16, 4) == [1] * 16  # the boundary: exactly one step, no stride
    assert S.trips(3, 4) == [1] * 3 + [0] * 13 and S.trips(0, 4) == [0] * 16
    plain = S.trips(S.PLAIN["m"], 1024)
    assert len(plain) == 4096 and plain[:4] == [2] * 4 and plain[4:8] == [2, 2, 1, 1] and plain[8:] == [1] * 4088
    assert sum(plain) == S.PLAIN["m"] == S.WEIGHTED["m"] and sum(S.trips(38, 4)) == 38
    assert S.trips(10, 2, waves=2) == [3, 3, 2, 2]


def positions(faulted, stride=16):
    """Per wavefront position of a group (its instances in instance order, as GroupIndex lists them): the fault flags of its trips."""
    return [list(map(bool, faulted[q0::stride])) for q0 in range(min(stride, len(faulted)))]


@pytest.mark.parametrize("flavour,outliers,outgrow", [("class0", 0, 15), ("partition", 0, 15), ("tiles", 4, 17)])
def test_the_oracles_chains_of_the_layout(oracle, flavour, outliers, outgrow):
    set_of, seeds, want = S.oracle_layout(oracle, flavour)
    lengths = want[1].max(axis=1)
    print("chain lengths per special group:", {g: (int(lengths[S.members(set_of, g)].min()), int(lengths[S.members(set_of, g)].max())) for g in S.SPECIAL})
    assert lengths.max() < LCAP  # nothing overflows the default capacities: cases A and C are clean
    fast = lengths[S.members(set_of, S.FAST)]
    # three 64-entry chunks (7 nodes with loss: two), but for the short-chain outliers these seeds leave
    floor = 128 if flavour != "tiles" else 64
    assert (fast <= 128).sum() == outliers and (fast > floor).all() and len(fast) == 38
    assert lengths[S.members(set_of, S.DEFAULT)].max() < 64 and lengths[S.members(set_of, S.DEFAULT)].min() > 0
    lcap, faults = S.fault_case(want, set_of)
    assert lcap == np.median(fast)
    if flavour == "tiles":  # (case C is clean: its median, and how many outgrow it, only for the record)
        assert (fast > lcap).sum() == outgrow
        return
    assert lcap == FAST_MEDIAN
    grown = faults[S.members(set_of, S.FAST)] != 0
    assert grown.sum() == outgrow and 0 < grown.sum() < len(grown)  # neither none nor all of it
    pos = positions(grown)
    assert [len(p) for p in pos] == S.trips(38, 4)
    assert any(p[0] and not all(p[1:]) for p in pos), pos  # a faulted first trip, a clean later one
    assert any(not p[0] and any(p[1:]) for p in pos), pos  # and the reverse
    assert any(p[1] and not p[0] and not p[2] for p in pos if len(p) == 3), pos  # the `continue` in the middle of three trips
    if flavour == "class0":  # case B: groups that are faulted throughout, and strided groups that hold no fault at all
        sizes = S.group_sizes()
        whole = [g for g in range(S.GROUPS) if sizes[g] and (faults[S.members(set_of, g)] != 0).all()]
        assert whole and S.FAST not in whole
        assert not faults[np.isin(set_of, (S.DEFAULT, S.THIRD, S.G33, S.G17, S.G16))].any()


def test_the_oracles_chains_of_the_plain_shapes(oracle):
    import round_stats_reference as round_ref
    from support import oracle_cfg
    for shape, least in ((S.PLAIN, 5), (S.WEIGHTED, 9)):  # (WEIGHTED: three epochs of 3 commands and more)
        seeds, want = S.oracle_plain(oracle, shape)
        lengths = want[1].max(axis=1)
        print("chain lengths:", int(lengths.min()), int(lengths.max()))
        assert len(seeds) == 4102 and len(set(seeds.tolist())) == 4102 and lengths.min() >= least and lengths.max() < 64
        # the six wavefronts that make two trips (positions 0 .. 5, then 4096 .. 4101): one of them takes a second instance with fewer
        # rounds than its first
        two = [q for q, t in enumerate(S.trips(shape["m"], 1024)) if t == 2]
        assert two == list(range(6))
        idx = np.r_[two, 4096 + np.array(two)]
        _, max_rounds, _ = round_ref.oracle_tables(oracle, oracle_cfg(oracle, shape["n"], S.ParamSet(), **shape["kw"]), seeds[idx], shape["max_clock"])
        print("rounds of the first and second trips:", max_rounds[:6].tolist(), max_rounds[6:].tolist())
        assert (max_rounds[:6] > max_rounds[6:]).any()
