"""The chunk head the host models of the pool-and-chain kernels share (tests/pool_walk_host.h: cw_chunk, cw_ends and the counted record
reader), held directly to what it must yield, at chunk widths 1, 7 and 64: on three 4-node instances whose chains are longer than one
chunk of 64, an id outside the pool written at entry 0, at the last lane of the first chunk, at the first lane of the second and at
the chain's last entry ends the chain exactly there, and a chain cut to exactly one chunk and to one entry more yields exactly those
entries -- without one read of a record whose id was not checked, and with the vote model and the epoch model agreeing on the length."""
import ctypes as C

import numpy as np
import pytest

import epoch_stats_reference as ep_ref
import test_epoch_stats_host as ep
import test_vote_stats_host as vt
import vote_stats_reference as vt_ref

KW, SEEDS, WIDTHS = dict(num_nodes=4), (1, 2, 3), (1, 7, 64)
BAD = (0, None, 0xfffffff0)  # per instance: 0, one above the block count, far outside the state array


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pw_host")
    return vt.load_shim(tmp), ep.load_shim(tmp)


def long_chain_clock(L, more_than=64):
    """The smallest clock (in steps of 50) at which every instance's chain has more than `more_than` entries."""
    for clock in range(50, 20000, 50):
        model = vt.Model(L, KW, clock, SEEDS)
        lengths = [model.chain(i)[1] for i in range(model.m)]
        model.close()
        if min(lengths) > more_than:
            return clock
    raise AssertionError("no chain grew past %d entries" % more_than)


@pytest.fixture(scope="module")
def clock(shims):
    return long_chain_clock(shims[0])


def entries(model, i, W):
    """What the chunk head alone yields for instance i in chunks of W: the ids, and the reads of records with an unchecked id."""
    ids, unchecked = np.full(model.lcap, 0xdead, dtype=np.uint32), C.c_uint64(0xdead)
    count = model.L.pw_chain_entries(model.h, i, W, ids.ctypes.data, model.lcap, C.byref(unchecked))
    return ids[:count].tolist(), unchecked.value


def yields(shims, clock, edit, want):
    """Both models after `edit(model, i, ref, ids)` on every instance: the walk gives the first want(i, len(ids)) entries of ids."""
    models = [vt.Model(shims[0], KW, clock, SEEDS), ep.Model(shims[1], KW, clock, SEEDS)]
    expected = []
    for model in models:
        expected = []
        for i in range(model.m):
            ref, length = model.chain(i)
            assert length > 64  # (entries 64 and length - 1 exist; a cut to 65 is one)
            ids, unchecked = entries(model, i, 64)
            assert len(ids) == length and unchecked == 0 and ids == [model.log(i, ref, k) for k in range(length)]
            edit(model, i, ref, ids)
            expected.append(ids[:want(i, length)])
        for i in range(model.m):
            for W in WIDTHS:
                assert entries(model, i, W) == (expected[i], 0), (i, W)
    total = sum(len(e) for e in expected)
    _, _, _, stats = models[0].same_for_every_width()  # (asserts: no read of an unchecked record, for every width)
    s = stats.astype(np.int64)[0]
    assert s[4 * vt_ref.BLOCKS + 1] - s[4 * vt_ref.ORPHANED + 1] - s[4 * vt_ref.PENDING + 1] == total  # lbft.h: blocks = L + orphaned + pending
    _, table, _ = models[1].same_for_every_width()
    assert table[0, :, ep_ref.COL_ENTRIES].sum() == total
    for model in models:
        model.close()


def bad_id_at(at):
    def edit(model, i, ref, ids):
        nb = int(model.counts()[2][i])
        model.log(i, ref, at(len(ids)), nb + 1 if BAD[i] is None else BAD[i])
    return edit


def test_an_id_of_0_at_entry_0_yields_no_entries(shims, clock):
    yields(shims, clock, lambda model, i, ref, ids: model.log(i, ref, 0, 0), lambda i, length: 0)


@pytest.mark.parametrize("W", WIDTHS)
def test_a_bad_id_in_the_last_lane_of_the_first_chunk_ends_the_chain_there(shims, clock, W):
    yields(shims, clock, bad_id_at(lambda length: W - 1), lambda i, length: W - 1)


@pytest.mark.parametrize("W", WIDTHS)
def test_a_bad_id_in_the_first_lane_of_the_second_chunk_ends_the_chain_there(shims, clock, W):
    yields(shims, clock, bad_id_at(lambda length: W), lambda i, length: W)


def test_a_bad_id_at_the_last_entry_ends_the_chain_there(shims, clock):
    yields(shims, clock, bad_id_at(lambda length: length - 1), lambda i, length: length - 1)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("more", (0, 1))
def test_a_chain_of_exactly_one_chunk_and_of_one_entry_more_yields_exactly_those(shims, clock, W, more):
    yields(shims, clock, lambda model, i, ref, ids: model.L.pw_cut(model.h, i, W + more), lambda i, length: W + more)
