"""The four kernels that walk chain and block pool with csrc/lbft_chain_walk.h -- lbft_k_cs_chain, lbft_k_rh_chain, lbft_k_ps_votes and
lbft_k_ps_epochs -- on one finished run each of two clean batches: the three 4-node instances of tests/test_pool_walk_host.py, whose
chains exceed one chunk of 64, and two instances of 100 nodes (two node rounds in the node pass).  The four calls must tell of the same
chains: the chain statistics' `length` sums to the heads' lengths, to the epoch table's entries and to blocks - orphaned - pending of
the vote statistics (include/lbft.h: per instance blocks = L + orphaned + pending), and every head names the reference node and the
length the host model's node pass gives."""
import numpy as np
import pytest

import chain_stats_reference as cs_ref
import epoch_stats_reference as ep_ref
import test_pool_walk_host as host
import test_vote_stats_host as vt
import vote_stats_reference as vt_ref
from support import amd, device_batch  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return vt.load_shim(tmp_path_factory.mktemp("pw_gpu"))


@pytest.mark.parametrize("batch", ("3x4", "2x100"))
def test_the_four_walks_agree_on_the_chains(amd, shim, batch):
    kw, seeds, clock = (host.KW, host.SEEDS, host.long_chain_clock(shim)) if batch == "3x4" else (dict(num_nodes=100), (1, 2), 300)
    sim = device_batch(amd, kw, seeds)
    res = sim.loop_until(clock)
    assert not res.faults.any()
    _, _, chain = res.chain_stats()
    heads = res.chain_heads()
    _, _, _, votes = res.vote_stats()
    _, table, _ = res.epoch_stats()
    lengths = int(heads["length"].sum())
    v = votes.astype(np.int64)[0]
    print(batch, "clock", clock, "lengths", heads["length"].tolist(), "ref", heads["ref_node"].tolist())
    assert lengths > 0 and int(chain[0, 4 * cs_ref.LENGTH + 1]) == lengths
    assert int(table[0, :, ep_ref.COL_ENTRIES].sum()) == lengths
    assert int(v[4 * vt_ref.BLOCKS + 1] - v[4 * vt_ref.ORPHANED + 1] - v[4 * vt_ref.PENDING + 1]) == lengths
    model = vt.Model(shim, kw, clock, seeds)
    assert [model.chain(i) for i in range(model.m)] == [(int(h["ref_node"]), int(h["length"])) for h in heads]
    if batch == "3x4":
        assert heads["length"].min() > 64
    else:
        assert model.n > 64
    model.close()
    sim.close()
