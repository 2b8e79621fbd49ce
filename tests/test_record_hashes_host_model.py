"""The walk of lbft_k_rh_chain on the host (tests/record_hashes_host_model.cpp, compiled here with g++): plain batches run through the
kernel logic on the CPU, then every instance's committed chain hashed the way the kernel does it, with the segment width W (= the block
size) a parameter.  W = 4, 8 and 64 must give the same arrays; for every node they must equal SimT::committed_record_hashes (what
lbft_batch_committed_record_hashes runs) and the oracle's committed_record_hashes.  On state edited by hand: a log entry of 0 or above the
block count stops the walk with flag bit 2 and without a read of an unchecked block record, a differing entry of a node's log gives that
index as its node_prefix, an instance with a fault word is skipped."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from support import ModelBase, build_pool_walk_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "record_hashes_host_model.cpp")
HEAD_DTYPE = np.dtype([("block_hash", "<u8"), ("state", "<u8"), ("qc_hash", "<u8"), ("length", "<u4"), ("ref_node", "<u4"),
                       ("num_votes", "<u4"), ("flags", "<u4")])
SEEDS = np.array([52, 7, 1234567], dtype=np.uint64)
CONFIGS = {
    "golden_n3": (dict(num_nodes=3), 1000),
    "n4": (dict(num_nodes=4), 1000),
    "n7_weighted_epochs_q2": (dict(num_nodes=7, voting_rights=[2, 1, 1, 3, 1, 2, 1], commands_per_epoch=9, quirks=2), 2000),
    "n4_rotating_rights_q3": (dict(num_nodes=4, commands_per_epoch=5, quirks=3, voting_rights=[1, 2, 3, 4], rights_rotation=1), 1500),
    "n7_equivocators": (dict(num_nodes=7, equivocate_every=3), 1000),
    "n4_longer_than_64": (dict(num_nodes=4), 2500),
}
BAD_ID = 4


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = build_pool_walk_shim(tmp_path_factory.mktemp("rh_host"), "record_hashes_host_model.cpp", "librh_hostmodel.so", "rhm")
    vp, u32 = C.c_void_p, C.c_uint32
    L.rhm_counts.argtypes = [vp, vp, vp, vp]
    L.rhm_walk.argtypes = [vp, u32, vp, C.c_size_t, vp, vp]
    L.rhm_walk.restype = C.c_int64
    L.rhm_node.argtypes = [vp, u32, u32, vp, u32]
    L.rhm_node.restype = u32
    return L


class Model(ModelBase):
    PREFIX, WIDTHS = "rhm", (4, 8, 64)

    def __init__(self, L, kw, max_clock, seeds=SEEDS):
        super().__init__(L, kw, max_clock, seeds)

    def counts(self):
        cc = np.zeros((self.m, self.n), dtype=np.uint32)
        faults = np.zeros(self.m, dtype=np.uint32)
        nblocks = np.zeros(self.m, dtype=np.uint32)
        self.L.rhm_counts(self.h, cc.ctypes.data, faults.ctypes.data, nblocks.ctypes.data)
        return cc, faults, nblocks

    def walk(self, W, cap=None, entries=True, prefix=True):
        from librabft_simulator_amd import _lib
        cap = self.lcap if cap is None else cap
        out = np.zeros((self.m, cap), dtype=_lib.RECORD_HASH_DTYPE)
        out["flags"] = 0xdead  # (the walk zeroes its outputs itself)
        heads = np.zeros(self.m, dtype=HEAD_DTYPE)
        heads["length"] = 0xdead
        pre = np.full((self.m, self.n), 0xdead, dtype=np.uint32)
        unchecked = self.L.rhm_walk(self.h, W, out.ctypes.data if entries else None, cap, heads.ctypes.data, pre.ctypes.data if prefix else None)
        assert unchecked == 0, "the walk read %d block records whose id it had not checked" % unchecked
        return out, heads, pre

    def node(self, i, q):
        from librabft_simulator_amd import _lib
        out = np.zeros(self.lcap, dtype=_lib.RECORD_HASH_DTYPE)
        nc = self.L.rhm_node(self.h, i, q, out.ctypes.data, self.lcap)
        return out[:min(nc, self.lcap)]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_walk_equals_every_node_and_the_oracle_for_every_width(shim, oracle, name):
    kw, max_clock = CONFIGS[name]
    model = Model(shim, kw, max_clock)
    cc, faults, _ = model.counts()
    assert not faults.any() and cc.max() <= model.lcap
    out, heads, pre = model.same_for_every_width()
    assert HEAD_DTYPE.itemsize == 40 and out.dtype.itemsize == 32
    assert (pre == cc).all()  # every history is a prefix of its chain
    assert (heads["length"] == cc.max(axis=1)).all() and (heads["ref_node"] == cc.argmax(axis=1)).all()
    cfg = oracle.make_config(**kw)
    for i, seed in enumerate(SEEDS):
        sim = oracle.OracleSim(cfg, int(seed)).run_until(max_clock)
        length = int(heads["length"][i])
        if name == "n4_longer_than_64":
            assert max(sim.commit_counts()) > 64  # (on the oracle: the chain crosses the 64-entry seam at W = 64)
        assert not out[i, length:].tobytes().strip(b"\0")
        for f in ("block_hash", "state", "qc_hash", "num_votes", "flags"):
            assert heads[f][i] == out[f][i, length - 1]
        for q in range(model.n):
            mine = model.node(i, q)
            ref = sim.committed_record_hashes(q)
            assert len(mine) == len(ref) == cc[i, q] > 0
            assert out[i, :len(mine)].tobytes() == mine.tobytes()
            for f in ("block_hash", "state", "qc_hash", "num_votes"):
                assert (out[f][i, :len(ref)] == ref[f]).all(), (name, i, q, f)
            assert not out["flags"][i, :len(ref)].any() and ref["has_qc"].all()
    if "epochs" in name or "rotating" in name:  # the epoch-id hash was taken: more commits than an epoch holds
        assert cc.max() > kw["commands_per_epoch"]
    # heads alone, and a capacity below the chains: the heads stay, the entries are cut
    _, heads_only, _ = model.same_for_every_width(entries=False, prefix=False)
    assert heads_only.tobytes() == heads.tobytes()
    short, heads_short, _ = model.same_for_every_width(cap=5)
    assert heads_short.tobytes() == heads.tobytes() and short.tobytes() == np.ascontiguousarray(out[:, :5]).tobytes()
    model.close()


def test_ids_outside_the_pool_stop_the_walk(shim):
    model = Model(shim, dict(num_nodes=4), 1000)
    cc, _, nblocks = model.counts()
    out0, heads0, _ = model.same_for_every_width()
    assert heads0["length"].min() > 12
    refs = heads0["ref_node"]
    # (instance, entry, value): 0, just above the block count, far outside the state array, and at entry 0 / at a seam of W = 4 and 8
    edits = [(0, 6, 0), (1, 8, int(nblocks[1]) + 1), (2, 0, 0xfffffff0)]
    for i, k, v in edits:
        model.log(i, int(refs[i]), k, v)
    out, heads, pre = model.same_for_every_width()
    for i, k, v in edits:
        assert heads[i]["length"] == k + 1 and heads[i]["flags"] == BAD_ID and heads[i]["ref_node"] == refs[i]
        assert heads[i]["block_hash"] == heads[i]["state"] == heads[i]["qc_hash"] == heads[i]["num_votes"] == 0
        assert out[i, :k].tobytes() == out0[i, :k].tobytes()  # what lies below the entry is untouched
        assert out[i, k]["flags"] == BAD_ID and out[i, k]["block_hash"] == 0 and not out[i, k + 1:].tobytes().strip(b"\0")
        # the other nodes still hold the block there: their logs differ from the chain's at k
        for q in range(model.n):
            assert pre[i, q] == (k + 1 if q == refs[i] else min(k, cc[i, q])), (i, q)
    # the largest id of the pool is one of the pool's
    model.log(0, int(refs[0]), 6, int(nblocks[0]))
    _, heads, _ = model.same_for_every_width()
    assert heads[0]["length"] == heads0[0]["length"] and heads[0]["flags"] in (0, 2)
    model.close()


def test_node_prefix_is_the_first_differing_entry(shim):
    model = Model(shim, dict(num_nodes=4), 1000)
    cc, _, _ = model.counts()
    _, heads0, pre0 = model.same_for_every_width()
    assert (pre0 == cc).all()
    for i in range(model.m):
        ref = int(heads0["ref_node"][i])
        others = [q for q in range(model.n) if q != ref]
        # entry 0, the node's last entry, an entry at the seam of two blocks (W = 4, 8: entry 8; W = 64 has it inside a block)
        edits = [(others[0], 0), (others[1], int(cc[i, others[1]]) - 1), (others[2], 8)]
        for q, k in edits:
            old = model.log(i, q, k)
            model.log(i, q, k, old + 1)  # (another id)
        out, heads, pre = model.same_for_every_width()
        assert heads[i].tobytes() == heads0[i].tobytes()  # the chain is the reference node's: untouched
        want = cc[i].copy()
        for q, k in edits:
            want[q] = k
        assert (pre[i] == want).all(), (i, pre[i], want)
    model.close()


def test_a_faulted_instance_is_skipped(shim):
    model = Model(shim, dict(num_nodes=4), 600)
    out0, heads0, pre0 = model.same_for_every_width()
    model.L.rhm_set_fault(model.h, 1, 1 << 3)
    out, heads, pre = model.same_for_every_width()
    assert not heads[1].tobytes().strip(b"\0") and not out[1].tobytes().strip(b"\0") and not pre[1].any()
    for i in (0, 2):
        assert out[i].tobytes() == out0[i].tobytes() and heads[i].tobytes() == heads0[i].tobytes() and (pre[i] == pre0[i]).all()
    model.close()


def test_an_empty_chain_gives_zeros(shim):
    model = Model(shim, dict(num_nodes=4), 5)
    cc, _, _ = model.counts()
    assert not cc.any()
    out, heads, pre = model.same_for_every_width()
    assert not heads.tobytes().strip(b"\0") and not out.tobytes().strip(b"\0") and not pre.any()
    model.close()


@pytest.mark.skipif(not shutil.which("g++"), reason="needs g++")
def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The shim with its own main as a program, under the address and undefined-behaviour sanitizers: the walks over an id of 0 and one
    far above the pool read nothing outside the state array."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")
    exe = str(tmp_path / "rh_hostmodel_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-w", "-DRHM_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout[-500:], run.stderr[-3000:])
