"""The three passes of lbft_k_ps_votes on the host (tests/vote_stats_host_model.cpp, compiled here with g++): plain batches run through the
kernel logic on the CPU, then every instance's chain and block pool walked over csrc/lbft_vote_rules.h the way the kernel does it, with
the chunk width a parameter.  Widths 1, 7 and 64 must give the same four arrays, and those must equal the definitions restated over the
oracle's node images (tests/vote_stats_reference.py) -- which are pinned to literals first.  The walk reads no block record whose id it
has not checked, and its membership rule (one gather by ledger depth) agrees with set membership in the chain on every block of every
case.  On state edited by hand: a log entry of 0 or above the block count ends the chain there, a chain entry without voters gives no
sample to the vote families, an instance with a fault word is skipped."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import vote_stats_cases as cases
import vote_stats_reference as ref
from support import ModelBase, build_pool_walk_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "vote_stats_host_model.cpp")


def load_shim(tmp_dir):
    L = build_pool_walk_shim(tmp_dir, "vote_stats_host_model.cpp", "libvt_hostmodel.so", "vtm")
    vp, u32 = C.c_void_p, C.c_uint32
    L.vtm_counts.argtypes = [vp, vp, vp, vp]
    L.vtm_walk.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, vp]
    L.vtm_walk.restype = C.c_int
    L.vtm_clear_voters.argtypes = [vp, u32, u32]
    L.vtm_clear_voters.restype = u32
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_shim(tmp_path_factory.mktemp("vt_host"))


class Model(ModelBase):
    PREFIX = "vtm"

    def counts(self):
        cc = np.zeros((self.m, self.n), dtype=np.uint32)
        faults = np.zeros(self.m, dtype=np.uint32)
        nblocks = np.zeros(self.m, dtype=np.uint32)
        self.L.vtm_counts(self.h, cc.ctypes.data, faults.ctypes.data, nblocks.ctypes.data)
        return cc, faults, nblocks

    def walk(self, W, width=None, bins=None):
        w, b = ref.default_binning(self.rights, self.n)
        width, bins = (w if width is None else width), (b if bins is None else bins)
        margin = np.full((1, bins), 0xdead, dtype=np.uint64)  # (the walk zeroes its outputs itself)
        votes = np.full((1, self.n + 1), 0xdead, dtype=np.uint64)
        nodes = np.full((1, self.n, ref.NODE_COLUMNS), 0xdead, dtype=np.uint64)
        stats = np.full((1, ref.VOTE_STATS), 0xdead, dtype=np.uint64)
        check = np.zeros(2, dtype=np.uint64)
        assert self.L.vtm_walk(self.h, W, width, bins, margin.ctypes.data, votes.ctypes.data, nodes.ctypes.data, stats.ctypes.data, check.ctypes.data) == 0
        assert check[0] == 0, "the walk read %d block records whose id it had not checked" % check[0]
        assert check[1] == 0, "the membership rule differs from set membership on %d blocks" % check[1]
        return margin, votes, nodes, stats


def equal(got, want):
    for name, a, b in zip(("margin_hist", "votes_hist", "node_table", "stats"), got, want):
        assert a.shape == b.shape and (a == b).all(), (name, a.tolist(), b.tolist())


def test_the_reference_gives_the_published_figures(oracle):
    """The oracle's side of the four configurations, pinned to literals before anything is held to it."""
    s = lambda name: cases.expected(cases.case_instances(oracle, name), cases.CASES[name][0]["num_nodes"], cases.CASES[name][0].get("voting_rights"))
    fam = lambda stats, f: [int(v) for v in stats[0, 4 * f:4 * f + 4]]
    # 4 nodes, seeds 1..16, clock 1000
    margin, votes, nodes, stats = s("n4")
    assert fam(stats, ref.BLOCKS)[1] == 633 and fam(stats, ref.ORPHANED)[1] == 60 and fam(stats, ref.PENDING)[1] == 47
    assert fam(stats, ref.VOTES) == [526, 3 * 526, 3, 3] and votes.tolist() == [[0, 0, 0, 526, 0]]
    assert nodes[0, :, ref.COL_ORPHANED].tolist() == [9, 18, 20, 13] and nodes[0, :, ref.VOTED].tolist() == [405, 375, 393, 405]
    assert fam(stats, ref.SKIPPED)[1:] == [60, 0, 1] and sum(i["length"] for i in cases.case_instances(oracle, "n4")) == 526
    # rights [5, 1, 1, 1, 1], seeds 1..8
    margin, votes, nodes, stats = s("n5_weighted")
    assert votes.tolist() == [[0, 0, 0, 225, 30, 35]] and margin.tolist() == [[225, 30, 35]] and fam(stats, ref.BLOCKS)[1] == 341
    voted = nodes[0, :, ref.VOTED].tolist()
    assert voted[0] == 290 and min(voted[1:]) == 162 and max(voted[1:]) == 183
    # node 0 cut off during [300, 600)
    margin, votes, nodes, stats = s("n4_partition_q3")
    assert nodes[0, :, ref.VOTED].tolist() == [400, 440, 468, 483] and fam(stats, ref.VOTES)[0] == 597 and fam(stats, ref.BLOCKS)[1] == 729
    skipped = sum((i["skipped"] for i in cases.case_instances(oracle, "n4_partition_q3")), [])
    assert {v: skipped.count(v) for v in set(skipped)} == {0: 490, 1: 81, 2: 8, 3: 2}
    # rotating rights
    margin, votes, nodes, stats = s("n4_rotating_q3")
    assert [fam(stats, f)[1] for f in (ref.BLOCKS, ref.ORPHANED, ref.PENDING, ref.CERTIFIED_OFF)] == [511, 176, 31, 154]
    assert sum(i["length"] for i in cases.case_instances(oracle, "n4_rotating_q3")) == 304


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_walk_equals_the_reference_for_every_width(shim, oracle, name):
    kw, max_clock, seeds = cases.CASES[name]
    model = Model(shim, kw, max_clock, seeds)
    cc, faults, nblocks = model.counts()
    assert not faults.any() and cc.max() <= model.lcap and nblocks.max() <= model.bcap
    instances = cases.case_instances(oracle, name)
    # the pool of the host build has exactly the blocks of the union of the oracle's node images
    assert nblocks.tolist() == [i["blocks"] for i in instances] and cc.max(axis=1).tolist() == [i["length"] for i in instances]
    lengths = sum(i["length"] for i in instances)
    for width, bins in ((None, None), (7, 5)):
        got = model.same_for_every_width(width=width, bins=bins)
        equal(got, cases.expected(instances, model.n, model.rights, width, bins))
        ref.identities(*got, lengths_sum=[lengths], unit=model.rights is None)
    margin, votes, nodes, stats = got
    if name == "n4_longer_than_64":
        assert cc.max(axis=1).min() > 64 and nblocks.min() > 64
    if name == "n4_empty_chain":
        assert not cc.any() and stats[0, 4 * ref.ORPHANED + 1] == 0 and stats[0, 4 * ref.PENDING + 1] == nblocks.sum() > 0
    if name == "n33":
        assert nodes[0, 32, ref.VOTED] > 0 and votes[0, 23:].sum() == stats[0, 0] > 0  # the 33rd node: the second voter word
    if name == "n65_q3":
        assert nodes[0, 64, ref.VOTED] > 0 and votes[0, 44:].sum() == stats[0, 0] > 0  # the 65th node: the third voter word
    if "rotating" in name:
        assert cc.max() > kw["commands_per_epoch"] and stats[0, 4 * ref.SKIPPED] < stats[0, 0] - model.m  # pairs across epochs give no sample
    model.close()


def test_ids_outside_the_pool_end_the_chain(shim):
    for k, value in ((6, 0), (8, None), (0, 0xfffffff0), (70, 0)):
        model = Model(shim, dict(num_nodes=4), 2500, [1])
        _, _, nblocks = model.counts()
        nb = int(nblocks[0])
        r, length = model.chain(0)
        assert length > 71
        _, votes0, nodes0, stats0 = model.same_for_every_width()
        model.log(0, r, k, nb + 1 if value is None else value)
        margin, votes, nodes, stats = model.same_for_every_width()  # (asserts: no read of an unchecked record, for every width)
        # entries 0 .. k - 1 are the chain: each has a certificate of three votes; the pool is sorted against that chain
        assert stats[0, 4 * ref.VOTES:4 * ref.VOTES + 2].tolist() == [k, 3 * k] and stats[0, 4 * ref.SKIPPED] == max(k - 1, 0)
        assert stats[0, 4 * ref.BLOCKS + 1] == nb == k + stats[0, 4 * ref.ORPHANED + 1] + stats[0, 4 * ref.PENDING + 1]
        assert (nodes[0, :, ref.PROPOSED] == nodes0[0, :, ref.PROPOSED]).all()
        if k == 0:
            assert stats[0, 4 * ref.ORPHANED + 1] == 0 and stats[0, 4 * ref.PENDING + 1] == nb  # no tip
        ref.identities(margin, votes, nodes, stats, lengths_sum=[k])
        model.close()


def test_a_chain_entry_without_voters_gives_no_vote_sample(shim):
    model = Model(shim, dict(num_nodes=4), 1000, [1, 2])
    r, length = model.chain(1)
    _, votes0, nodes0, stats0 = model.same_for_every_width()
    b = model.log(1, r, 9)
    assert model.L.vtm_clear_voters(model.h, 1, b) == 3
    margin, votes, nodes, stats = model.same_for_every_width()
    for f in (ref.VOTES, ref.WEIGHT, ref.MARGIN):
        assert stats[0, 4 * f] == stats0[0, 4 * f] - 1
    assert stats[0, 4 * ref.VOTES + 1] == stats0[0, 4 * ref.VOTES + 1] - 3 and votes[0, 3] == votes0[0, 3] - 1
    assert nodes[0, :, ref.VOTED].sum() == nodes0[0, :, ref.VOTED].sum() - 3
    keep = [4 * f + w for f in (ref.SKIPPED, ref.BLOCKS, ref.ORPHANED, ref.PENDING, ref.CERTIFIED_OFF) for w in range(4)]
    assert (stats[0, keep] == stats0[0, keep]).all()  # the entry stays on the chain
    ref.identities(margin, votes, nodes, stats)
    model.close()


def test_a_faulted_instance_is_skipped(shim, oracle):
    kw, max_clock, seeds = cases.CASES["n4"]
    seeds = list(seeds)[:3]
    model = Model(shim, kw, max_clock, seeds)
    instances = cases.oracle_instances(oracle, kw, max_clock, seeds)
    equal(model.same_for_every_width(), cases.expected(instances, 4, None))
    model.L.vtm_set_fault(model.h, 1, 1 << 3)
    got = model.same_for_every_width()
    equal(got, cases.expected(instances, 4, None, faults=[0, 8, 0]))
    assert got[3][0, 4 * ref.BLOCKS] == 2
    model.close()


@pytest.mark.skipif(not shutil.which("g++"), reason="needs g++")
def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The shim with its own main as a program, under the address and undefined-behaviour sanitizers: the walks over an id of 0 and one
    far above the pool read nothing outside the state array."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")
    exe = str(tmp_path / "vt_hostmodel_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-w", "-DVTM_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout[-500:], run.stderr[-3000:])
