"""The three passes of lbft_k_ps_epochs on the host (tests/epoch_stats_host_model.cpp, compiled here with g++): plain batches run through
the kernel logic on the CPU, then every instance's nodes, chain and block pool walked over csrc/lbft_epoch_rules.h the way the kernel does
it, with the chunk width a parameter.  Widths 1, 7 and 64 must give the same three arrays, and those must equal the definitions restated
over the oracle's node images (tests/epoch_stats_reference.py) -- which are pinned to literals first.  The walk reads no block record
whose id it has not checked.  On state edited by hand: a log entry of 0 or above the block count ends the chain and its open segment
there, decreasing epochs still give maximal runs, an epoch of 2^31 lands in the last row, an instance with a fault word is skipped, and
sums of times past 2^32 stay exact."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import epoch_stats_cases as cases
import epoch_stats_reference as ref
from support import ModelBase, build_pool_walk_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "epoch_stats_host_model.cpp")
EPOCH, ROUND, AUTHOR, TIME, DEPTH = range(5)  # epm_block's `what`


def load_shim(tmp_dir):
    L = build_pool_walk_shim(tmp_dir, "epoch_stats_host_model.cpp", "libep_hostmodel.so", "epm")
    vp, u32 = C.c_void_p, C.c_uint32
    L.epm_counts.argtypes = [vp, vp, vp, vp, vp, vp]
    L.epm_walk.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp]
    L.epm_walk.restype = C.c_int
    L.epm_block.argtypes = [vp, u32, u32, u32, C.c_int, u32]
    L.epm_block.restype = u32
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_shim(tmp_path_factory.mktemp("ep_host"))


class Model(ModelBase):
    PREFIX = "epm"

    def counts(self):
        cc, faults, nblocks = np.zeros((self.m, self.n), dtype=np.uint32), np.zeros(self.m, dtype=np.uint32), np.zeros(self.m, dtype=np.uint32)
        startup, epochs = np.zeros((self.m, self.n), dtype=np.int32), np.zeros((self.m, self.n), dtype=np.uint32)
        self.L.epm_counts(self.h, cc.ctypes.data, faults.ctypes.data, nblocks.ctypes.data, startup.ctypes.data, epochs.ctypes.data)
        return cc, faults, nblocks, startup, epochs

    def walk(self, W, width=None, bins=None, epoch_bins=64):
        width, bins = ref.default_binning(self.max_clock, width, bins)
        hist = np.full((1, bins), 0xdead, dtype=np.uint64)  # (the walk zeroes its outputs itself)
        table = np.full((1, epoch_bins, len(ref.COLUMNS)), 0xdead, dtype=np.uint64)
        stats = np.full((1, ref.EPOCH_STATS), 0xdead, dtype=np.uint64)
        check = np.zeros(1, dtype=np.uint64)
        assert self.L.epm_walk(self.h, W, width, bins, epoch_bins, hist.ctypes.data, table.ctypes.data, stats.ctypes.data, check.ctypes.data) == 0
        assert check[0] == 0, "the walk read %d block records whose id it had not checked" % check[0]
        return hist, table, stats

    def block(self, i, b, what, value=None):
        return self.L.epm_block(self.h, i, b, what, 0 if value is None else 1, 0 if value is None else value)

    def instances(self):
        """The reference's samples of every instance from the model's own state, read back field by field: the definitions of
        include/lbft.h in Python (the chain ends at the first log entry that is no pool index)."""
        cc, faults, nblocks, startup, epochs = self.counts()
        out = []
        for i in range(self.m):
            r, length = self.chain(i)
            nb = min(int(nblocks[i]), self.bcap)
            ids = []
            for k in range(length):
                y = self.log(i, r, k)
                if not 1 <= y <= nb:
                    break
                ids.append(y)
            i32 = lambda v: int(np.int32(np.uint32(v)))
            g = lambda b: i32((int(startup[i, self.block(i, b, AUTHOR)]) + self.block(i, b, TIME)) & 0xffffffff)
            chain = [(self.block(i, b, EPOCH), self.block(i, b, ROUND), g(b)) for b in ids]
            pool = [(self.block(i, b, EPOCH), b in set(ids)) for b in range(1, nb + 1)]
            out.append(ref.samples(chain, pool, [int(e) for e in epochs[i]]))
        return out, faults

    def expected(self, width=None, bins=None, epoch_bins=64):
        instances, faults = self.instances()
        return cases.expected(instances, self.max_clock, epoch_bins, width, bins, faults=faults), instances


def equal(got, want):
    for name, a, b in zip(("handover_hist", "epoch_table", "stats"), got, want):
        assert a.shape == b.shape and (a == b).all(), (name, a.tolist(), b.tolist())


def fam(stats, f):
    return [int(v) for v in stats[0, 4 * f:4 * f + 4]]


def test_the_reference_gives_the_published_figures(oracle):
    """The oracle's side, pinned to literals before anything is held to it (4 nodes, LogNormal(10, 4), seeds 1..4)."""
    s = lambda name: cases.expected(cases.case_instances(oracle, name), cases.CASES[name][1], cases.CASES[name][3])
    lengths = lambda name: [i["length"] for i in cases.case_instances(oracle, name)]
    hist, table, stats = s("n4_default")
    assert lengths("n4_default") == [30, 30, 33, 34] and fam(stats, ref.SEGMENTS) == [4, 4, 1, 1] and fam(stats, ref.BLOCKS) == [4, 157, 39, 40]
    assert fam(stats, ref.STRANDED) == [4, 0, 0, 0] and fam(stats, ref.HANDOVER) == [0, 0, 0, 0] and not hist.any()
    assert table[0, 0].tolist() == [4, 0, 127, 0, 0, 0, 157] and not table[0, 1:].any()
    hist, table, stats = s("n4_cpe5_q3")
    assert lengths("n4_cpe5_q3") == [26, 25, 26, 26] and fam(stats, ref.SEGMENTS) == [4, 23, 5, 6] and fam(stats, ref.BLOCKS) == [4, 182, 45, 46]
    assert fam(stats, ref.STRANDED) == [4, 66, 15, 18] and fam(stats, ref.LENGTH) == [19, 95, 5, 5]
    assert fam(stats, ref.DURATION) == [19, 2071, 88, 128] and fam(stats, ref.HANDOVER) == [19, 1436, 69, 84]
    assert table[0, :6, ref.COL_ENTRIES].tolist() == [20, 20, 20, 20, 20, 3] and table[0, :7, ref.COL_SEGMENTS].tolist() == [4, 4, 4, 4, 4, 3, 0]
    hist, table, stats = s("n4_cpe1_q3")
    assert lengths("n4_cpe1_q3") == [15, 15, 14, 15] and fam(stats, ref.STRANDED) == [4, 165, 39, 42] and fam(stats, ref.BLOCKS) == [4, 244, 59, 62]
    assert fam(stats, ref.LENGTH) == [55, 55, 1, 1] and fam(stats, ref.DURATION) == [55, 0, 0, 0] and fam(stats, ref.HANDOVER)[0] == 55
    # the stall after the first epoch change: two nodes stay behind, the one segment never completes
    hist, table, stats = s("n4_cpe50_q0")
    assert lengths("n4_cpe50_q0") == [50] * 4 and fam(stats, ref.SEGMENTS) == [4, 4, 1, 1] and fam(stats, ref.LENGTH) == [0, 0, 0, 0]
    assert sorted(cases.case_instances(oracle, "n4_cpe50_q0")[0]["node_epochs"]) == [0, 0, 1, 1] and fam(stats, ref.BEHIND) == [16, 8, 0, 1]
    # the boundaries at the chunk edge: entries 64, 63 and 65 begin a segment
    for name, cpe, at in (("n4_cpe32_q3", 32, 64), ("n4_cpe64_q3", 64, 64), ("n4_cpe21_q3", 21, 63), ("n4_cpe13_q3", 13, 65), ("n4_cpe70_q3", 70, 140)):
        _, table, _ = s(name)
        assert at % cpe == 0 and (table[0, :at // cpe, ref.COL_ENTRIES] == 4 * cpe).all() and table[0, at // cpe, ref.COL_ENTRIES] > 0, name
    assert min(lengths("n4_cpe70_q3")) > 140
    _, table, _ = s("n4_three_epoch_bins")
    assert table[0, :, ref.COL_ENTRIES].tolist() == [20, 20, 63]


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_walk_equals_the_reference_for_every_width(shim, oracle, name):
    kw, max_clock, seeds, epoch_bins = cases.CASES[name]
    model = Model(shim, kw, max_clock, seeds)
    cc, faults, nblocks, _, epochs = model.counts()
    assert not faults.any() and cc.max() <= model.lcap and nblocks.max() <= model.bcap
    instances = cases.case_instances(oracle, name)
    assert nblocks.tolist() == [i["families"][ref.BLOCKS][0] for i in instances] and cc.max(axis=1).tolist() == [i["length"] for i in instances]
    assert epochs.tolist() == [i["node_epochs"] for i in instances]
    lengths, with_chain = sum(i["length"] for i in instances), sum(1 for i in instances if i["length"])
    for width, bins in ((None, None), (7, 5)):
        got = model.same_for_every_width(width=width, bins=bins, epoch_bins=epoch_bins)
        equal(got, cases.expected(instances, max_clock, epoch_bins, width, bins))
        equal(got, model.expected(width, bins, epoch_bins)[0])  # (the read-back of the hand-edit tests gives the same)
        ref.identities(*got, lengths_sum=[lengths], with_chain=[with_chain])
    hist, table, stats = got
    if name == "n4_empty_chain":
        assert not cc.any() and fam(stats, ref.SEGMENTS) == [3, 0, 0, 0] and fam(stats, ref.STRANDED) == [3, 0, 0, 0] and fam(stats, ref.FIRST_ROUND)[0] == 0
    if name == "n65_cpe4_q3":
        assert model.n == 65 and fam(stats, ref.NODE_EPOCH) == [130, 260, 2, 2]
    if name == "n4_cpe1_q3":
        assert fam(stats, ref.SEGMENTS)[1] == lengths
    model.close()


def test_ids_outside_the_pool_end_the_chain_and_its_open_segment(shim):
    for k, value in ((12, 0), (5, None), (0, 0xfffffff0), (64, 0), (70, 0)):
        model = Model(shim, dict(cases.Q3, commands_per_epoch=32), 2500, [1])
        nb = int(model.counts()[2][0])
        r, length = model.chain(0)
        assert length > 71
        _, table0, stats0 = model.same_for_every_width()
        model.log(0, r, k, nb + 1 if value is None else value)
        got = model.same_for_every_width()  # (asserts: no read of an unchecked record, for every width)
        want, _ = model.expected()
        equal(got, want)
        hist, table, stats = got
        # entries 0 .. k - 1 are the chain: k // 32 complete segments of 32 and, unless k is a multiple of 32, an open one
        assert table[0, :, ref.COL_ENTRIES].sum() == k and fam(stats, ref.SEGMENTS)[1] == -(-k // 32) and fam(stats, ref.LENGTH)[:2] == [max(-(-k // 32) - 1, 0), 32 * max(-(-k // 32) - 1, 0)]
        assert fam(stats, ref.BLOCKS) == fam(stats0, ref.BLOCKS) and (table[0, :, ref.COL_BLOCKS] == table0[0, :, ref.COL_BLOCKS]).all()
        if k == 0:
            assert fam(stats, ref.STRANDED) == [1, 0, 0, 0] and not hist.any()  # no tip
        ref.identities(*got, lengths_sum=[k], with_chain=[1 if k else 0])
        model.close()


def test_decreasing_and_huge_epochs_still_give_maximal_runs(shim):
    model = Model(shim, dict(cases.Q3, commands_per_epoch=5), 1000, [1, 2])
    r, length = model.chain(0)
    assert length == 26
    ids = [model.log(0, r, k) for k in range(length)]
    for k in (10, 11, 12):  # epoch 2's first three entries fall back to epoch 0: runs 0 0 0 0 0 | 1 x 5 | 0 0 0 | 2 2 | 3 ...
        model.block(0, ids[k], EPOCH, 0)
    model.block(0, ids[20], EPOCH, 1 << 31)  # ... 3 x 5 | 2^31 | 4 4 4 4 | 5
    for epoch_bins in (64, 3, 512):
        got = model.same_for_every_width(epoch_bins=epoch_bins)
        want, instances = model.expected(epoch_bins=epoch_bins)
        equal(got, want)
        ref.identities(*got, lengths_sum=[26 + model.chain(1)[1]], with_chain=[2])
        hist, table, stats = got
        assert instances[0]["families"][ref.SEGMENTS] == [8] and instances[0]["families"][ref.LENGTH] == [5, 5, 3, 2, 5, 1, 4]
        assert table[0, epoch_bins - 1, ref.COL_SEGMENTS] >= 1 and table[0, epoch_bins - 1, ref.COL_BLOCKS] >= 1  # 2^31: the last row
        if epoch_bins > 8:
            assert table[0, epoch_bins - 1].tolist()[:3] == [1, 1, 1] and table[0, 0, ref.COL_SEGMENTS] == 3
    model.close()


def test_a_faulted_instance_is_skipped(shim, oracle):
    kw, max_clock, seeds, _ = cases.CASES["n4_cpe5_q3"]
    seeds = list(seeds)[:3]
    model = Model(shim, kw, max_clock, seeds)
    instances = cases.oracle_instances(oracle, kw, max_clock, seeds)
    equal(model.same_for_every_width(), cases.expected(instances, max_clock))
    model.L.epm_set_fault(model.h, 1, 1 << 3)
    got = model.same_for_every_width()
    equal(got, cases.expected(instances, max_clock, faults=[0, 8, 0]))
    assert got[2][0, 4 * ref.BLOCKS] == 2 and got[2][0, 4 * ref.NODE_EPOCH] == 8
    model.close()


def test_sums_of_times_past_2_to_the_32_stay_exact(shim):
    """Every second entry of every chain proposed near 2^30 (cpe 1: every entry a segment of duration 0, every pair a boundary): half of
    the handovers are about 2^30, and 8 instances of 14 entries sum past 2^32; with cpe 2 and the first entry of every segment at 0, the
    second near 2^30, so do the durations."""
    for cpe, hot, family, column in ((1, lambda k: k % 2 == 1, ref.HANDOVER, ref.COL_HANDOVER), (2, lambda k: k % 2 == 1, ref.DURATION, ref.COL_DURATION)):
        model = Model(shim, dict(cases.Q3, commands_per_epoch=cpe), 1000, range(1, 9))
        for i in range(model.m):
            r, length = model.chain(i)
            for k in range(length):
                model.block(i, model.log(i, r, k), TIME, (1 << 30) - 1000 + k if hot(k) else 0)
        got = model.same_for_every_width(width=1 << 20, bins=2048)
        want, _ = model.expected(1 << 20, 2048)
        equal(got, want)
        hist, table, stats = got
        print(cpe, fam(stats, family))
        assert fam(stats, family)[1] > 1 << 32 and table[0, :, column].sum() == fam(stats, family)[1] and fam(stats, family)[3] >= (1 << 30) - 1100
        ref.identities(*got)
        model.close()


@pytest.mark.skipif(not shutil.which("g++"), reason="needs g++")
def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The shim with its own main as a program, under the address and undefined-behaviour sanitizers: the walks over an id of 0, one far
    above the pool, falling and huge epochs, times near 2^30 and a fault word read nothing outside the state array."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")
    exe = str(tmp_path / "ep_hostmodel_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-w", "-DEPM_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout[-500:], run.stderr[-3000:])
