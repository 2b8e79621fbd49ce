"""CPU-side checks of the per-instance statistics: the arithmetic the device kernel shares with the host
(csrc/lbft_instance_stats.h and the rule headers it includes), compiled into a g++ shim (tests/instance_stats_host.cpp) that walks an
instance the way lbft_k_ct_instances does -- `chunk` entries side by side in place of the wavefront --, equals the numpy reference
(tests/instance_stats_reference.py: the grouped calls' references with every instance a group of its own) on oracle-run batches and on
logs written by hand: chains that end just before, at and just after a chunk seam, nodes without commits, counts past the capacity,
equal times, a log that differs from the chain, `since` at both ends and between two instants, one node and 32.  The same walk, built
as a stand-alone program under the address and undefined-behaviour sanitizers, runs the hand-written cases once."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import commit_finality_reference as fin_ref
import instance_stats_reference as ref
from support import TESTS, build_shim
from test_commit_finality_host import oracle_case, records_of

ROOT = os.path.dirname(TESTS)
CHUNKS = (4, 8, 64)  # entries side by side in the shim's walk (the kernel: 64)
MAX_CLOCK = 2000


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = build_shim(tmp_path_factory.mktemp("ist_host"), "instance_stats_host.cpp", "libist_host.so", "-Wall", "-Werror")
    vp = C.c_void_p
    L.ist_host.argtypes = [vp] * 9 + [C.c_uint32, C.c_uint64] + [C.c_uint32] * 7 + [vp, C.c_int32, C.c_uint32, vp]
    L.ist_host.restype = C.c_int
    L.ist_workgroups_host.argtypes = [C.c_uint64] * 2
    L.ist_workgroups_host.restype = C.c_uint64
    L.ist_words_host.restype = L.ist_waves_host.restype = C.c_uint32
    return L


def arrays_of(x, faults, group_of):
    logs = np.ascontiguousarray(x["logs"], dtype=np.uint32)
    m, n, lcap = logs.shape
    ct = np.ascontiguousarray(x["ctimes"], dtype=np.int32)
    commits = np.ascontiguousarray(x["commits"], dtype=np.uint32)
    blk_author = np.ascontiguousarray(x["blk_author"], dtype=np.uint32)
    blk_time = np.ascontiguousarray(x["blk_time"], dtype=np.int32)
    startup = np.ascontiguousarray(x["startup"], dtype=np.int32)
    assert ct.shape == logs.shape and commits.shape == startup.shape == (m, n) and blk_author.shape == blk_time.shape and blk_author.shape[0] == m
    faults = np.ascontiguousarray(faults if faults is not None else np.zeros(m), dtype=np.uint32)
    group = np.ascontiguousarray(group_of if group_of is not None else np.zeros(m), dtype=np.uint32)
    return ct, logs, commits, blk_author, blk_time, startup, faults, group


def run_shim(L, x, faults, group_of, groups, since, max_clock, chunk):
    ct, logs, commits, blk_author, blk_time, startup, faults, group = a = arrays_of(x, faults, group_of)
    m, n, lcap = logs.shape
    rights = None if x.get("rights") is None else np.ascontiguousarray(x["rights"], dtype=np.uint32)
    since = None if since is None else np.ascontiguousarray(since, dtype=np.int32)
    total, quorum, _ = fin_ref.thresholds([1] * n if rights is None else rights)
    rows = np.zeros((m, ref.INSTANCE_STATS), dtype=np.uint64)
    rc = L.ist_host(*[v.ctypes.data for v in a], None if rights is None else rights.ctypes.data, x.get("rot", 0), x.get("cpe", 30000), total, quorum,
                    m, n, lcap, blk_author.shape[1] - 1, groups, None if since is None else since.ctypes.data, max_clock, chunk, rows.ctypes.data)
    assert rc == 0, rc
    return rows.reshape(m, ref.FAMILIES, 4)


def reference(x, faults, group_of, since, max_clock, histories=None):
    """The reference on what a read-back of the state `x` would give: -1 past the clamped counts, records from the logs and the pool."""
    m, n, lcap = x["logs"].shape
    ct = np.asarray(x["ctimes"]).astype(np.int64).copy()
    ct[np.arange(lcap)[None, None, :] >= np.minimum(np.asarray(x["commits"]).astype(np.int64), lcap)[:, :, None]] = -1
    res = ref.Readbacks(ct, records_of(x, faults) if histories is None else histories, x["commits"], x["startup"], faults)
    return ref.instance_stats(res, max_clock, since, group_of, x.get("rights"), x.get("rot", 0), x.get("cpe", 30000), log_capacity=lcap)


def compare(L, x, faults=None, group_of=None, groups=1, since=None, max_clock=MAX_CLOCK, histories=None, families=slice(None)):
    want = reference(x, faults, group_of, since, max_clock, histories)
    for chunk in CHUNKS:
        got = run_shim(L, x, faults, group_of, groups, since, max_clock, chunk)
        assert (got[:, families] == want[:, families]).all(), (chunk, np.argwhere(got != want)[:8], got[got != want][:8], want[got != want][:8])
    return want


# ---- logs written by hand ----
def chain(n, commits, lcap=None, tie=3, per_node=1, rights=None, rot=0, cpe=30000):
    """One instance whose nodes hold prefixes of one chain: block k + 1 at entry k, authored by node k % n at its clock 10 k (startup j % 4),
    committed by node j at 30 + 10 * (k // tie * tie) + per_node * j -- `tie` consecutive entries share a commit instant, also across a
    chunk seam; per_node = 0: equal commit times across the nodes.  Past a node's count the buffers hold garbage."""
    commits = np.asarray(commits, dtype=np.int64)
    lcap = int(lcap or max(int(commits.max()), 1))
    k = np.arange(lcap)
    x = dict(logs=np.tile((k + 1).astype(np.uint32), (1, n, 1)), commits=commits[None].astype(np.uint32),
             blk_author=np.r_[0, k % n].astype(np.uint32)[None], blk_time=np.r_[0, 10 * k].astype(np.int32)[None],
             startup=(np.arange(n) % 4).astype(np.int32)[None], rights=rights, rot=rot, cpe=cpe)
    ct = (30 + 10 * (k // tie * tie))[None, :] + per_node * np.arange(n)[:, None]
    past = k[None, :] >= np.minimum(commits, lcap)[:, None]
    x["ctimes"] = np.where(past, 7, ct).astype(np.int32)[None]
    x["logs"][0][past] = 0xdeadbeef
    return x


def stack(cases):
    """Instances of equal n side by side, padded to the widest log and the largest pool."""
    lcap = max(c["logs"].shape[2] for c in cases)
    blocks = max(c["blk_author"].shape[1] for c in cases)

    def pad(a, width, fill):
        out = np.full(a.shape[:-1] + (width,), fill, dtype=a.dtype)
        out[..., :a.shape[-1]] = a
        return out
    x = dict(cases[0])
    for key, width, fill in (("logs", lcap, 0), ("ctimes", lcap, -1), ("blk_author", blocks, 0), ("blk_time", blocks, 0)):
        x[key] = np.concatenate([pad(c[key], width, fill) for c in cases])
    for key in ("commits", "startup"):
        x[key] = np.concatenate([c[key] for c in cases])
    return x


def seams():
    """Chains of 63 / 64 / 65 / 129 entries with rows of unequal length, a node that ends on the seam, a node with no commit, an
    instance without any, equal times across the nodes, and a faulted instance full of holes; two groups with their own `since`."""
    cases = [chain(4, [L, L - 1, max(L - 3, 0), L]) for L in (63, 64, 65, 129)]
    cases += [chain(4, [65, 0, 64, 1]), chain(4, [0, 0, 0, 0]), chain(4, [129, 129, 129, 129], per_node=0)]
    holes = chain(4, [40, 40, 40, 40])
    holes["ctimes"][0, :, 5::7] = -1
    x = stack(cases + [holes])
    faults = np.array([0] * len(cases) + [1 << 3], dtype=np.uint32)
    group_of = np.array([0, 1, 0, 1, 1, 0, 1, 0], dtype=np.uint32)
    return x, faults, group_of


def differing():
    """Node 1's entries 5 and 64 are blocks of its own (ids L + 1, L + 2; proposed earlier than the chain's): its latency there is taken
    after its own block's proposal time, the finality after the chain's."""
    L, n = 66, 4
    x = chain(n, [L, L, L, 2])
    x["blk_author"] = np.c_[x["blk_author"], [[3, 2]]].astype(np.uint32)
    x["blk_time"] = np.c_[x["blk_time"], [[11, 333]]].astype(np.int32)
    x["logs"][0, 1, 5], x["logs"][0, 1, 64] = L + 1, L + 2
    return x


def hand_cases():
    """(name, x, faults, group_of, groups, since) of every hand-written case."""
    x, faults, group_of = seams()
    out = [("seams", x, faults, group_of, 2, [0, 675]), ("seams at the horizon", x, faults, group_of, 2, [MAX_CLOCK, 0]),
           ("seams, no since", x, faults, group_of, 2, None)]
    out.append(("counts past the capacity", chain(4, [70, 4000000000, 3, 66], lcap=66), None, None, 1, [40]))
    out.append(("differing", differing(), None, None, 1, [45]))
    out.append(("one node", chain(1, [67]), None, None, 1, [100]))
    out.append(("32 nodes", chain(32, list(range(66, 34, -1)), rights=list(range(1, 33)), rot=31, cpe=1), None, None, 1, [331]))
    out.append(("weighted", chain(5, [70, 70, 69, 0, 70], rights=[5, 1, 1, 1, 1], rot=1, cpe=3), None, None, 1, [31]))
    return out


def test_shim_equals_the_reference_on_hand_written_logs(shim):
    assert shim.ist_words_host() == ref.INSTANCE_STATS
    for name, x, faults, group_of, groups, since in hand_cases():
        want = compare(shim, x, faults, group_of, groups, since)
        if faults is not None:
            assert not want[faults != 0].any(), name
    x, faults, group_of = seams()
    want = compare(shim, x, faults, group_of, 2, [0, 675])
    S, F = ref.SAMPLES, ref
    assert want[0, F.LATENCY, S] == 63 + 62 + 60 + 63 and want[3, F.FIN_FIRST, S] == 129 and want[5, F.LATENCY, S] == 0
    assert want[5, F.TAIL].tolist() == [4, 4 * MAX_CLOCK, MAX_CLOCK, MAX_CLOCK] and want[5, F.OPEN].tolist() == [1, 0, 0, 0]  # no commit at all
    assert want[4, F.LONGEST, ref.MAX] == MAX_CLOCK and want[4, F.FIRST, S] == 0  # node 1 never commits; the last instant is 660 + j < since = 675
    assert (want[6, F.SPREAD, 1:] == 0).all() and want[6, F.SPREAD, S] == 129  # equal times across the nodes: no spread
    # a tie that spans the seam (entries 63, 64 and 65 share an instant) closes no gap: 129 entries are 43 instants
    assert want[6, F.GAPS].tolist() == [4 * 42, 4 * 42 * 30, 30, 30]
    over = compare(shim, chain(4, [70, 4000000000, 3, 66], lcap=66), since=[40])
    assert over[0, F.LATENCY, S] == 66 + 66 + 3 + 66 and over[0, F.FIN_FIRST, S] == 66  # counts past the capacity are the capacity
    # since between two instants: 675 lies between 660 + j and 690 + j
    first = compare(shim, chain(4, [129] * 4), since=[675])[0, F.FIRST]
    assert first.tolist() == [4, 15 + 16 + 17 + 18, 15, 18]
    first = compare(shim, chain(4, [129] * 4), since=[MAX_CLOCK])[0, F.FIRST]
    assert first.tolist() == [0, 0, 0, 0]  # nothing at or after the horizon


def test_latency_is_taken_on_the_nodes_own_log(shim):
    x = differing()
    own = compare(shim, x, since=[45])
    x["logs"][0, 1, 5], x["logs"][0, 1, 64] = 6, 65  # the same instance with node 1 on the chain
    agree = compare(shim, x, since=[45])
    # entry 5: the chain's block 6 is proposed at 50 + startup[1] = 51, node 1's own at 11 + startup[3] = 14; entry 64: 640 against 333 + 2
    assert own[0, ref.LATENCY, ref.SUM] - agree[0, ref.LATENCY, ref.SUM] == (51 - 14) + (640 - 335)
    assert (own[0, 1:] == agree[0, 1:]).all()  # the timeline and the finality do not look at the log of node 1


def test_a_hole_inside_a_row(shim):
    """An entry below the count that was never recorded is no commit: no latency sample, no committer, and for the timeline no instant
    -- the entry after it is looked at as the row's first.  (The numpy reference of the stalls takes no holes; the stall families of
    this row are written by hand.)  Row [10, -1, 20, 20, 50] to clock 100: leading intervals 10 and 20, one gap of 30, tail 50."""
    x = chain(1, [5])
    x["ctimes"][0, 0] = [10, -1, 20, 20, 50]
    x["blk_time"][0] = [0, 0, 1, 2, 3, 4]
    for chunk in (1, 2, 4, 64):
        got = run_shim(shim, x, None, None, 1, [15], 100, chunk)[0]
        assert got[ref.GAPS].tolist() == [1, 30, 30, 30] and got[ref.FIRST].tolist() == [1, 5, 5, 5], chunk
        assert got[ref.TAIL].tolist() == [1, 50, 50, 50] and got[ref.LONGEST].tolist() == [1, 50, 50, 50]
        assert got[ref.LATENCY].tolist() == [4, 10 + 18 + 17 + 46, 10, 46] and got[ref.OPEN].tolist() == [1, 0, 0, 0]
        assert got[ref.FIN_QUORUM].tolist() == got[ref.FIN_ALL].tolist() == got[ref.LATENCY].tolist() and got[ref.SPREAD].tolist() == [4, 0, 0, 0]


# ---- oracle-run batches ----
def test_shim_equals_the_reference_on_oracle_runs(shim, oracle):
    n, seeds, max_clock = 4, range(1, 17), 300
    x, histories = oracle_case(oracle, oracle.make_config(num_nodes=n), seeds, max_clock)
    want = compare(shim, x, since=[150], max_clock=max_clock, histories=histories)
    assert (want[:, ref.LATENCY, ref.SAMPLES] == x["commits"].sum(axis=1)).all() and (want[:, ref.OPEN, ref.SAMPLES] == 1).all()
    assert (want[:, ref.FIRST, ref.SAMPLES] == n).all() and (want[:, ref.GAPS, ref.SAMPLES] > 0).all()


def test_shim_equals_the_reference_on_weighted_rotating_oracle_runs(shim, oracle):
    n, rights, cpe = 7, [3, 1, 1, 2, 1, 1, 4], 3
    cfg = oracle.make_config(num_nodes=n, voting_rights=rights, commands_per_epoch=cpe, rights_rotation=2, quirks=3)
    x, histories = oracle_case(oracle, cfg, range(1, 9), 600, rights=rights, rot=2, cpe=cpe)
    want = compare(shim, x, since=[300], max_clock=600, histories=histories)
    assert x["commits"].max() > 2 * cpe and (want[:, ref.FIN_QUORUM, ref.SAMPLES] > 0).all()
    unit = reference(dict(x, rights=None, rot=0), None, None, [300], 600, histories)
    assert (unit[:, ref.FIN_QUORUM] != want[:, ref.FIN_QUORUM]).any()  # the rights matter on this data


# ---- the grid rule ----
def test_grid_rule_of_the_launcher(shim):
    """gridDim.x = min(max(1, 1024 / groups), ceil(largest group / 4)) workgroups of 4 wavefronts: a wavefront takes a second instance
    exactly when the largest group has more than 4 * max(1, 1024 / groups) instances -- a plain batch of 4097 is the smallest."""
    src = open(os.path.join(ROOT, "librabft_simulator_amd", "csrc", "lbft_instance_stats.h")).read()
    assert "#define IST_WORKGROUPS 1024u" in src and "#define IST_WAVES 4u" in src and shim.ist_waves_host() == 4
    for groups, max_group, want in ((1, 1, 1), (1, 4, 1), (1, 5, 2), (1, 4096, 1024), (1, 4097, 1024), (1, 65536, 1024), (64, 1024, 16), (256, 38, 4),
                                    (256, 1, 1), (256, 1 << 24, 4), (2048, 9, 1)):
        assert shim.ist_workgroups_host(groups, max_group) == want, (groups, max_group)
    strides = lambda groups, m: shim.ist_workgroups_host(groups, m) * 4 < m  # noqa: E731
    assert not any(strides(1, m) for m in range(1, 4097)) and strides(1, 4097)
    assert not strides(256, 16) and strides(256, 17) and not strides(3, 4 * 341) and strides(3, 4 * 341 + 1)


# ---- the same walk under the sanitizers ----
def test_stand_alone_walk_under_the_sanitizers(shim, tmp_path):
    exe = str(tmp_path / "ist_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DIST_HOST_MAIN", os.path.join(TESTS, "instance_stats_host.cpp"), "-o", exe])
    cases, text = [], []
    for name, x, faults, group_of, groups, since in hand_cases():
        for chunk in (8, 64):
            a = arrays_of(x, faults, group_of)
            m, n, lcap = a[1].shape
            rights = x.get("rights")
            total, quorum, _ = fin_ref.thresholds([1] * n if rights is None else rights)
            head = [m, n, lcap, a[3].shape[1] - 1, groups, x.get("rot", 0), x.get("cpe", 30000), total, quorum, MAX_CLOCK, chunk,
                    int(rights is not None), int(since is not None)]
            body = [v.reshape(-1).astype(np.int64) for v in a] + [np.asarray(rights or [], dtype=np.int64), np.asarray(since or [], dtype=np.int64)]
            text.append(" ".join(str(v) for v in head) + "\n" + "\n".join(" ".join(str(int(v)) for v in part) for part in body))
            cases.append((name, chunk, reference(x, faults, group_of, since, MAX_CLOCK)))
    out = subprocess.run([exe], input="%d\n%s\n" % (len(cases), "\n".join(text)), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    for (name, chunk, want), line in zip(cases, lines):
        words = [int(v) for v in line.split()]
        assert words[0] == 0 and words[1:] == want.reshape(-1).tolist(), (name, chunk)
