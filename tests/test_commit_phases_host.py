"""CPU-side checks of the commit phases: the arithmetic the device kernel shares with the host (csrc/lbft_commit_phases.h and the rule
headers of the two calls it splits), compiled into a g++ shim (tests/commit_phases_host.cpp) that walks an instance the way
lbft_k_ct_phases does -- `chunk` entries side by side in place of the wavefront, the virtual histograms in passes of `lds_bins` bins --,
equals the numpy reference written from the definitions (tests/commit_phases_reference.py) on logs written by hand and on drawn data
that no run produces: an edge between two entries of one chunk and edges on the chunk seams, equal edges, edges 0 and max_clock + 1, a
proposal time that goes back, a node whose log differs from the chain's, commit times that were never recorded, a faulted instance
between clean ones, an empty group, weighted rights that rotate inside a phase.  With one phase the result is the latency histogram's
and the finality's; for any edges the phases add up to it.  The same walk, built as a stand-alone program under the address and
undefined-behaviour sanitizers, runs the hand-written cases once."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import commit_finality_reference as fin_ref
import commit_phases_reference as ref
import strided_shapes as S
from support import TESTS, build_shim
from test_commit_finality_host import draw, records_of
from test_instance_stats_host import arrays_of, chain, differing, stack

CHUNKS = (4, 8, 64)  # entries side by side in the shim's walk (the kernel: 64)
MAX_CLOCK = 2000
SEAMS = [15, 40, 80, 640]  # chain(): entry k is proposed at 10 k + (k % n) % 4 -- 15 parts entries 1 | 2, the others 3 | 4, 7 | 8 and 63 | 64


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = build_shim(tmp_path_factory.mktemp("cph_host"), "commit_phases_host.cpp", "libcph_host.so", "-Wall", "-Werror")
    vp = C.c_void_p
    L.cph_host.argtypes = [vp] * 9 + [C.c_uint32, C.c_uint64] + [C.c_uint32] * 7 + [vp] + [C.c_uint32] * 5 + [vp] * 3
    L.cph_host.restype = C.c_int
    L.cph_phase_host.argtypes = [vp, C.c_uint32, C.c_int32]
    L.cph_phase_host.restype = C.c_uint32
    L.cph_workgroups_host.argtypes = [C.c_uint64] * 6
    L.cph_workgroups_host.restype = C.c_uint64
    L.cph_stats_host.restype = C.c_uint32
    return L


def run_shim(L, x, faults, group_of, groups, edges, width, bins, lds_bins, chunk):
    a = arrays_of(x, faults, group_of)
    m, n, lcap = a[1].shape
    rights = None if x.get("rights") is None else np.ascontiguousarray(x["rights"], dtype=np.uint32)
    total, quorum, _ = fin_ref.thresholds([1] * n if rights is None else rights)
    e = np.ascontiguousarray(ref.edges_per_group(edges, groups), dtype=np.int32)
    phases = e.shape[1] + 1
    lat = np.zeros((groups, phases, bins), dtype=np.uint64)
    fin = np.zeros((groups, phases, bins), dtype=np.uint64)
    stats = np.zeros((groups, phases, ref.FAMILIES, 4), dtype=np.uint64)
    rc = L.cph_host(*[v.ctypes.data for v in a], None if rights is None else rights.ctypes.data, x.get("rot", 0), x.get("cpe", 30000), total, quorum,
                    m, n, lcap, a[3].shape[1] - 1, groups, e.ctypes.data if phases > 1 else None, phases, width, bins, lds_bins, chunk,
                    lat.ctypes.data, fin.ctypes.data, stats.ctypes.data)
    assert rc == 0, rc
    return lat, fin, stats


def families(x, faults, group_of, groups, edges, histories=None):
    histories = records_of(x, faults) if histories is None else histories
    return ref.samples(x["ctimes"], x["commits"], histories, x["startup"], faults, x.get("rights"), x.get("rot", 0), x.get("cpe", 30000), group_of,
                       groups, edges, log_capacity=x["logs"].shape[2])


def compare(L, x, edges, faults=None, group_of=None, groups=1, binnings=((1, 700, ref.LDS_BINS), (7, 5, ref.LDS_BINS), (1, 700, 64))):
    """The shim equals the reference for every chunk and binning (width, bins, bins per pass); one phase is the pooled calls' result
    and the phases add up to it.  -> (the families, the last binning's arrays)."""
    fam = families(x, faults, group_of, groups, edges)
    one = families(x, faults, group_of, groups, [])
    for width, bins, lds_bins in binnings:
        want = ref.bin_phases(fam, width, bins, MAX_CLOCK)
        whole = ref.bin_phases(one, width, bins, MAX_CLOCK)
        for chunk in CHUNKS:
            got = run_shim(L, x, faults, group_of, groups, edges, width, bins, lds_bins, chunk)
            for name, a, b in zip(("latency_hist", "finality_hist", "stats"), got, want):
                assert (a == b).all(), (name, chunk, width, bins, lds_bins, np.argwhere(a != b)[:8], a[a != b][:8], b[a != b][:8])
            pooled = run_shim(L, x, faults, group_of, groups, [], width, bins, lds_bins, chunk)
            for a, b, c in zip(pooled, whole, ref.pooled(*got)):
                assert (a == b).all() and (a[:, 0] == c).all(), (chunk, width, bins)
    lat, fin, stats = want
    assert (lat.sum(axis=2) == stats[:, :, ref.LATENCY, ref.SAMPLES]).all() and (fin.sum(axis=2) == stats[:, :, ref.QUORUM, ref.SAMPLES]).all()
    return fam, want


# ---- one phase is the two pooled calls ----
def test_one_phase_is_the_latency_histogram_and_the_finality(shim):
    """The reference with no edge against the references of the calls it pools: commit_finality_reference for families 1 to 5 and the
    quorum histogram, the latency written out here (every recorded entry of every node, after its own record's proposal time)."""
    assert shim.cph_stats_host() == ref.PHASE_STATS == 4 * ref.FAMILIES
    x = differing()
    fam, (lat, fin, stats) = compare(shim, x, [], binnings=((1, 700, 64), (7, 5, ref.LDS_BINS)))
    f_fam, fc = fin_ref.samples(x["ctimes"], x["commits"], records_of(x), x["startup"], None, None, 0, 30000, None, 1, log_capacity=x["logs"].shape[2])
    want_fin, _, _, want_stats = fin_ref.bin_finality(f_fam, fc, 7, 5)
    assert (fin[:, 0] == want_fin).all() and (stats[:, 0, 1:].reshape(1, 20) == want_stats[:, :20]).all()
    hist = records_of(x)
    latency = [int(x["ctimes"][0, j, k]) - int(x["startup"][0, hist[0, j, k]["proposer"]]) - int(hist[0, j, k]["time"])
               for j in range(4) for k in range(min(int(x["commits"][0, j]), 66))]
    assert stats[0, 0, ref.LATENCY].tolist() == [len(latency), sum(latency), min(latency), max(latency)]
    assert (lat[0, 0] == np.bincount(np.minimum(np.array(latency) // 7, 4), minlength=5)).all()


# ---- the phase of a time ----
def test_phase_lookup(shim):
    def phase(edges, t):
        e = np.array(edges, dtype=np.int32)
        got = shim.cph_phase_host(e.ctypes.data if len(edges) else None, len(edges), t)
        assert got == ref.phase_of(edges, t), (edges, t)
        return got
    assert [phase([], t) for t in (0, 5, 2 ** 31 - 3)] == [0, 0, 0]
    assert [phase([300, 600], t) for t in (0, 299, 300, 599, 600, 2000)] == [0, 0, 1, 1, 2, 2]  # phase p covers [e_{p-1}, e_p)
    assert [phase([0, 10], t) for t in (0, 9, 10)] == [1, 1, 2]  # an edge 0 leaves phase 0 empty
    assert [phase([5, 5, 9], t) for t in (4, 5, 8, 9)] == [0, 2, 2, 3]  # equal edges: phase 1 is empty
    assert [phase([10, MAX_CLOCK + 1], t) for t in (10, MAX_CLOCK)] == [1, 1]  # an edge max_clock + 1 is never reached
    assert [phase([1, 2, 3, 4, 5, 6, 7], t) for t in (0, 4, 7, 8)] == [0, 4, 7, 7]
    assert phase([2 ** 31 - 2], 2 ** 31 - 3) == 0 and phase([2 ** 31 - 3], 2 ** 31 - 3) == 1  # the largest clock and the largest edge
    assert phase([100], -5) == 0  # (a time below every edge)


# ---- logs written by hand ----
def inversion():
    """Entry 6's block is proposed at 12 + startup, before entries 2 to 5: its phase is lower than its predecessor's."""
    x = chain(4, [70, 70, 70, 70])
    x["blk_time"][0, 7] = 12
    return x


def holes():
    x = chain(4, [40, 40, 40, 40])
    x["ctimes"][0, :, 5::7] = -1  # never recorded: no latency sample, no committer
    x["ctimes"][0, 2, 0:9] = -1
    return x


def mixed_groups():
    """Three groups, the middle one empty; a faulted instance (full of garbage) between clean ones of group 2."""
    broken = chain(4, [66, 66, 66, 66])
    broken["logs"][:] = 0xdeadbeef
    x = stack([chain(4, [129, 128, 126, 129]), chain(4, [65, 0, 64, 1]), broken, chain(4, [70, 70, 69, 70])])
    return x, np.array([0, 1 << 3, 1 << 3, 0], dtype=np.uint32), np.array([0, 2, 2, 2], dtype=np.uint32)


def hand_cases():
    """(name, x, edges, faults, group_of, groups) of every hand-written case."""
    long = chain(4, [129, 128, 126, 129])
    x, faults, group_of = mixed_groups()
    out = [("an edge inside a chunk, edges on the seams", long, SEAMS, None, None, 1),
           ("equal edges", long, [40, 40, 640, 640, 640], None, None, 1),
           ("edges 0 and max_clock + 1", long, [0, 500, MAX_CLOCK + 1], None, None, 1),
           ("both ends twice", long, [0, 0, MAX_CLOCK + 1, MAX_CLOCK + 1], None, None, 1),
           ("eight phases", long, [11, 22, 33, 33, 640, 641, 1280], None, None, 1),
           ("inversion", inversion(), [15, 40, 80], None, None, 1),
           ("differing", differing(), SEAMS, None, None, 1),
           ("holes", holes(), [15, 80], None, None, 1),
           ("groups", x, [[40, 640], [0, 0], [15, 80]], faults, group_of, 3),
           ("one node", chain(1, [67]), [80, 640], None, None, 1),
           ("32 nodes", chain(32, list(range(66, 34, -1)), rights=list(range(1, 33)), rot=31, cpe=1), [80, 640], None, None, 1),
           ("weighted", chain(5, [70, 70, 69, 0, 70], rights=[5, 1, 1, 1, 1], rot=1, cpe=3), [100, 400], None, None, 1)]
    return out


def test_shim_equals_the_reference_on_hand_written_logs(shim):
    got = {}
    for name, x, edges, faults, group_of, groups in hand_cases():
        got[name] = compare(shim, x, edges, faults, group_of, groups)
    S_, L_ = ref.SAMPLES, ref.LATENCY
    fam, (lat, fin, stats) = got["an edge inside a chunk, edges on the seams"]
    # entries 0..1 | 2..3 | 4..7 | 8..63 | 64..128 of a chain of 129; the nodes hold 129, 128, 126 and 129 entries
    assert stats[0, :, ref.FIRST, S_].tolist() == [2, 2, 4, 56, 65] and stats[0, :, L_, S_].tolist() == [8, 8, 16, 224, 65 + 64 + 62 + 65]
    fam, (lat, fin, stats) = got["equal edges"]
    assert stats[0, :, ref.FIRST, S_].tolist() == [4, 0, 60, 0, 0, 65] and not stats[0, [1, 3, 4]].any() and not lat[0, [1, 3, 4]].any()
    fam, (lat, fin, stats) = got["edges 0 and max_clock + 1"]
    assert stats[0, :, ref.FIRST, S_].tolist() == [0, 50, 79, 0]  # phase 0 is empty, the last edge is never reached
    assert got["both ends twice"][1][2][0, :, ref.FIRST, S_].tolist() == [0, 0, 129, 0, 0]
    assert (got["eight phases"][1][2][0, :, ref.FIRST, S_] > 0).tolist() == [True, True, True, False, True, True, True, True]
    # the inversion: entry 6 (proposed at 12 + startup 2) is in phase 0 between entries of phase 2
    fam, (lat, fin, stats) = got["inversion"]
    assert stats[0, :, ref.FIRST, S_].tolist() == [3, 2, 3, 62] and stats[0, 0, L_, S_] == 12
    # weighted rights rotate every 3 entries: phase 1 (entries 10 .. 39) holds ten epochs
    fam, (lat, fin, stats) = got["weighted"]
    assert stats[0, :, ref.FIRST, S_].tolist() == [10, 30, 30]
    x = chain(5, [70, 70, 69, 0, 70], rights=[5, 1, 1, 1, 1], rot=0, cpe=3)
    assert (ref.bin_phases(families(x, None, None, 1, [100, 400]), 1, 700)[2][0, 1, ref.QUORUM] != stats[0, 1, ref.QUORUM]).any()  # the rotation matters
    # a faulted instance gives nothing, the empty group stays zero
    fam, (lat, fin, stats) = got["groups"]
    assert not stats[1].any() and not lat[1].any() and not fin[1].any()
    assert stats[2, :, ref.FIRST, S_].sum() == 70 and stats[0, :, ref.FIRST, S_].tolist() == [4, 60, 65]
    # holes: 40 entries, rows of 35 recorded entries (k = 5, 12, 19, 26, 33 missing), node 2 also without entries 0 .. 8 (8 more)
    fam, (lat, fin, stats) = got["holes"]
    assert stats[0, :, L_, S_].sum() == 4 * 35 - 8 and stats[0, :, ref.ALL, S_].sum() == 40 - 5 - 8


def test_latency_phase_comes_from_the_nodes_own_block(shim):
    """differing(): node 1's entries 5 and 64 are blocks of its own, proposed at 11 + 3 = 14 (phase 0 of SEAMS) and 333 + 2 = 335 (phase
    3) where the chain's are proposed at 51 (phase 2) and 640 (phase 4): the latency samples move, the finality stays."""
    own = compare(shim, differing(), SEAMS)[1][2]
    x = differing()
    x["logs"][0, 1, 5], x["logs"][0, 1, 64] = 6, 65  # the same instance with node 1 on the chain
    agree = compare(shim, x, SEAMS)[1][2]
    moved = own[0, :, ref.LATENCY, ref.SAMPLES].astype(np.int64) - agree[0, :, ref.LATENCY, ref.SAMPLES].astype(np.int64)
    assert moved.tolist() == [1, 0, -1, 1, -1]
    assert (own[0, :, 1:] == agree[0, :, 1:]).all()


def test_shim_equals_the_reference_on_drawn_data(shim):
    """Logs that are permutations of the pool per node (most entries differ from the chain's), proposal times in any order."""
    for n, rights, rot, cpe in ((4, None, 0, 30000), (7, [3, 1, 1, 2, 1, 1, 4], 2, 5), (32, list(range(1, 33)), 31, 1)):
        rng = np.random.default_rng(2000 + n)
        x = draw(rng, 7, n, 70 if n < 32 else 66, rights, rot, cpe)
        faults = np.array([0, 0, 1 << 3, 0, 0, 0, 0], dtype=np.uint32)
        x["logs"][2] = 0xdeadbeef
        group_of = np.array([0, 1, 1, 1, 0, 3, 3], dtype=np.uint32)
        edges = [[10, 25, 25, 45], [0, 20, 30, 61], [1, 2, 3, 4], [30, 30, 30, MAX_CLOCK + 1]]
        fam, (lat, fin, stats) = compare(shim, x, edges, faults, group_of, 4, ((1, 600, ref.LDS_BINS), (3, 9, 16)))
        assert (stats[0, :, ref.LATENCY, ref.SAMPLES] > 0).sum() >= 3 and not stats[2].any()


# ---- the grid rule ----
def test_grid_rule_of_the_launcher(shim):
    """gridDim.x = gs_workgroups(1024, groups, ceil(largest group / 4), largest group x n x lcap): the strided layouts of
    tests/strided_shapes.py give a second and a third trip with it."""
    src = open(os.path.join(os.path.dirname(TESTS), "librabft_simulator_amd", "csrc", "lbft_commit_times.hip")).read()
    assert "#define LBFT_PH_WORKGROUPS 1024u" in src and "#define LBFT_PH_BLOCK 256" in src and "#define LBFT_PH_LDS_BINS %d" % ref.LDS_BINS in src
    for groups, max_group, n, lcap in ((1, 1, 4, 100), (1, 4102, 4, 2048), (256, 38, 4, 2048), (256, 1 << 20, 32, 4096), (3, 9000, 7, 512)):
        want = S.grid_x(groups, max_group, n * lcap)
        assert shim.cph_workgroups_host(S.TARGET, groups, max_group, S.WAVES, n, lcap) == want, (groups, max_group)
    gx = shim.cph_workgroups_host(S.TARGET, S.GROUPS, 38, S.WAVES, 4, 2048)
    assert gx == 4 and max(S.trips(38, gx)) == 3 and max(S.trips(17, gx)) == 2
    gx = shim.cph_workgroups_host(S.TARGET, 1, S.PLAIN["m"], S.WAVES, 4, 2048)
    assert gx == 1024 and sorted(set(S.trips(S.PLAIN["m"], gx))) == [1, 2]


# ---- the same walk under the sanitizers ----
def test_stand_alone_walk_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "cph_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DCPH_HOST_MAIN", os.path.join(TESTS, "commit_phases_host.cpp"), "-o", exe])
    cases, text = [], []
    for name, x, edges, faults, group_of, groups in hand_cases():
        for chunk, (width, bins, lds_bins) in ((8, (1, 700, 64)), (64, (7, 5, ref.LDS_BINS))):
            a = arrays_of(x, faults, group_of)
            m, n, lcap = a[1].shape
            rights = x.get("rights")
            total, quorum, _ = fin_ref.thresholds([1] * n if rights is None else rights)
            e = ref.edges_per_group(edges, groups)
            head = [m, n, lcap, a[3].shape[1] - 1, groups, x.get("rot", 0), x.get("cpe", 30000), total, quorum, e.shape[1] + 1, width, bins, lds_bins, chunk,
                    int(rights is not None)]
            body = [v.reshape(-1).astype(np.int64) for v in a] + [np.asarray(rights or [], dtype=np.int64), e.reshape(-1)]
            text.append(" ".join(str(v) for v in head) + "\n" + "\n".join(" ".join(str(int(v)) for v in part) for part in body))
            cases.append((name, chunk, ref.bin_phases(families(x, faults, group_of, groups, edges), width, bins, MAX_CLOCK)))
    out = subprocess.run([exe], input="%d\n%s\n" % (len(cases), "\n".join(text)), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    for (name, chunk, want), line in zip(cases, lines):
        words = [int(v) for v in line.split()]
        assert words[0] == 0 and words[1:] == np.concatenate([w.reshape(-1) for w in want]).tolist(), (name, chunk)
