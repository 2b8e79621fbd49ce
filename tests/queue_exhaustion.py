"""What the calendar queue's exhausted-pool tests share (tests/test_queue_exhaustion_host.py on the CPU, tests/test_queue_exhaustion_gpu.py on the
device): the cases, the text protocol of the fenced stand-alone host program (tests/queue_exhaustion_host.cpp), and the comparison with the oracle.

The calendar's pool holds ceil(qcap / 31) + max(256, qcap / 32) chunks of 31 entries and every non-empty (time, kind) bucket pins at least one, so
a delay spread of hundreds of ticks uses the pool up long before the queue holds qcap entries.  The contract is the one of every other capacity:
F_QUEUE_OVERFLOW on that instance and nothing else -- no access outside the instance's rows, the neighbours exact."""
import os
import subprocess

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(TESTS, "queue_exhaustion_host.cpp")

F_QUEUE, F_SNAP, F_BLOCK, F_LOG, F_NOT_SUCCESSOR, F_EPOCH = 1, 2, 4, 8, 1 << 7, 1 << 12
# What a run that dropped events for want of a capacity may raise: the capacities' own bits.  The other bits of lbft_core.h's fault word say that
# the state is not a state of the protocol any more (a commit of an unknown state, an internal error, a runaway step count ...): garbage.
CAPACITY_BITS = F_QUEUE | F_SNAP | F_BLOCK | F_LOG | F_EPOCH
RESULT_KEYS = ("commit_counts", "active_rounds", "last_states", "histories")
STATS = ("empty_bucket", "full_tail", "bulk_1", "bulk_2", "bulk_3", "short_stack")  # the program's counters, LBFT_POOL_STAT 0..5 of lbft_core.h

CONFIG_FIELDS = ("num_nodes", "delay_model", "mean", "variance", "uniform_lo", "uniform_hi", "commands_per_epoch", "quirks", "equivocate_every",
                 "drop_per_million", "partition_size", "partition_start", "partition_end")
CONFIG_DEFAULTS = dict(num_nodes=3, delay_model=0, mean=10.0, variance=4.0, uniform_lo=5, uniform_hi=15, commands_per_epoch=30000, quirks=0,
                       equivocate_every=0, drop_per_million=0, partition_size=0, partition_start=0, partition_end=0)
CAPS_FIELDS = ("qcap", "scap", "bcap", "lcap", "ql", "qheap", "qcal", "ring", "ring_topup", "tw", "state_fill")


def uniform(n, lo, hi, **kw):
    return dict(num_nodes=n, delay_model=1, uniform_lo=lo, uniform_hi=hi, **kw)


def caps_of(qcap, scap, ring=0, bcap=512, lcap=512, **kw):
    return dict(qcap=qcap, scap=scap, bcap=bcap, lcap=lcap, ql=0, qheap=1, qcal=1, ring=ring, **kw)


# (a) The cases that crashed, or returned garbage fault bits, before the pool's exhaustion dropped the event: (configuration, max_clock, capacities),
# seeds 1..3.  The last one is the sizing gap that remains: the binary heap runs it clean with the same queue_capacity.
REGRESSION = {
    "n20_u0_250": (uniform(20, 0, 250), 400, caps_of(3200, 320)),
    "n20_u0_250_exchange": (uniform(20, 0, 250, quirks=1), 400, caps_of(3200, 2720)),
    "n20_u0_300": (uniform(20, 0, 300), 1000, caps_of(3200, 320)),
    "n40_u0_300_coop512": (uniform(40, 0, 300), 1000, caps_of(12800, 640, ring=512)),
    "n20_u20_120_heap_is_clean": (uniform(20, 20, 120), 3000, caps_of(3200, 320)),
}
REGRESSION_SEEDS = (1, 2, 3)


def case_line(kw, max_clock, caps, seeds, history_cap):
    """One case as the program reads it.  `kw` may also hold voting_rights (one per node) and rights_rotation: they follow the seeds as the
    line's optional tail; a line without it means unit rights and no rotation, as before."""
    kw = dict(kw)
    rights, rotation = kw.pop("voting_rights", None), kw.pop("rights_rotation", 0)
    cfg = dict(CONFIG_DEFAULTS, **kw)
    assert set(cfg) == set(CONFIG_FIELDS) and set(caps) <= set(CAPS_FIELDS), (kw, caps)
    words = [repr(float(cfg[k])) if k in ("mean", "variance") else str(int(cfg[k])) for k in CONFIG_FIELDS]
    words += [str(int(max_clock))] + [str(int(caps.get(k, 0))) for k in CAPS_FIELDS] + [str(int(history_cap)), str(len(seeds))]
    words += [str(int(s)) for s in seeds]
    if rights is not None or rotation:
        rights = [1] * cfg["num_nodes"] if rights is None else list(rights)
        assert len(rights) == cfg["num_nodes"], (kw, rights)
        words += [str(int(rotation))] + [str(int(w)) for w in rights]
    return " ".join(words)


def compile_program(out, sanitize):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-pthread", "-w", SRC, "-o", out])
    return out


def run_program(exe, cases, timeout=600):
    """cases: (kw, max_clock, caps, seeds, history_cap) -> (exit status, one dict per case: the arrays of oracle_ctypes.hostmodel_run_batch plus
    the pool's words, the fence's count per instance and the branch counters; stderr's tail).  A crash is an exit status, not an exception."""
    text = "%d\n%s\n" % (len(cases), "\n".join(case_line(*c) for c in cases))
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    lines = run.stdout.splitlines()
    out, at = [], 0
    while at < len(lines) and len(out) < len(cases):
        head = lines[at].split()
        assert head[0] == "case", lines[at][:200]
        rc, m, n = int(head[1]), int(head[2]), int(head[3])
        at += 1
        if rc < 0:
            out.append(dict(rc=rc))
            continue
        if at + m + 1 > len(lines):  # (the program died inside this case)
            break
        cap = int(cases[len(out)][4])
        d = dict(rc=rc, faults=np.zeros(m, np.uint32), maxq=np.zeros(m, np.uint32), maxsnap=np.zeros(m, np.uint32), cal_free=np.zeros(m, np.uint32),
                 cal_bump=np.zeros(m, np.uint32), cal_chunks=np.zeros(m, np.uint32), violations=np.zeros(m, np.uint64), first_violation=[None] * m,
                 commit_counts=np.zeros((m, n), np.uint32), active_rounds=np.zeros((m, n), np.uint64), last_states=np.zeros((m, n), np.uint64),
                 histories=np.zeros((m, n, cap), dtype=[("proposer", "<u8"), ("index", "<u8"), ("time", "<i8")]))
        for i in range(m):
            w = [int(v) for v in lines[at + i].split()]
            for k, key in enumerate(("faults", "maxq", "maxsnap", "cal_free", "cal_bump", "cal_chunks", "violations")):
                d[key][i] = w[k]
            if w[6]:
                d["first_violation"][i] = (w[7], "store" if w[8] else "load")
            w = w[9:]
            d["commit_counts"][i], d["active_rounds"][i], d["last_states"][i] = w[:n], w[n:2 * n], w[2 * n:3 * n]
            w = w[3 * n:]
            for node in range(n):
                cnt = min(int(d["commit_counts"][i, node]), cap)
                rows = np.array(w[:3 * cnt], dtype=np.int64).reshape(cnt, 3)
                d["histories"][i, node, :cnt]["proposer"], d["histories"][i, node, :cnt]["index"] = rows[:, 0], rows[:, 1]
                d["histories"][i, node, :cnt]["time"] = rows[:, 2]
                w = w[3 * cnt:]
            assert not w
        stats = lines[at + m].split()
        assert stats[0] == "stats"
        d["stats"] = dict(zip(STATS, (int(v) for v in stats[1:])))
        at += m + 1
        out.append(d)
    return run.returncode, out, run.stderr[-3000:]


def oracle_run(oracle, kw, seeds, max_clock, history_cap):
    return oracle.run_batch(oracle.make_config(math_mode=1, **kw), np.asarray(seeds, dtype=np.uint64), max_clock, threads=4, history_cap=history_cap)


def assert_clean_equal(want, got, faults, what):
    """Every instance whose fault word is 0 equals the oracle: commit counts, active rounds, last states, histories."""
    clean = np.asarray(faults) == 0
    for key in RESULT_KEYS:
        assert (np.asarray(got[key])[clean] == want[key][clean]).all(), (what, key, np.flatnonzero(clean))
    return clean


def assert_faulted_cleanly(d, caps, what, allowed=CAPACITY_BITS):
    """The contract of a capacity that ran out, on every instance of the program's case `d`: no access outside the instance's rows, only capacity
    bits in the fault word, the allocator's words within the pool, commit counts within the log."""
    assert not d["violations"].any(), (what, "the fence", [(i, v) for i, v in enumerate(d["first_violation"]) if v])
    assert not (d["faults"] & ~np.uint32(allowed)).any(), (what, [hex(int(f)) for f in d["faults"]])
    if caps.get("qcal"):
        assert (d["cal_free"] <= d["cal_chunks"]).all() and (d["cal_bump"] <= d["cal_chunks"]).all(), (what, d["cal_free"], d["cal_bump"], d["cal_chunks"])
    assert (d["commit_counts"] <= caps["lcap"]).all(), what
    assert (d["maxq"] <= caps["qcap"]).all(), what


# (b) Mixed batches, 8 seeds at the capacities the planner gives the batch (queue_capacity 0 = automatic): (configuration, max_clock,
# queue_capacity, the host model's fault word per instance).  At 20 nodes (tiled class, push_event) the automatic 3200 entries give one faulted
# instance at uniform [0, 125]; at 40 nodes (cooperative loop, bulk_append) no upper bound gives a mixed batch within 400 ticks at the automatic
# 12800, so the queue_capacity is 12000.
MIXED = {
    "n20_push_event": (uniform(20, 0, 125), 400, 0, (0, 1, 0, 0, 0, 0, 0, 0)),
    "n40_bulk_append": (uniform(40, 0, 300), 400, 12000, (0, 0, 0, 1, 0, 1, 0, 0)),
}
MIXED_SEEDS = tuple(range(1, 9))


def planned_caps(oracle, kw, m, max_clock, queue_capacity=0, **plan_kw):
    """The host model's capacities and geometry as the device library plans the batch (csrc/lbft_plan.h through oracle_ctypes.plan)."""
    p = oracle.plan(oracle.make_config(math_mode=1, **kw), m, max_clock, queue_capacity=queue_capacity, **plan_kw)
    return {k: p[k] for k in ("qcap", "scap", "bcap", "lcap", "ql", "qheap", "qcal", "ring", "ring_topup", "tw")}


# (c) Every branch of the exhausted pool: (configuration, max_clock, capacities, seeds, the counters the case must raise).  Dense buckets (a group
# of 63 or 64 messages of one broadcast in ONE bucket takes three new chunks, a bucket of more than 31 entries has a full tail chunk) and more
# than 256 sparse ones at once need a delay that is 0 for most messages and anything up to the horizon for the rest: log-normal delays with
# sigma = 8 whose 95th percentile is half a tick, and the plain long tail of mean 20, variance 10000 for the tiled class.
BRANCHES = {
    "n65_coop_dense_and_sparse": (dict(num_nodes=65, mean=76107153.47807553, variance=3.611584660429568e+43), 1500,
                                  caps_of(4225, 16 * 65, ring=512, ring_topup=16, bcap=256, lcap=256), (1,),
                                  ("empty_bucket", "full_tail", "bulk_1", "bulk_2", "bulk_3", "short_stack")),
    "n20_tiled_long_tail": (dict(num_nodes=20, mean=20.0, variance=10000.0), 1500, caps_of(800, 320, bcap=256, lcap=256), (1, 2),
                            ("empty_bucket", "full_tail")),
}

# (e) Small capacities, drawn: FUZZ_DRAWS configurations of 3 seeds each, every capacity automatic (the planner's), generous or small.
FUZZ_SEED, FUZZ_DRAWS = 20261, 120  # (73 of the 120 draws end clean, 47 faulted; the plain program runs them in 4 s)


def fuzz_draws(oracle, seed=None, draws=None):
    """-> (configuration, max_clock, capacities, seeds, the fault bits the draw may raise) per draw.  A capacity drawn small may run out (its own
    bit); on the calendar the pool may as well (bit 0); nothing else may.  One capacity is never drawn automatic: the snapshot pool under the
    record exchange (quirks bit 0).  lbft_plan.h sizes it from high-water marks measured at the default delays (~n^2 requests and responses in
    flight, each holding a slot); the number in flight grows with the delay, and at 33 and 40 nodes with uniform delays of [10, 100] and [10, 30]
    the automatic 2112 / 2560 slots run out on the binary heap and the calendar alike (fault words [2, 2, 2] and [2, 2, 0], clean otherwise).
    That is a sizing question of the planner like the calendar pool's, not the fault safety these draws are about."""
    rng = np.random.default_rng(FUZZ_SEED if seed is None else seed)
    out = []
    for _ in range(FUZZ_DRAWS if draws is None else draws):
        n = int(rng.choice([5, 8, 17, 20, 33, 40]))
        kw = dict(num_nodes=n, quirks=int(rng.integers(0, 4)))
        if rng.random() < 0.5:
            kw.update(delay_model=1, uniform_lo=int(rng.integers(0, 21)), uniform_hi=int(rng.choice([30, 60, 100, 200, 300])))
        else:
            kw.update(mean=float(rng.choice([10.0, 25.0, 50.0])), variance=float(rng.choice([4.0, 400.0, 2500.0, 10000.0])))
        if rng.random() < 0.3:
            kw["equivocate_every"] = int(rng.integers(2, 6))
        if rng.random() < 0.3:
            kw["drop_per_million"] = int(rng.choice([1000, 50000, 300000]))
        max_clock = int(rng.choice([150, 300] if n > 20 else [200, 300]))
        qcal = int(rng.random() < 0.6)
        auto = planned_caps(oracle, kw, 3, max_clock, calendar_queue=bool(qcal))
        caps = dict(ql=0, qheap=1, qcal=qcal, ring=int(rng.choice([0, 128, 512])) if (qcal and n > 32) else 0, ring_topup=int(rng.choice([0, 4, 16])))
        allowed = F_QUEUE if qcal else 0
        generous = dict(qcap=max(4096, 64 * n * n), scap=max(128, 128 * n) if not kw["quirks"] & 1 else 6 * n * n + 16 * n, bcap=1024, lcap=1024)
        # (a full log comes with F_COMMIT_NOT_SUCCESSOR: commit_block stops a chain of commits at the full log after it has moved the node's last
        # committed block, so the node's next commit does not extend the last one it logged -- lbft_core.h commit_block and its callers)
        for bit, key in ((F_QUEUE, "qcap"), (F_SNAP, "scap"), (F_BLOCK, "bcap"), (F_LOG | F_NOT_SUCCESSOR, "lcap")):
            how = rng.choice(["auto", "generous", "small"], p=[0.35, 0.25, 0.4])
            if how == "auto" and key == "scap" and kw["quirks"] & 1:
                how = "generous"  # (see fuzz_draws' docstring)
            if how == "small":
                caps[key] = max(2, auto[key] // int(rng.choice([2, 4, 8, 16])))
                allowed |= bit
            else:
                caps[key] = auto[key] if how == "auto" else max(auto[key], generous[key])
        seeds = tuple(int(s) for s in rng.integers(1, 2 ** 62, 3, dtype=np.uint64))
        out.append((kw, max_clock, caps, seeds, allowed))
    return out
