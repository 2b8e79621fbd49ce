"""Edge cases of the accepted parameter domain: one table, run by the CPU tier (tests/test_edge_cases_host.py: the host build of the kernel
logic against the oracle) and the device tier (tests/test_edge_cases_gpu.py: BatchSimulator / with_param_sets against the oracle).

Every case sits at a boundary where the kernels keep state in fewer bits than the reference's i64, switch data structure or take a
different arithmetic path.  Its expected outcome is one of
  "equal"          every instance equals the oracle (math_mode 1);
  "fault:<bits>"   every instance has exactly these fault bits set (a value the kernels cannot represent is reported, never silently wrong);
  "refused:<code>" the C ABI rejects the configuration / horizon with that error code before any HIP call.
Parameter-set batches ("sets") carry an expectation per set: a lane's extreme set must neither leak into nor fault its neighbours.
A case with "host_only" runs on the CPU tier alone, for the reason written in it.

Sizing: slow delays with scaled delta and target_commit_interval keep the event counts of the huge horizons small (about 50 rounds), so
every oracle run here is bounded in time and memory.  (target_commit_interval = 0 never terminates in the reference and is not a case.)
"""

# fault bits (include/lbft.h)
F_QUEUE_OVERFLOW = 1 << 0
F_DURATION_TABLE = 1 << 5
F_STAMP_OVERFLOW = 1 << 8
F_INTERNAL = 1 << 9

LBFT_ERR_INVALID = -1

MAX_CLOCK_LIMIT = 2 ** 31 - 3  # the largest horizon lbft_batch_run_until accepts (LBFT_MAX_CLOCK in include/lbft.h)
CAL_MAX_CLOCK = 16383          # the largest horizon of the calendar event queue (LBFT_CAL_MAX_CLOCK, csrc/lbft_core.h)
QP_TIME_BITS = 21              # class 0's packed queue entries hold times < 2^21 (LBFT_QP_TIME_BITS)

# layout flag word (lbft_batch_layout out[7]): size class in the low byte, calendar queue bit 9
LAYOUT_CALENDAR = 1 << 9

# A slow network that runs to the top of the clock range in about 50 rounds: mean delay 2^24, delta 2^25, a commit deadline of 2^28.
SLOW = dict(mean=float(2 ** 24), variance=float(2 ** 46), delta=2 ** 25, target_commit_interval=2 ** 28)
# The same network scaled down by 2^10 so that it is busy around the class-0 horizon 2^21.
SLOW21 = dict(mean=float(2 ** 14), variance=float(2 ** 26), delta=2 ** 15, target_commit_interval=2 ** 18)
# A lossy mid-size network busy around the calendar limit (n = 7: outside class 0, queue capacity > 256 -> calendar or heap).
LOSSY = dict(mean=10.0, variance=4.0, drop_per_million=50000, delta=20, target_commit_interval=400)


def _seeds(k, first=1):
    return list(range(first, first + k))


CASES = [
    # ---- horizon limits -------------------------------------------------------------------------------------------------------------
    dict(name="max_clock_largest_accepted", n=4, cfg=SLOW, seeds=_seeds(6), max_clock=MAX_CLOCK_LIMIT, expect="equal"),
    dict(name="max_clock_one_above", n=4, cfg=SLOW, seeds=_seeds(2), max_clock=MAX_CLOCK_LIMIT + 1, expect="refused:%d" % LBFT_ERR_INVALID),
    dict(name="max_clock_2p31_minus_1", n=4, cfg=SLOW, seeds=_seeds(2), max_clock=2 ** 31 - 1, expect="refused:%d" % LBFT_ERR_INVALID),
    dict(name="max_clock_negative", n=4, cfg=SLOW, seeds=_seeds(2), max_clock=-1, expect="refused:%d" % LBFT_ERR_INVALID),
    # startup = delay + 1: 2^30 - 1 is the largest startup time the 32-bit node rows hold
    dict(name="startup_2p30_minus_1", n=4, cfg=dict(delay_model=1, uniform_lo=2 ** 30 - 2, uniform_hi=2 ** 30 - 2, delta=2 ** 25,
                                                     target_commit_interval=2 ** 28),
         seeds=_seeds(4), max_clock=MAX_CLOCK_LIMIT, expect="equal"),
    dict(name="startup_2p30", n=4, cfg=dict(delay_model=1, uniform_lo=2 ** 30 - 1, uniform_hi=2 ** 30 - 1, delta=2 ** 25,
                                            target_commit_interval=2 ** 28),
         seeds=_seeds(4), max_clock=MAX_CLOCK_LIMIT, expect="fault:%d" % F_INTERNAL),
    dict(name="startup_2p40", n=4, cfg=dict(delay_model=1, uniform_lo=2 ** 40, uniform_hi=2 ** 40, delta=2 ** 25, target_commit_interval=2 ** 28),
         seeds=_seeds(2), max_clock=MAX_CLOCK_LIMIT, expect="fault:%d" % F_INTERNAL),
    # ---- class 0's packed queue (times < 2^21) ----------------------------------------------------------------------------------------
    dict(name="class0_last_horizon", n=4, cfg=SLOW21, seeds=_seeds(8), max_clock=2 ** QP_TIME_BITS - 1, expect="equal", kernel_class=0),
    dict(name="class0_first_horizon_past", n=4, cfg=SLOW21, seeds=_seeds(8), max_clock=2 ** QP_TIME_BITS, expect="equal", kernel_class=1),
    dict(name="class0_uniform_last_horizon", n=3, cfg=dict(delay_model=1, uniform_lo=2 ** 13, uniform_hi=2 ** 15, delta=2 ** 15,
                                                           target_commit_interval=2 ** 18),
         seeds=_seeds(8), max_clock=2 ** QP_TIME_BITS - 1, expect="equal", kernel_class=0),
    # 2^25 creation stamps inside class 0's horizon: a commit deadline of 2 clock units makes every node query its peers at almost every
    # update (~590 stamps per round), rounds of ~40 units keep the blocks under the automatic capacity (65 534).  ~33.5 M events per instance.
    dict(name="class0_stamp_overflow", n=4, cfg=dict(mean=16.0, variance=4.0, delta=32, target_commit_interval=2, commands_per_epoch=10 ** 9),
         seeds=_seeds(2), max_clock=2 ** QP_TIME_BITS - 1, expect="fault:%d" % F_STAMP_OVERFLOW, kernel_class=0,
         host_only="33.5 M events executed one after another on a single lane: minutes on the device, past the device tier's budget"),
    # ---- calendar queue limit (LBFT_CAL_MAX_CLOCK) ------------------------------------------------------------------------------------
    dict(name="calendar_last_horizon", n=7, cfg=LOSSY, seeds=_seeds(4), max_clock=CAL_MAX_CLOCK, expect="equal", calendar=True),
    dict(name="calendar_last_horizon_heap", n=7, cfg=LOSSY, seeds=_seeds(4), max_clock=CAL_MAX_CLOCK, expect="equal", calendar=False,
         calendar_queue=False),
    dict(name="calendar_first_horizon_past", n=7, cfg=LOSSY, seeds=_seeds(4), max_clock=CAL_MAX_CLOCK + 1, expect="equal", calendar=False),
    dict(name="calendar_quirks1_last_horizon", n=5, cfg=dict(quirks=1, delta=20, target_commit_interval=400), seeds=_seeds(3),
         max_clock=CAL_MAX_CLOCK, expect="equal", calendar=True),
    dict(name="calendar_quirks1_first_horizon_past", n=5, cfg=dict(quirks=1, delta=20, target_commit_interval=400), seeds=_seeds(3),
         max_clock=CAL_MAX_CLOCK + 1, expect="equal", calendar=False),
    # ---- duration table: 4 096 rounds without a commit (gamma = 0: every round lasts delta) --------------------------------------------
    # (delta 5 against delays of mean 10: every round times out, about 14 clock units each; round 4 096 comes near clock 59 000)
    dict(name="duration_table_exhausted", n=4, cfg=dict(gamma=0.0, delta=5, target_commit_interval=2 ** 40),
         seeds=_seeds(3), max_clock=120000, expect="fault:%d" % F_DURATION_TABLE),
    dict(name="duration_table_last_entry", n=4, cfg=dict(gamma=0.0, delta=5, target_commit_interval=2 ** 40),
         seeds=_seeds(3), max_clock=50000, expect="equal"),
    # ---- f64_to_i64_sat: lambda * duration crosses 2^31; a duration that saturates to INT64_MAX ---------------------------------------
    dict(name="lambda_duration_crosses_2p31", n=4, cfg=dict(mean=float(2 ** 24), variance=float(2 ** 46), delta=2 ** 27, gamma=2.0,
                                                            lambda_=3.0, target_commit_interval=2 ** 28),
         seeds=_seeds(6), max_clock=MAX_CLOCK_LIMIT, expect="equal"),
    dict(name="delta_1e18", n=4, cfg=dict(delta=10 ** 18), seeds=_seeds(6), max_clock=3000, expect="equal"),
    dict(name="delta_1e15_gamma2", n=4, cfg=dict(delta=10 ** 15, gamma=2.0), seeds=_seeds(6), max_clock=3000, expect="equal"),
    dict(name="duration_saturates", n=4, cfg=dict(delta=2 ** 62, gamma=2.0, lambda_=4.0), seeds=_seeds(6), max_clock=3000, expect="equal"),
    dict(name="tci_2p62", n=4, cfg=dict(target_commit_interval=2 ** 62), seeds=_seeds(6), max_clock=3000, expect="equal"),
    # ---- uniform delays: span 1, ~2^32, ~2^62, lo above max_clock; small networks and a large one (cooperative fast_delay) ---------------
    dict(name="uniform_span1", n=4, cfg=dict(delay_model=1, uniform_lo=7, uniform_hi=7), seeds=_seeds(6), max_clock=2000, expect="equal"),
    # Spans of 2^32 and more: a startup time (first delay + 1) above 2^30 - 1 does not fit the node rows -> F_INTERNAL at init ...
    dict(name="uniform_span_2p32", n=4, cfg=dict(delay_model=1, uniform_lo=3, uniform_hi=2 ** 32 + 2), seeds=_seeds(6), max_clock=2000,
         expect="fault:%d" % F_INTERNAL),
    dict(name="uniform_span_2p62", n=4, cfg=dict(delay_model=1, uniform_lo=0, uniform_hi=2 ** 62 + 12345), seeds=_seeds(6), max_clock=2000,
         expect="fault:%d" % F_INTERNAL),
    dict(name="uniform_span_2p63", n=4, cfg=dict(delay_model=1, uniform_lo=0, uniform_hi=2 ** 63 - 1), seeds=_seeds(6), max_clock=2000,
         expect="fault:%d" % F_INTERNAL),
    # ... except for seeds whose four startups all fit (1 in ~256): then the run to the top of the clock range equals the oracle
    dict(name="uniform_span_2p32_startups_fit", n=4, cfg=dict(delay_model=1, uniform_lo=3, uniform_hi=2 ** 32 + 2, delta=2 ** 25,
                                                              target_commit_interval=2 ** 28),
         seeds=[467, 506, 582, 1132, 1164, 1503], max_clock=MAX_CLOCK_LIMIT, expect="equal", startups_fit=True),
    dict(name="uniform_lo_above_horizon", n=4, cfg=dict(delay_model=1, uniform_lo=5000, uniform_hi=9000), seeds=_seeds(6), max_clock=2000,
         expect="equal"),
    dict(name="uniform_span_2p32_lossy7", n=7, cfg=dict(delay_model=1, uniform_lo=3, uniform_hi=2 ** 32 + 2, drop_per_million=10000),
         seeds=_seeds(4), max_clock=2000, expect="fault:%d" % F_INTERNAL, calendar=True),
    dict(name="large_uniform_span1", n=40, cfg=dict(delay_model=1, uniform_lo=7, uniform_hi=7), seeds=_seeds(2), max_clock=300,
         expect="equal", calendar=True),
    dict(name="large_uniform_span_3x2p61", n=40, cfg=dict(delay_model=1, uniform_lo=1, uniform_hi=3 * 2 ** 61), seeds=_seeds(2),
         max_clock=300, expect="fault:%d" % F_INTERNAL, calendar=True),
    dict(name="large_uniform_span_2p32_plus", n=40, cfg=dict(delay_model=1, uniform_lo=2, uniform_hi=2 ** 32 + 2 ** 31), seeds=_seeds(2),
         max_clock=300, expect="fault:%d" % F_INTERNAL, calendar=True),
    dict(name="large_uniform_span_17", n=40, cfg=dict(delay_model=1, uniform_lo=1, uniform_hi=17), seeds=_seeds(2), max_clock=300,
         expect="equal", calendar=True),
    dict(name="large_uniform_lo_above_horizon", n=40, cfg=dict(delay_model=1, uniform_lo=400, uniform_hi=1000), seeds=_seeds(2),
         max_clock=300, expect="equal", calendar=True),
    # ---- log-normal delays: variance 1e12 (exp leaves trunc_exp's |t| < 20 window), mean below 1 (every delay 0) ------------------------
    dict(name="lognormal_variance_1e12", n=4, cfg=dict(mean=10.0, variance=1e12), seeds=_seeds(6), max_clock=3000, expect="equal"),
    dict(name="lognormal_mean_below_1", n=4, cfg=dict(mean=0.5, variance=0.01, target_commit_interval=50), seeds=[1], max_clock=1,
         expect="equal", block_capacity=1024),  # (zero delays: ~600 rounds at clock 1, more blocks than the automatic capacity)
    # ---- refused configurations (validate(): lbft_batch_create before any HIP call) ------------------------------------------------------
    dict(name="refused_negative_delta", n=4, cfg=dict(delta=-1), seeds=_seeds(1), max_clock=100, expect="refused:%d" % LBFT_ERR_INVALID),
    dict(name="refused_nan_gamma", n=4, cfg=dict(gamma=float("nan")), seeds=_seeds(1), max_clock=100, expect="refused:%d" % LBFT_ERR_INVALID),
    dict(name="refused_infinite_lambda", n=4, cfg=dict(lambda_=float("inf")), seeds=_seeds(1), max_clock=100,
         expect="refused:%d" % LBFT_ERR_INVALID),
    dict(name="refused_negative_tci", n=4, cfg=dict(target_commit_interval=-1), seeds=_seeds(1), max_clock=100,
         expect="refused:%d" % LBFT_ERR_INVALID),
    dict(name="refused_uniform_hi_below_lo", n=4, cfg=dict(delay_model=1, uniform_lo=10, uniform_hi=9), seeds=_seeds(1), max_clock=100,
         expect="refused:%d" % LBFT_ERR_INVALID),
]


# ---- parameter-set batches: extreme sets next to an ordinary one (set 0), in the small (K_SMALL_SETS) and the mid (K_MID_SETS) class -------
# (a set: the ParamSet fields that differ from the ordinary set, and its expectation)
_ORDINARY = dict(mean=10.0, variance=4.0, uniform_lo=5, uniform_hi=15, delta=20, gamma=2.0, lambda_=0.5, target_commit_interval=100000)
_LOGNORMAL_SETS = [
    (dict(), "equal"),
    (dict(delta=10 ** 18), "equal"),
    (dict(delta=10 ** 15, gamma=2.0), "equal"),
    (dict(delta=2 ** 62, lambda_=4.0), "equal"),
    (dict(target_commit_interval=2 ** 62), "equal"),
    (dict(variance=1e12), "equal"),
    (dict(gamma=0.0, delta=5, target_commit_interval=2 ** 40), "equal"),
    (dict(mean=float(2 ** 40), variance=1.0), "fault:%d" % F_INTERNAL),
]
_UNIFORM_SETS = [
    (dict(), "equal"),
    (dict(uniform_lo=7, uniform_hi=7), "equal"),
    (dict(uniform_lo=5000, uniform_hi=9000), "equal"),
    (dict(uniform_lo=1, uniform_hi=40), "equal"),
    (dict(uniform_lo=3, uniform_hi=2 ** 32 + 2), "fault:%d" % F_INTERNAL),
    (dict(uniform_lo=0, uniform_hi=2 ** 63 - 1), "fault:%d" % F_INTERNAL),
]
PARAM_SET_CASES = [
    dict(name="sets_small_lognormal", n=4, delay_model=0, sets=_LOGNORMAL_SETS, per=3, max_clock=3000, kernel_class=0),
    dict(name="sets_mid_lognormal", n=7, delay_model=0, drop_per_million=20000, sets=_LOGNORMAL_SETS, per=3, max_clock=3000, kernel_class=1),
    dict(name="sets_small_uniform", n=4, delay_model=1, sets=_UNIFORM_SETS, per=3, max_clock=2000, kernel_class=0),
    dict(name="sets_mid_uniform", n=7, delay_model=1, drop_per_million=20000, sets=_UNIFORM_SETS, per=3, max_clock=2000, kernel_class=1),
]


def set_fields(case, k):
    """The full ParamSet fields of set k of a parameter-set case (loss is the case's, for every set)."""
    f = dict(_ORDINARY)
    f.update(case["sets"][k][0])
    f["drop_per_million"] = case.get("drop_per_million", 0)
    return f


def set_layout(case):
    """(set_of_instance, seeds): `per` instances of every set, interleaved so that extreme and ordinary sets share wavefronts."""
    n_sets = len(case["sets"])
    m = n_sets * case["per"]
    set_of = [i % n_sets for i in range(m)]
    seeds = [1000 + i for i in range(m)]
    return set_of, seeds


def set_as_case(case, k):
    """Set k of a parameter-set case as a plain case (for the oracle and the plain-batch comparisons)."""
    f = set_fields(case, k)
    cfg = {key: f[key] for key in ("target_commit_interval", "delta", "gamma", "lambda_", "drop_per_million")}
    if case["delay_model"] == 1:
        cfg.update(delay_model=1, uniform_lo=f["uniform_lo"], uniform_hi=f["uniform_hi"])
    else:
        cfg.update(mean=f["mean"], variance=f["variance"])
    return dict(name="%s[%d]" % (case["name"], k), n=case["n"], cfg=cfg, max_clock=case["max_clock"], expect=case["sets"][k][1])


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def expected(case):
    """("equal", None) | ("fault", bits) | ("refused", code)."""
    kind, _, arg = case["expect"].partition(":")
    return kind, (int(arg) if arg else None)


def oracle_config(oc, case, math_mode=1):
    return oc.make_config(num_nodes=case["n"], math_mode=math_mode, **case["cfg"])


def host_caps(case):
    """The capacities and queue discipline the device library chooses for this case (oracle_ctypes.plan: csrc/lbft_plan.h compiled into
    the host model), as arguments of oracle_ctypes.hostmodel_run_batch."""
    import oracle_ctypes as oc
    c = oc.plan(oracle_config(oc, case), len(case["seeds"]), case["max_clock"], block_capacity=case.get("block_capacity", 0),
                calendar_queue=case.get("calendar_queue", True))
    return dict({k: c[k] for k in ("qcap", "scap", "bcap", "lcap", "qheap", "qcal", "ring", "ring_topup")}, ql=0 if c["qcal"] else 16)


def expected_layout(case):
    """(kernel size class, heap flag, calendar flag, cooperative flag) as lbft_batch_layout must report them: stated here from the case
    alone (every capacity of the table but block_capacity is automatic), independently of the planner the device and host_caps use."""
    n, mc, cfg = case["n"], case["max_clock"], case["cfg"]
    q1 = cfg.get("quirks", 0) & 1
    qcap = max(128, 16 * n * n if n <= 16 else 8 * n * n)
    scap = max(32, min(65535, max(n * n + 8 * n, 64 * n) if q1 else 8 * n))
    heap = qcap > 256 or n > 32
    small = n <= 16 and not heap and not cfg.get("drop_per_million") and not cfg.get("partition_size") and not q1
    cls = 2 if n > 32 else (0 if small and mc < 2 ** QP_TIME_BITS and scap <= 256 else 1)
    qcal = int(not small and heap and case.get("calendar_queue", True) and mc <= CAL_MAX_CLOCK)
    return cls, int(heap), qcal, int(n > 32 and qcal)


def lbft_config(case):
    """The case's configuration as the C ABI's lbft_config (for the argument checks)."""
    from librabft_simulator_amd import _lib
    c = _lib.LbftConfig()
    f = dict(mean=10.0, variance=4.0, delay_model=0, uniform_lo=5, uniform_hi=15, target_commit_interval=100000, delta=20, gamma=2.0,
             lambda_=0.5, quirks=0, drop_per_million=0)
    f.update(case["cfg"])
    c.num_nodes, c.commands_per_epoch = case["n"], 30000
    for k, v in f.items():
        setattr(c, k, v)
    return c


COMPARED = ("commit_counts", "active_rounds", "last_states", "histories")
COMPARED_COUNTERS = ("events", "rng_draws", "events_scheduled")
HISTORY_CAP = 64
