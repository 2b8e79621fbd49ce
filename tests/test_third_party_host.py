"""The arithmetic both sides of every parity test share, held to a reference neither has a part in.

The oracle includes the product's csrc/lbft_tables.h and csrc/lbft_math.h and restates the same third-party arithmetic as the kernels
(SURVEY.md Appendix A), so a wrong table word or slow-path constant moves device and oracle together.  tests/third_party_reference.py
restates Appendix A a third time, in plain Python on the host libm, with no table, header or code in common.  Here, on the CPU:
 (a) the reference reproduces the literals of Appendix A / B, which come from the reference project's own runs;
 (b) the committed lbft_tables.h equals the reference's ziggurat tables and a >= 200-bit 2^(k/128) table, and tools/gen_tables.py still
     generates exactly that header;
 (c) the log data block of lbft_math.h has the construction glibc gives it;
 (d) the oracle, through every export of this layer and in both math modes, equals the reference;
 (e) the reference's own counters show that (d) reached the rare paths: wedge rejections, the tail loop, gen_range rejections."""
import ctypes
import fractions
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import third_party_cases as cases
import third_party_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "librabft_simulator_amd", "csrc")
Fraction = fractions.Fraction


# ---- (a) the reference against the literals of Appendix A / B --------------------------------------------------------------------
def test_reference_xoshiro_siphash_pick_author_literals():
    rng = ref.Xoshiro(52)
    assert [rng.next_u64() for _ in range(3)] == [0x81e93ae64dfa3e63, 0x79f50e0b404f5d45, 0x0beae4adbcb274ae]
    assert rng.draws == 3
    assert ref.siphash13(ref.le64(0)) == 13646096770106105413
    assert ref.siphash13(ref.le64(1)) == 2206609067086327257
    assert [ref.pick_author([1, 2, 5], s) for s in range(20, 28)] == [1, 0, 1, 2, 1, 2, 1, 1]
    assert [ref.leader([1] * 3, r) for r in range(1, 13)] == [1, 2, 2, 2, 1, 2, 1, 1, 2, 1, 2, 0]
    assert [ref.leader([1] * 8, r) for r in range(1, 13)] == [7, 6, 3, 5, 6, 6, 3, 5, 3, 5, 3, 7]


def test_reference_ziggurat_table_literals():
    X, F = ref.ziggurat_tables()
    assert len(X) == len(F) == 257
    assert ["%.18f" % v for v in X[:4]] == ["3.910757959537090045", "3.654152885361008796", "3.449278298560964462", "3.320244733839166074"]
    assert ["%.18f" % v for v in F[:2]] == ["0.000477467764586655", "0.001260285930498598"]
    assert abs(X[255] - 0.2152418959132738) < 1e-15
    assert X[256] == 0.0 and F[256] == 1.0
    assert all(a > b for a, b in zip(X, X[1:])) and all(a < b for a, b in zip(F, F[1:]))


def test_reference_startup_times():
    """Startup time = the node's first delay + 1 (Appendix B)."""
    assert [d + 1 for d in ref.lognormal_delays(52, 10.0, 4.0, 3)] == [10, 10, 8]
    assert [d + 1 for d in ref.lognormal_delays(48, 10.0, 4.0, 8)] == [12, 10, 11, 14, 7, 8, 7, 13]
    assert [d + 1 for d in ref.lognormal_delays(1, 10.0, 0.0, 3)] == [11, 11, 11]


# ---- high-precision helpers: exact rationals out of mpmath (>= 200 bits), or decimal at 80 digits without it ----------------------
try:
    import mpmath
except ImportError:  # pragma: no cover
    mpmath = None
import decimal


def _frac_of_mpf(v):
    sign, man, exp, _ = v._mpf_  # (man_exp alone drops the sign)
    return Fraction(-man if sign else man) * Fraction(2) ** exp


def hp_pow2(k, n):
    """2^(k/n)"""
    if mpmath is not None:
        with mpmath.workprec(256):
            return _frac_of_mpf(mpmath.power(2, mpmath.mpf(k) / n))
    with decimal.localcontext() as c:
        c.prec = 80
        return Fraction((decimal.Decimal(2).ln() * k / n).exp())


def hp_ln(q):
    """ln of a positive Fraction"""
    if mpmath is not None:
        with mpmath.workprec(256):
            return _frac_of_mpf(mpmath.log(mpmath.mpf(q.numerator) / mpmath.mpf(q.denominator)))
    with decimal.localcontext() as c:
        c.prec = 80
        return Fraction((decimal.Decimal(q.numerator) / decimal.Decimal(q.denominator)).ln())


def nearest_double(q):
    return q.numerator / q.denominator  # int / int is correctly rounded in CPython


# ---- (b) the committed header ----------------------------------------------------------------------------------------------------
def header_words(text, name):
    m = re.search(r"#define\s+%s\s*\{(.*?)\}" % re.escape(name), text, re.S)
    assert m, name
    return [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]{16})ULL", m.group(1))]


@pytest.fixture(scope="module")
def tables_h():
    with open(os.path.join(CSRC, "lbft_tables.h")) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def gen_tables():
    spec = importlib.util.spec_from_file_location("gen_tables_under_test", os.path.join(ROOT, "tools", "gen_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # (defines functions only: the header is written by its main())
    return mod


def exp_tab_reference():
    out = []
    for k in range(128):
        v = hp_pow2(k, 128)
        h = nearest_double(v)
        t = nearest_double(v / Fraction(h) - 1)
        out.append((ref.bits(t), ref.bits(h) - (k << 45)))
    return out


def test_header_ziggurat_tables_equal_the_reference(tables_h, gen_tables):
    X, F = ref.ziggurat_tables()
    hx, hf = header_words(tables_h, "LBFT_ZIG_NORM_X_BITS_INIT"), header_words(tables_h, "LBFT_ZIG_NORM_F_BITS_INIT")
    assert len(hx) == len(hf) == 257
    assert [i for i in range(257) if hx[i] != ref.bits(X[i])] == []
    assert [i for i in range(257) if hf[i] != ref.bits(F[i])] == []
    m = re.search(r"#define\s+LBFT_ZIG_NORM_R_BITS\s+0x([0-9a-fA-F]{16})ULL", tables_h)
    assert m and int(m.group(1), 16) == ref.bits(3.6541528853610088)
    gx, gf = gen_tables.gen_zig()  # (runs the generator's own asserts too)
    assert [ref.bits(v) for v in gx] == hx and [ref.bits(v) for v in gf] == hf


def test_header_exp_table_equals_a_200_bit_computation(tables_h, gen_tables):
    words = header_words(tables_h, "LBFT_EXP_TAB_INIT")
    assert len(words) == 256
    pairs = list(zip(words[0::2], words[1::2]))
    want = exp_tab_reference()
    assert [k for k in range(128) if pairs[k] != want[k]] == []
    assert gen_tables.gen_exp_tab() == pairs


# ---- (c) the log data block of lbft_math.h ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def log_data():
    with open(os.path.join(CSRC, "lbft_math.h")) as fh:
        words = header_words(fh.read(), "LBFT_LOG_DATA_INIT")
    assert len(words) == 274
    return words


def test_log_data_block_construction(log_data):
    """What glibc's table generator guarantees, whatever binary the words were read out of.  ln2hi + ln2lo is ln 2 to double-double
    accuracy, and ln2hi leaves its 11 low bits free so that k * ln2hi is exact for |k| < 2^11.  invc_i is chosen near 1 / (centre of
    interval i) such that -ln(invc_i) lies within 2^-60 of a multiple of 2^-43, and logc_i is that multiple, so k * ln2hi + logc_i is
    exact as well.  Intervals are 2^-7 wide in z / centre, so |z invc_i - 1| < 2^-8 over each.  Measured on the committed block:
    ln2hi + ln2lo - ln 2 = -1.9e-31, worst |logc + ln invc| = 2^-66.9, worst |z invc - 1| = 0.003891."""
    D = [Fraction(ref.from_bits(w)) for w in log_data]
    ln2 = hp_ln(Fraction(2))
    err = D[0] + D[1] - ln2
    print("ln2hi + ln2lo - ln 2 = %.3g" % float(err))
    assert abs(err) <= Fraction(1, 2 ** 100)
    assert log_data[0] & 0x7ff == 0
    worst_logc = worst_r = Fraction(0)
    for i in range(128):
        invc, logc = D[18 + 2 * i], D[19 + 2 * i]
        assert (logc * 2 ** 43).denominator == 1, i
        worst_logc = max(worst_logc, abs(logc + hp_ln(invc)))
        lo = cases.LOG_SEAM0 + (i << 45)
        for zb in (lo, lo + (1 << 45)):  # the interval's first point and its (exclusive) upper end
            worst_r = max(worst_r, abs(Fraction(ref.from_bits(zb)) * invc - 1))
    print("worst |logc + ln invc| = 2^%.1f, worst |z invc - 1| = %.6f" % (math.log2(float(worst_logc)), float(worst_r)))
    assert worst_logc <= Fraction(1, 2 ** 60)
    assert worst_r < Fraction(1, 2 ** 8)


# ---- (d) the oracle equals the reference -----------------------------------------------------------------------------------------
def test_oracle_xoshiro(oracle):
    L = oracle.lib()
    for seed in (0, 1, 52, 2 ** 63, 2 ** 64 - 1):
        out = np.zeros(1000, dtype=np.uint64)
        L.lbft_oracle_xoshiro_first(seed, out.ctypes.data, 1000)
        rng = ref.Xoshiro(seed)
        assert [int(v) for v in out] == [rng.next_u64() for _ in range(1000)], seed


def test_oracle_shuffle(oracle):
    L = oracle.lib()
    for seed in (0, 1, 52, 2 ** 64 - 1):
        for n in range(129):
            out = np.full(max(n, 1), 0xdeadbeef, dtype=np.uint32)
            L.lbft_oracle_shuffle(seed, out.ctypes.data, n)
            want = ref.shuffle(seed, n)
            assert sorted(want) == list(range(n))
            assert [int(v) for v in out[:n]] == want, (seed, n)


@pytest.mark.parametrize("wi", range(len(cases.WEIGHTS)), ids=[cases.weights_id(w) for w in cases.WEIGHTS])
def test_oracle_leader_and_pick_author(oracle, wi):
    L = oracle.lib()
    w = cases.WEIGHTS[wi]
    wa = np.array(w, dtype=np.uint64)
    want, _ = cases.leaders(wi, 300)
    got = [int(L.lbft_oracle_leader(wa.ctypes.data, len(w), r)) for r in range(300)]
    assert got == want
    for r in cases.BIG_ROUNDS:
        assert int(L.lbft_oracle_leader(wa.ctypes.data, len(w), r)) == ref.leader(w, r), r
    assert all(w[a] > 0 for a in want)  # an author without votes never leads
    assert [int(L.lbft_oracle_pick_author(wa.ctypes.data, len(w), s)) for s in range(100)] == [ref.pick_author(w, s) for s in range(100)]
    if all(v == 1 for v in w):  # (NULL rights = all 1)
        assert [int(L.lbft_oracle_leader(None, len(w), r)) for r in range(300)] == want


@pytest.mark.parametrize("seed,mean,variance", cases.LOGNORMAL_ROWS)
def test_oracle_lognormal_delays(oracle, seed, mean, variance):
    L = oracle.lib()
    n = 100000
    want, _, _ = cases.lognormal(seed, mean, variance, n)
    for mode in (0, 1):
        out = np.zeros(n, dtype=np.int64)
        L.lbft_oracle_sample_delays(ctypes.byref(oracle.make_config(mean=mean, variance=variance, math_mode=mode)), seed, out.ctypes.data, n)
        bad = np.flatnonzero(out != np.array(want, dtype=np.int64))
        assert bad.size == 0, (mode, bad[:5], out[bad[:5]], [want[i] for i in bad[:5]])


@pytest.mark.parametrize("lo,hi", cases.UNIFORM_ROWS)
def test_oracle_uniform_delays(oracle, lo, hi):
    L = oracle.lib()
    n = 5000
    want = ref.uniform_delays(cases.UNIFORM_SEED, lo, hi, n)
    assert lo <= min(want) and max(want) <= hi
    for mode in (0, 1):
        out = np.zeros(n, dtype=np.int64)
        cfg = oracle.make_config(delay_model=1, uniform_lo=lo, uniform_hi=hi, math_mode=mode)
        L.lbft_oracle_sample_delays(ctypes.byref(cfg), cases.UNIFORM_SEED, out.ctypes.data, n)
        assert [int(v) for v in out] == want, mode


def test_oracle_siphash13_every_tail_length(oracle):
    L = oracle.lib()
    for n in range(25):
        for data in (bytes((37 * i + 11) & 0xff for i in range(n)), b"\xff" * n, b"\x00" * n):
            assert int(L.lbft_oracle_siphash13(data, n)) == ref.siphash13(data), (n, data)


def test_oracle_strict_exp_log_at_the_branch_boundaries(oracle):
    """The points tests/test_third_party_gpu.py gives the device, on the g++ build of the same source: every one equals the host libm."""
    L = oracle.lib()
    log_x = [ref.from_bits(b) for b in cases.log_points()]
    exp_x = cases.exp_points()
    assert len(log_x) == 1099 and len(exp_x) == 126
    assert [x.hex() for x in log_x if ref.bits(L.lbft_oracle_log_strict(x)) != ref.bits(math.log(x))] == []
    assert [x.hex() for x in exp_x if ref.bits(L.lbft_oracle_exp_strict(x)) != ref.bits(math.exp(x))] == []
    assert L.lbft_oracle_log_strict(0.0) == L.lbft_oracle_log_strict(-0.0) == -math.inf and L.lbft_oracle_log_strict(math.inf) == math.inf
    assert all(math.isnan(L.lbft_oracle_log_strict(x)) for x in (-1.5, -math.inf, math.nan))
    assert L.lbft_oracle_exp_strict(math.inf) == L.lbft_oracle_exp_strict(709.79) == math.inf and math.isnan(L.lbft_oracle_exp_strict(math.nan))
    assert ref.bits(L.lbft_oracle_exp_strict(-math.inf)) == ref.bits(L.lbft_oracle_exp_strict(-745.14)) == 0


# ---- (e) the rare paths were reached: the reference's own counters ---------------------------------------------------------------
def test_reference_reaches_the_sampler_slow_paths():
    """Seed 99, 100 000 normals (the path counts do not depend on mean or variance: they are decided before mu and sigma apply).
    Measured with this module: 102 287 draws = 100 000 + 721 rejected first draws + 1 494 wedge draws + 2 (34 + 2) tail draws;
    1 494 wedge tests, 721 rejected; 34 tail entries, 2 tail-loop rejections.  The expected tail rate is 2.7e-4 per sample (27 in
    100 000) and the wedge-test rate about 1.5 %, so the floors below are what the distribution gives, not what a run happened to."""
    for _, mean, variance in (row for row in cases.LOGNORMAL_ROWS if row[0] == 99):
        d, c, draws = cases.lognormal(99, mean, variance, 100000)
        assert c == dict(fast=99193, wedge=1494, wedge_rejected=721, tail=34, tail_rejected=2), (mean, variance, c)
        assert draws == 102287 == 100000 + c["wedge_rejected"] + c["wedge"] + 2 * (c["tail"] + c["tail_rejected"])
        assert c["tail"] >= 30 and c["tail_rejected"] >= 1 and c["wedge_rejected"] >= 700
        assert c["fast"] + (c["wedge"] - c["wedge_rejected"]) + c["tail"] == 100000
        if mean == 1e16:  # the magnifier row: every delay carries at least 45 bits of its sample and none saturates an i64
            assert 2 ** 45 <= min(d) and max(d) < 2 ** 62 and sum(v >= 2 ** 52 for v in d) > 50000
    _, c, _ = cases.lognormal(2 ** 64 - 1, 10.0, 4.0, 100000)
    assert c["tail"] >= 10 and c["tail_rejected"] >= 1 and c["wedge_rejected"] >= 500, c  # measured: 20, 3, 636
    # the tail magnifier (third_party_cases.TAIL_SEED): the chosen sample is the largest of its first 2 000, a positive tail sample
    # beyond 5 sigma, and its delay is wide enough to carry the normal's last bits
    mu, sigma = ref.lognormal_params(1e10, 2e41)
    rng, c = ref.Xoshiro(cases.TAIL_SEED), ref.NormalCounts()
    normals = [ref.standard_normal(rng, c) for _ in range(2000)]
    assert c.as_dict() == dict(fast=1987, wedge=25, wedge_rejected=15, tail=3, tail_rejected=0)
    assert max(normals) == normals[cases.TAIL_SAMPLE] > 5.16 and 6.99 < sigma < 7.01
    d, _, _ = cases.lognormal(cases.TAIL_SEED, 1e10, 2e41, 100000)
    assert d[cases.TAIL_SAMPLE] == int(math.exp(mu + sigma * normals[cases.TAIL_SAMPLE])) > 2 ** 49 and max(d) < 2 ** 62


def test_reference_reaches_gen_range_rejections():
    """gen_range_u64 rejects a draw with probability 1 - (zone + 1) / 2^64, zone + 1 = n << clz(n): a third for a total of 3 or 12
    (measured over rounds 0..299: 105 and 101), one half for a power of two, about 2^-33 for 128 x 0xffffff (measured 0; kept for its
    64 x 64 products, the largest the accepted rights give).  gen_range_u32 over the shuffles of lengths 0..128, seed 52: 3 639."""
    rejects = {cases.weights_id(w): cases.leaders(wi, 300)[1] for wi, w in enumerate(cases.WEIGHTS)}
    print(rejects)
    assert rejects["n3_total3"] == 105 and rejects["n5_total12"] == 101 and rejects["n128_total%d" % (128 * 0xffffff)] == 0
    assert max(rejects.values()) >= 50
    total = 0
    for n in range(129):
        rng = []
        ref.shuffle(52, n, rng)
        total += rng[0].rejects_u32
        assert rng[0].draws == (n - 1 if n > 1 else 0) + rng[0].rejects_u32
    assert total == 3639 and total >= 1000


# ---- the CLI's defaults (section 3d's CPU part): librabft-v2/src/main.rs of the reference, read once, as literals ------------------
def test_cli_defaults_are_the_reference_cli_defaults():
    from librabft_simulator_amd.__main__ import get_arguments
    a = get_arguments([])
    assert (a.max_clock, a.mean, a.variance, a.nodes) == (1000, 10.0, 4.0, 3)
    assert (a.commands_per_epoch, a.target_commit_interval) == (30000, 100000)
    assert (a.delta, a.gamma, a.lambda_) == (20, 2.0, 0.5)
    assert a.seed is None and a.instances == 1
