"""The third-party arithmetic of the reference simulator, restated from SURVEY.md Appendix A and from nothing else: SplitMix64 /
Xoshiro256**, rand 0.8 gen_range and shuffle, SipHash-1-3 with zero keys, pick_author and the leader of a round, the ziggurat tables
of rand_distr 0.4 with their "%.18f" round trip, StandardNormal, the LogNormal and the uniform delay.

The module is the INDEPENDENT party of tests/test_third_party_host.py and tests/test_third_party_gpu.py: it imports nothing from the
package, csrc/ or oracle/, reads no generated header and shares no table with them.  Integers are Python ints masked to 64 / 32 bits;
doubles are Python floats (binary64, one rounding per operation, never contracted); exp / log / sqrt are the host libm's through
`math`, scalar by scalar, which is what the Rust reference calls.  No vectorised transcendental anywhere: those are not libm."""
import math
import struct

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


def bits(x):
    """The binary64 bit pattern of a float."""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u & M64))[0]


def _rotl(x, b):
    return ((x << b) | (x >> (64 - b))) & M64


class Xoshiro:
    """Xoshiro256** seeded as seed_from_u64 does (four SplitMix64 outputs).  `draws` counts next_u64 calls; `rejects_u64` /
    `rejects_u32` count the draws gen_range threw away."""

    def __init__(self, seed):
        x = seed & M64
        s = []
        for _ in range(4):
            x = (x + 0x9e3779b97f4a7c15) & M64
            z = x
            z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
            z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
            s.append(z ^ (z >> 31))
        self.s = s
        self.draws = 0
        self.rejects_u64 = 0
        self.rejects_u32 = 0

    def next_u64(self):
        s = self.s
        self.draws += 1
        r = (_rotl((s[1] * 5) & M64, 7) * 9) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = _rotl(s[3], 45)
        return r

    def next_u32(self):
        return self.next_u64() >> 32

    def gen_range_u64(self, n):
        """gen_range(0..n) on the u64 / usize path; 1 <= n < 2^64."""
        assert 0 < n <= M64
        zone = ((n << (64 - n.bit_length())) - 1) & M64  # n << clz64(n)
        while True:
            m = self.next_u64() * n  # the 128-bit product
            if m & M64 <= zone:
                return m >> 64
            self.rejects_u64 += 1

    def gen_range_u32(self, n):
        """gen_range(0..n) on the u32 path; 1 <= n < 2^32."""
        assert 0 < n <= M32
        zone = ((n << (32 - n.bit_length())) - 1) & M32
        while True:
            m = self.next_u32() * n
            if m & M32 <= zone:
                return m >> 32
            self.rejects_u32 += 1

    def shuffle(self, v):
        """SliceRandom::shuffle in place: fewer than two elements draw nothing."""
        for i in range(len(v) - 1, 0, -1):
            j = self.gen_range_u32(i + 1)
            v[i], v[j] = v[j], v[i]
        return v


def shuffle(seed, n, rng_out=None):
    """[0..n) shuffled by a fresh Xoshiro(seed); `rng_out`: a list that receives the generator (for its counters)."""
    rng = Xoshiro(seed)
    if rng_out is not None:
        rng_out.append(rng)
    return rng.shuffle(list(range(n)))


def siphash13(data):
    """SipHash-1-3, k0 = k1 = 0, over a byte string."""
    v = [0x736f6d6570736575, 0x646f72616e646f6d, 0x6c7967656e657261, 0x7465646279746573]

    def rnd():
        v[0] = (v[0] + v[1]) & M64; v[1] = _rotl(v[1], 13); v[1] ^= v[0]; v[0] = _rotl(v[0], 32)
        v[2] = (v[2] + v[3]) & M64; v[3] = _rotl(v[3], 16); v[3] ^= v[2]
        v[0] = (v[0] + v[3]) & M64; v[3] = _rotl(v[3], 21); v[3] ^= v[0]
        v[2] = (v[2] + v[1]) & M64; v[1] = _rotl(v[1], 17); v[1] ^= v[2]; v[2] = _rotl(v[2], 32)

    n = len(data)
    whole = n - n % 8
    for i in range(0, whole, 8):
        m = int.from_bytes(data[i:i + 8], "little")
        v[3] ^= m; rnd(); v[0] ^= m
    b = ((n & 0xff) << 56) | int.from_bytes(data[whole:], "little")
    v[3] ^= b; rnd(); v[0] ^= b
    v[2] ^= 0xff
    rnd(); rnd(); rnd()
    return v[0] ^ v[1] ^ v[2] ^ v[3]


def le64(*words):
    return b"".join((w & M64).to_bytes(8, "little") for w in words)


def pick_author(weights, seed, rng_out=None):
    """EpochConfiguration::pick_author: the first author, in order, whose votes exceed what is left of the target."""
    rng = Xoshiro(seed)
    if rng_out is not None:
        rng_out.append(rng)
    target = rng.gen_range_u64(sum(weights))
    for a, w in enumerate(weights):
        if w > target:
            return a
        target -= w
    raise AssertionError("pick_author: unreachable")


def leader(weights, rnd, rng_out=None):
    return pick_author(weights, siphash13(le64(rnd)), rng_out)


ZIG_R = 3.6541528853610088
ZIG_V = 0.00492867323399
_tables = None


def ziggurat_tables():
    """(X, F), 257 floats each: the recurrence of the 256-layer normal ziggurat, each entry sent through "%.18f" text as the crate's
    generated source is."""
    global _tables
    if _tables is None:
        def f(x):
            return math.exp(-x * x / 2.0)

        def f_inv(y):
            return math.sqrt(-2.0 * math.log(y))

        x = [ZIG_V / f(ZIG_R), ZIG_R]
        for i in range(2, 256):
            x.append(f_inv(ZIG_V / x[i - 1] + f(x[i - 1])))
        x.append(0.0)
        fx = [f(xi) for xi in x]
        _tables = ([float("%.18f" % xi) for xi in x], [float("%.18f" % fi) for fi in fx])
    return _tables


class NormalCounts:
    """Which paths StandardNormal took: fast accepts, wedge tests and their rejections, tail entries and the tail loop's rejections."""

    def __init__(self):
        self.fast = self.wedge = self.wedge_rejected = self.tail = self.tail_rejected = 0

    def as_dict(self):
        return dict(fast=self.fast, wedge=self.wedge, wedge_rejected=self.wedge_rejected, tail=self.tail, tail_rejected=self.tail_rejected)


_OPEN01_SUB = 1.0 - 2.0 ** -53
_EXP1024 = 1024 << 52
_EXP1023 = 1023 << 52


def _open01(rng):
    return from_bits(_EXP1023 | (rng.next_u64() >> 12)) - _OPEN01_SUB


def standard_normal(rng, counts=None):
    X, F = ziggurat_tables()
    c = counts if counts is not None else NormalCounts()
    while True:
        b = rng.next_u64()
        i = b & 0xff
        u = from_bits(_EXP1024 | (b >> 12)) - 3.0
        x = u * X[i]
        if abs(x) < X[i + 1]:
            c.fast += 1
            return x
        if i == 0:
            c.tail += 1
            while True:
                xx = math.log(_open01(rng)) / ZIG_R
                y = math.log(_open01(rng))
                if not -2.0 * y < xx * xx:
                    break
                c.tail_rejected += 1
            return xx - ZIG_R if u < 0.0 else ZIG_R - xx
        c.wedge += 1
        f01 = float(rng.next_u64() >> 11) * 2.0 ** -53
        if F[i + 1] + (F[i] - F[i + 1]) * f01 < math.exp(-x * x / 2.0):
            return x
        c.wedge_rejected += 1


def lognormal_params(mean, variance):
    mu = math.log(mean / math.sqrt(1.0 + variance / (mean * mean)))
    sigma = math.sqrt(math.log(1.0 + variance / (mean * mean)))
    return mu, sigma


def lognormal_delays(seed, mean, variance, n, counts=None, rng_out=None):
    """n delays of LogNormal(mean, variance) off a fresh Xoshiro(seed): exp(mu + sigma N) truncated toward zero."""
    mu, sigma = lognormal_params(mean, variance)
    rng = Xoshiro(seed)
    if rng_out is not None:
        rng_out.append(rng)
    return [int(math.exp(mu + sigma * standard_normal(rng, counts))) for _ in range(n)]


def uniform_delays(seed, lo, hi, n, rng_out=None):
    """n uniform integer delays in [lo, hi] off a fresh Xoshiro(seed)."""
    rng = Xoshiro(seed)
    if rng_out is not None:
        rng_out.append(rng)
    span = hi - lo + 1
    return [lo + rng.gen_range_u64(span) for _ in range(n)]
