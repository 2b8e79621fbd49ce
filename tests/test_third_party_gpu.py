"""The device's third-party arithmetic against tests/third_party_reference.py directly -- not through the oracle, which shares the
product's tables and exp / log source (tests/test_third_party_host.py holds the oracle to the same reference on the CPU):
 (a) lbft_device_sample_delays: log-normal rows whose first 20 000 normals reach the wedge rejection and the tail, and uniform rows up
     to the full span 2^63;
 (b) lbft_device_leaders over several 256-thread blocks with a partial last one, and for a single round;
 (c) lbft_device_exp_log at every branch boundary of lbft_exp / lbft_log, against the host libm point by point;
 (d) `python -m librabft_simulator_amd`, the reference's CLI on the HIP path, as a child process."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import third_party_cases as cases
import third_party_reference as ref
from support import amd  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DELAYS = 20000  # the sampling kernel runs on one lane


def device_delays(amd, delay, seed, n):
    from librabft_simulator_amd import _lib
    from librabft_simulator_amd.simulator import make_config
    cfg = make_config(3, delay, amd.NodeConfig())
    out = np.full(n, -1, dtype=np.int64)
    _lib.check(_lib.lib().lbft_device_sample_delays(0, ctypes.byref(cfg), seed, out.ctypes.data, n))
    return [int(v) for v in out]


# ---- (a) delays ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed,mean,variance", cases.LOGNORMAL_ROWS)
def test_device_lognormal_delays(amd, seed, mean, variance):
    """Measured with the reference, first 20 000 normals: seed 99 takes 298 wedge tests (134 rejected) and enters the tail 5 times;
    seed 2^64 - 1 takes 317 (133 rejected) and 5; seed 12776 (third_party_cases.TAIL_SEED) enters the tail 3 times in its first
    2 000.  So every row decides samples by the exact exp of the wedge test and by the log of the tail loop, not only by the fast
    path, and the two wide rows carry the normal's last bits into the delay."""
    want, c, _ = cases.lognormal(seed, mean, variance, N_DELAYS)
    assert c["tail"] >= 1 and c["wedge_rejected"] >= 1, c
    got = device_delays(amd, amd.RandomDelay.new(mean, variance), seed, N_DELAYS)
    bad = [i for i in range(N_DELAYS) if got[i] != want[i]]
    assert bad == [], (bad[:5], [got[i] for i in bad[:5]], [want[i] for i in bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", cases.UNIFORM_ROWS + ((0, 2 ** 63 - 1),))  # the last: span 2^63, no leading zero to shift out
def test_device_uniform_delays(amd, lo, hi):
    rng = []
    want = ref.uniform_delays(cases.UNIFORM_SEED, lo, hi, N_DELAYS, rng)
    print("span %d: %d rejections in %d draws" % (hi - lo + 1, rng[0].rejects_u64, rng[0].draws))
    assert device_delays(amd, amd.RandomDelay.uniform(lo, hi), cases.UNIFORM_SEED, N_DELAYS) == want


# ---- (b) leaders -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wi", range(len(cases.WEIGHTS)), ids=[cases.weights_id(w) for w in cases.WEIGHTS])
def test_device_leaders(amd, wi):
    from librabft_simulator_amd import _lib
    L = _lib.lib()
    w = cases.WEIGHTS[wi]
    wa = np.array(w, dtype=np.uint64)
    want, _ = cases.leaders(wi, 1000)
    for n_rounds in (1000, 1):  # three full blocks and a partial one; a single thread's worth
        out = np.full(n_rounds + 8, 0xee, dtype=np.uint8)
        _lib.check(L.lbft_device_leaders(0, wa.ctypes.data, len(w), out.ctypes.data, n_rounds))
        assert [int(v) for v in out[:n_rounds]] == want[:n_rounds], n_rounds
        assert (out[n_rounds:] == 0xee).all()
    if all(v == 1 for v in w):  # (NULL rights = all 1)
        out = np.zeros(1000, dtype=np.uint8)
        _lib.check(L.lbft_device_leaders(0, None, len(w), out.ctypes.data, 1000))
        assert [int(v) for v in out] == want


# ---- (c) exp / log at the branch boundaries ---------------------------------------------------------------------------------------
def as_bits(a):
    return [int(v) for v in np.asarray(a, dtype=np.float64).view(np.uint64)]


@pytest.mark.gpu
def test_device_exp_log_branch_boundaries(amd, oracle):
    from librabft_simulator_amd import _lib
    inf, nan = math.inf, math.nan
    log_x = [ref.from_bits(b) for b in cases.log_points()]
    exp_x = cases.exp_points()
    log_special = [(0.0, -inf), (-0.0, -inf), (-1.5, nan), (ref.from_bits(0x8000000000000001), nan), (-inf, nan), (inf, inf), (nan, nan)]
    exp_special = [(inf, inf), (-inf, 0.0), (nan, nan), (709.79, inf), (-745.14, 0.0)]
    beyond = list(cases.EXP_BEYOND_512)
    x = np.array(log_x + exp_x + [v for v, _ in log_special] + [v for v, _ in exp_special] + beyond, dtype=np.float64)
    assert len(log_x) == 1099 and len(exp_x) == 126 and len(x) % 256 != 0 and len(x) > 4 * 256
    e, l = np.full(len(x), 123.0), np.full(len(x), 123.0)
    _lib.check(_lib.lib().lbft_device_exp_log(0, x.ctypes.data, e.ctypes.data, l.ctypes.data, len(x)))
    o = 0
    got = as_bits(l[o:o + len(log_x)])
    bad = [(log_x[i].hex(), hex(got[i]), math.log(log_x[i]).hex()) for i in range(len(log_x)) if got[i] != ref.bits(math.log(log_x[i]))]
    assert bad == [], (len(bad), bad[:5])
    o += len(log_x)
    got = as_bits(e[o:o + len(exp_x)])
    bad = [(exp_x[i].hex(), hex(got[i]), math.exp(exp_x[i]).hex()) for i in range(len(exp_x)) if got[i] != ref.bits(math.exp(exp_x[i]))]
    assert bad == [], (len(bad), bad[:5])
    o += len(exp_x)
    for k, (v, want) in enumerate(log_special):
        g = float(l[o + k])
        assert (math.isnan(g) if math.isnan(want) else ref.bits(g) == ref.bits(want)), ("log", v, g)
    o += len(log_special)
    for k, (v, want) in enumerate(exp_special):
        g = float(e[o + k])
        assert (math.isnan(g) if math.isnan(want) else ref.bits(g) == ref.bits(want)), ("exp", v, g)
    o += len(exp_special)
    OL = oracle.lib()
    for k, v in enumerate(beyond):  # the same source under g++: deterministic there, not correctly rounded, so no libm claim
        assert 512.0 <= abs(v) <= 708.0
        assert ref.bits(float(e[o + k])) == ref.bits(OL.lbft_oracle_exp_strict(v)), v
    assert o + len(beyond) == len(x)


# ---- (d) the CLI ------------------------------------------------------------------------------------------------------------------
def run_cli(*args):
    """A fresh child process, as a user starts it: from the repository's root, nothing else on the path."""
    p = subprocess.run([sys.executable, "-m", "librabft_simulator_amd", *args], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout, p.stderr


@pytest.mark.gpu
def test_cli_reproduces_the_reference_goldens(amd):
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as fh:
        golden = json.load(fh)
    out, err = run_cli("--seed", "52", "--nodes", "3")
    assert out == "Commands executed per node: [27, 27, 27]\n"
    assert golden["simulated_run_3_nodes"]["commits"] == [27, 27, 27] and "seed: 52" in err
    out, _ = run_cli("--seed", "48", "--nodes", "8")
    assert out == "Commands executed per node: %s\n" % golden["simulated_run_8_nodes"]["commits"]


@pytest.mark.gpu
def test_cli_batch_of_instances(amd):
    out, _ = run_cli("--seed", "52", "--nodes", "3", "--instances", "3")
    lines = out.splitlines()
    assert lines[0] == "Commands executed per node (instance 0): [27, 27, 27]"
    assert len(lines) == 2 and lines[1].startswith("instances 3: rounds ")
