"""What more than one test module uses: the fixtures that load the package and its libraries, the oracle's configuration of a parameter
set, small helpers of the statistics tests, and the g++ build of a host shim.  A plain module: tests import what they use, fixtures by
name (they keep their module scope)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import librabft_simulator_amd as L
    L.lib()  # fails loudly if liblbft_hip.so is missing
    return L


@pytest.fixture(scope="module")
def hiplib():
    from librabft_simulator_amd import build
    build.build()
    from librabft_simulator_amd import _lib
    return _lib


def other_libs(tag):
    """The files of every library of build.TABLE but `tag`'s: where its launchers and kernels must not be."""
    from librabft_simulator_amd import build
    return [lib.out for lib in build.TABLE if lib.tag != tag]


class Stub:  # (no batch behind it: the checks run before any library call)
    _h, _max_clock, param_sets, num_instances, num_nodes = None, 1000, None, 1, 4


def oracle_cfg(oc, n, ps, **kw):
    """The oracle's configuration of parameter set `ps`; kw: quirks, voting_rights, equivocate_every, commands_per_epoch, rights_rotation."""
    d, nc = ps.network_delay, ps.node_config
    part = ps.partition or (0, 0, 0)
    return oc.make_config(num_nodes=n, mean=d.mean, variance=d.variance, delay_model=d.model, uniform_lo=d.lo, uniform_hi=d.hi,
                          target_commit_interval=nc.target_commit_interval, delta=nc.delta, gamma=nc.gamma, lambda_=nc.lambda_,
                          drop_per_million=ps.drop_per_million, partition_size=part[0], partition_start=part[1], partition_end=part[2],
                          math_mode=1, **kw)


def set_oracle_cfg(oc, base, s, rights=None):
    """The oracle's configuration of the set struct `s` of a batch whose lbft_config is `base` (the host models' form)."""
    return oc.make_config(num_nodes=base.num_nodes, mean=s.mean, variance=s.variance, delay_model=base.delay_model, uniform_lo=s.uniform_lo,
                          uniform_hi=s.uniform_hi, commands_per_epoch=base.commands_per_epoch, target_commit_interval=s.target_commit_interval,
                          delta=s.delta, gamma=s.gamma, lambda_=s.lambda_, quirks=base.quirks, equivocate_every=base.equivocate_every,
                          drop_per_million=s.drop_per_million, partition_size=s.partition_size, partition_start=s.partition_start,
                          partition_end=s.partition_end, voting_rights=rights)


def plain(amd, seeds, n, ps, **kw):
    return amd.BatchSimulator.new(np.asarray(seeds, dtype=np.uint64), n, ps.network_delay, ps.node_config, drop_per_million=ps.drop_per_million,
                                  partition=ps.partition, **kw)


def binning(max_clock, width, bins):
    """latency_histogram's defaults: width 1 up to 65 536 bins, above that the smallest width that fits."""
    span = max_clock + 1
    if width is None:
        width = -(-span // bins) if bins else max(1, -(-span // (1 << 16)))
    if bins is None:
        bins = -(-span // width)
    return width, bins


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def run_to_end(sim, max_clock, cut):
    launches = 0
    while True:
        left, res = sim.run_steps(max_clock, cut)
        launches += 1
        assert launches < 200000
        if left == 0:
            return res


def build_shim(tmp_dir, source, name, *extra_flags):
    """Compiles tests/`source` with g++ into the shared object `name` in `tmp_dir` -> its CDLL (the caller binds argtypes / restype)."""
    out = str(tmp_dir / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", *extra_flags, os.path.join(TESTS, source), "-o", out])
    return ctypes.CDLL(out)
