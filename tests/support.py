"""What more than one test module uses: the fixtures that load the package and its libraries, the oracle's configuration of a parameter
set, small helpers of the statistics tests, the comparisons of the grouped device statistics with their numpy references, and the g++
build of a host shim.  A plain module: tests import what they use, fixtures by name (they keep their module scope)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chain_stats_reference
import commit_finality_reference
import round_stats_reference

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


def device_batch(amd, kw, seeds, **extra):
    """The plain device batch of an oracle configuration `kw` (the reference CLI defaults for everything else)."""
    kw = dict(kw)
    n = kw.pop("num_nodes")
    delay = amd.RandomDelay.new(kw.pop("mean", 10.0), kw.pop("variance", 4.0))
    node = amd.NodeConfig(kw.pop("target_commit_interval", 100000), kw.pop("delta", 20), 2.0, 0.5)
    part = (kw.pop("partition_size"), kw.pop("partition_start"), kw.pop("partition_end")) if "partition_size" in kw else None
    ps = amd.ParamSet(delay, node, drop_per_million=kw.pop("drop_per_million", 0), partition=part)
    return plain(amd, np.asarray(list(seeds), dtype=np.uint64), n, ps, **kw, **extra)


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


def check_chain_stats(res, want, max_clock, binnings=((None, None),), set_of=None, groups=1, faults=None, log_capacity=None):
    """chain_stats() for every (width, bins) of `binnings` (None = the default) equals the reference on the oracle's histories, commit
    counts and startup times.  Returns the reference's sample families and author counts and what the last binning gave."""
    ref = chain_stats_reference
    histories, counts, startup = want
    n = counts.shape[1]
    fam, authors_o = ref.samples(histories, counts, startup, faults, set_of, groups, log_capacity)
    for width, bins in binnings:
        hist, authors, stats = res.chain_stats(width, bins)
        w, b = binning(max_clock, width, bins)
        assert hist.shape == (groups, b) and authors.shape == (groups, n) and stats.shape == (groups, ref.CHAIN_STATS), (width, bins)
        assert hist.dtype == authors.dtype == stats.dtype == np.uint64
        want_hist, want_authors, want_stats = ref.bin_chain(fam, authors_o, w, b)
        print("binning (%s, %s): stats %s authors %s" % (width, bins, stats.tolist(), authors.tolist()))
        assert (stats == want_stats).all(), (width, bins, stats, want_stats)
        assert (authors == want_authors).all(), (width, bins, authors, want_authors)
        assert (hist == want_hist).all(), (width, bins)
        assert (hist.sum(axis=1) == stats[:, 0]).all() and (authors.sum(axis=1) == stats[:, 4 * ref.LENGTH + 1]).all()
    assert all(row["agreement"] is True for row in res.chain_by_param_set())
    return fam, authors_o, hist, authors, stats


def check_finality(res, max_clock, binnings=((None, None),), want=None, **kw):
    """finality_histogram() for every (width, bins) of `binnings` (None = the default) equals the reference: `want` = (families, first
    committers), or else the reference on the batch's own read-backs (kw: rights, rotation, commands_per_epoch, set_of, groups,
    log_capacity).  Returns the reference's families and what the last binning gave."""
    ref = commit_finality_reference
    fam, fc = want if want is not None else ref.of_result(res, **kw)
    groups, n = len(fam), fc.shape[1]
    for width, bins in binnings:
        fin, spread, first, stats = res.finality_histogram(width, bins)
        w, b = binning(max_clock, width, bins)
        assert fin.shape == spread.shape == (groups, b) and first.shape == (groups, n) and stats.shape == (groups, ref.FINALITY_STATS), (width, bins)
        assert fin.dtype == spread.dtype == first.dtype == stats.dtype == np.uint64
        want_fin, want_spread, want_first, want_stats = ref.bin_finality(fam, fc, w, b, max_clock)
        print("binning (%s, %s): stats %s first %s" % (width, bins, stats.tolist(), first.tolist()))
        assert (stats == want_stats).all(), (width, bins, stats, want_stats)
        assert (first == want_first).all(), (width, bins, first, want_first)
        assert (fin == want_fin).all() and (spread == want_spread).all(), (width, bins)
        assert (fin.sum(axis=1) == stats[:, 4 * ref.QUORUM]).all() and (spread.sum(axis=1) == stats[:, 4 * ref.SPREAD]).all()
        assert (first.sum(axis=1) == stats[:, 4 * ref.FIRST]).all()  # a group's row sums to family 0's sample count
    return fam, fin, spread, first, stats


def check_round_tables(res, want, clean=None):
    """round_tables() is the oracle's tables: max_rounds, messages and every cell, for every instance (`clean`: for those instances)."""
    ref = round_stats_reference
    tables_o, max_rounds_o, messages_o = want
    tables, max_rounds, messages = res.round_tables()
    sel = slice(None) if clean is None else clean
    assert tables.dtype == np.int64 and max_rounds.dtype == messages.dtype == np.uint64
    assert (max_rounds[sel] == max_rounds_o[sel]).all() and (messages[sel] == messages_o[sel]).all()
    rows = tables_o.shape[1]
    assert tables[sel].shape[1] >= int(max_rounds_o[sel].max()) and (tables[sel][:, rows:] == ref.EMPTY).all()
    assert (tables[sel][:, :rows] == tables_o[sel][:, :tables.shape[1]]).all()
    return tables, max_rounds, messages


def check_round_histograms(res, want, max_clock, binnings, set_of=None, groups=1):
    """round_histogram() for every (width, bins) of `binnings` (None = the default) equals the reference on the tables `want` (the
    oracle's, or the device's own read-back) and the device's fault words.  Returns the reference's sample families and what the last
    binning gave."""
    ref = round_stats_reference
    tables_o, max_rounds_o, _ = want
    fam = ref.samples(tables_o, max_rounds_o, res.faults, set_of, groups)
    for width, bins in binnings:
        stay, skew, stats = res.round_histogram(width, bins)
        w, b = binning(max_clock, width, bins)
        assert stay.shape == skew.shape == (groups, b) and stats.shape == (groups, 16), (width, bins)
        assert stay.dtype == skew.dtype == stats.dtype == np.uint64
        want_stay, want_skew, want_stats = ref.bin_rounds(fam, w, b)
        print("binning (%s, %s): stats %s" % (width, bins, stats.tolist()))
        assert (stats == want_stats).all(), (width, bins, stats, want_stats)
        assert (stay == want_stay).all() and (skew == want_skew).all(), (width, bins)
        assert (stay.sum(axis=1) == stats[:, 4 * ref.STAY]).all() and (skew.sum(axis=1) == stats[:, 4 * ref.SKEW]).all()
    return fam, stay, skew, stats


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


def build_pool_walk_shim(tmp_dir, source, name, prefix):
    """A host model over tests/pool_walk_host.h (symbol prefix `prefix`: vtm, epm, rhm) with the accessors they share bound; the caller
    binds its own walk and counts."""
    L = build_shim(tmp_dir, source, name, "-ffp-contract=off", "-pthread", "-w")
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    sym = lambda what: getattr(L, "%s_%s" % (prefix, what))
    sym("create").argtypes, sym("create").restype = [vp, vp, ctypes.c_size_t, ctypes.c_int64, u32, vp], vp
    sym("destroy").argtypes = [vp]
    sym("log").argtypes, sym("log").restype = [vp, u32, u32, u32, ctypes.c_int, u32], u32
    sym("set_fault").argtypes = [vp, u32, u32]
    if prefix != "rhm":
        sym("chain").argtypes = [vp, u32, vp, vp]
    L.pw_chain_entries.argtypes, L.pw_chain_entries.restype = [vp, u32, u32, vp, u32, vp], u32
    L.pw_cut.argtypes = [vp, u32, u32]
    return L


class ModelBase:
    """A plain batch run on the host and kept in a handle of a pool-walk shim: the configuration (the reference CLI defaults, `kw` on
    top), the accessors the three models share.  A subclass sets PREFIX and WIDTHS and has its own walk and counts."""
    PREFIX, WIDTHS = None, (1, 7, 64)

    def __init__(self, L, kw, max_clock, seeds):
        from librabft_simulator_amd import _lib
        self.L, self.max_clock = L, max_clock
        cfg = _lib.LbftConfig()
        defaults = dict(mean=10.0, variance=4.0, commands_per_epoch=30000, target_commit_interval=100000, delta=20, gamma=2.0, lambda_=0.5)
        for k, v in {**defaults, **kw}.items():
            if k == "voting_rights":
                self._rights = np.ascontiguousarray(v, dtype=np.uint64)
                cfg.voting_rights = self._rights.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
            else:
                setattr(cfg, k, v)
        info = np.zeros(4, dtype=np.uint32)
        seeds = np.ascontiguousarray(list(seeds), dtype=np.uint64)
        self.h = self.sym("create")(ctypes.byref(cfg), seeds.ctypes.data, len(seeds), max_clock, 4, info.ctypes.data)
        assert self.h, "the host model refused the configuration"
        self.m = len(seeds)
        self.n, self.lcap, self.bcap, self.cls = (int(x) for x in info)
        self.rights = kw.get("voting_rights")

    def sym(self, what):
        return getattr(self.L, "%s_%s" % (self.PREFIX, what))

    def chain(self, i):
        r, length = ctypes.c_uint32(), ctypes.c_uint32()
        self.sym("chain")(self.h, i, ctypes.byref(r), ctypes.byref(length))
        return r.value, length.value

    def log(self, i, q, k, value=None):
        return self.sym("log")(self.h, i, q, k, 0 if value is None else 1, 0 if value is None else value)

    def set_fault(self, i, value):
        self.sym("set_fault")(self.h, i, value)

    def same_for_every_width(self, **kw):
        got = [self.walk(W, **kw) for W in self.WIDTHS]
        for other in got[1:]:
            for a, b in zip(got[0], other):
                assert a.tobytes() == b.tobytes()
        return got[0]

    def close(self):
        self.sym("destroy")(self.h)
