"""Host-side mirror of the reference's simulator interface for the hot path, on top of the C ABI.

Reference surface mirrored here (names and argument meaning kept):
  * ``RandomDelay::new(mean, variance)``                       bft-lib/src/simulator.rs:98-107
  * ``GlobalTime(i64)``                                        bft-lib/src/simulator.rs:35-37
  * ``NodeConfig{target_commit_interval, delta, gamma, lambda}`` librabft-v2/src/node.rs:76-81
  * ``Simulator::new(rng_seed, num_nodes, network_delay, context_factory)`` and
    ``Simulator::loop_until(max_clock, csv_path) -> Vec<&Context>``  bft-lib/src/simulator.rs:200-250,380-475
  * ``SimulatedContext::committed_history()`` / ``last_committed_state()``
                                                               bft-lib/src/simulated_context.rs:98-100,194-196
``BatchSimulator`` is the batched form (many independent ``Simulator``s, one GPU lane each); it is
what the HIP path natively executes.  Everything computes on the GPU through liblbft_hip.so; there
is no CPU path in this package.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import CHAIN_HEAD_DTYPE, COMMIT_DTYPE, RECORD_HASH_DTYPE, LbftActions, LbftConfig, LbftCounters, LbftError, LbftNodeView, check

Command = namedtuple("Command", ["proposer", "index"])  # simulated_context.rs:31-35
Author = int


class NodeTime(int):
    """bft-lib/src/base_types.rs NodeTime(i64): a node's local clock (global time minus its startup time)."""

    def __repr__(self):
        return "NodeTime(%d)" % int(self)


class State(int):
    """simulated_context.rs:28-29: State(u64)."""

    def __repr__(self):
        return "State(%d)" % int(self)


class GlobalTime(int):
    """bft-lib/src/simulator.rs:35-37; the conversions of :120-126 (a node's startup time: ``BatchResult.startup_times``)."""

    def __repr__(self):
        return "GlobalTime(%d)" % int(self)

    def to_node_time(self, startup_time):
        return NodeTime(int(self) - int(startup_time))

    @classmethod
    def from_node_time(cls, node_time, startup_time):
        return cls(int(node_time) + int(startup_time))

    def __add__(self, duration):  # GlobalTime + Duration (simulator.rs:90-96)
        return GlobalTime(int(self) + int(duration))


class Duration(int):
    """bft-lib/src/base_types.rs Duration(i64)."""


class RandomDelay:
    """bft-lib/src/simulator.rs:39-43,98-107.  ``RandomDelay.new(mean, variance)`` is the reference's
    log-normal delay; ``RandomDelay.uniform(lo, hi)`` is this framework's integer-uniform extension."""

    def __init__(self, mean=10.0, variance=4.0, model=0, lo=0, hi=0):
        self.mean, self.variance, self.model, self.lo, self.hi = float(mean), float(variance), int(model), int(lo), int(hi)

    @classmethod
    def new(cls, mean, variance):
        return cls(mean, variance, 0)

    @classmethod
    def uniform(cls, lo, hi):
        return cls(10.0, 4.0, 1, lo, hi)


class NodeConfig:
    """librabft-v2/src/node.rs:76-81 (defaults = CLI defaults, librabft-v2/src/main.rs:111-134)."""

    def __init__(self, target_commit_interval=100000, delta=20, gamma=2.0, lambda_=0.5):
        self.target_commit_interval = int(target_commit_interval)
        self.delta = int(delta)
        self.gamma = float(gamma)
        self.lambda_ = float(lambda_)


class ParamSet:
    """One parameter set of a batch (``BatchSimulator.with_param_sets``): the delay, NodeConfig and loss settings its instances run;
    everything else is the batch's.  ``partition`` = (size of the first side, start, end) as in ``BatchSimulator``."""

    def __init__(self, network_delay=None, node_config=None, drop_per_million=0, partition=None):
        self.network_delay = network_delay or RandomDelay()
        self.node_config = node_config or NodeConfig()
        self.drop_per_million = int(drop_per_million)
        self.partition = None if partition is None else tuple(int(v) for v in partition)

    def to_struct(self):
        d, nc = self.network_delay, self.node_config
        s = _lib.LbftParamSet()
        s.mean, s.variance, s.uniform_lo, s.uniform_hi = d.mean, d.variance, d.lo, d.hi
        s.target_commit_interval, s.delta, s.gamma, s.lambda_ = nc.target_commit_interval, nc.delta, nc.gamma, nc.lambda_
        s.drop_per_million = self.drop_per_million
        if self.partition is not None:
            s.partition_size, s.partition_start, s.partition_end = self.partition
        return s


def make_config(num_nodes, network_delay, node_config, commands_per_epoch=30000, voting_rights=None,
                queue_capacity=0, snapshot_capacity=0, block_capacity=0, log_capacity=0, equivocate_every=0,
                drop_per_million=0, partition=None, quirks=0, rights_rotation=0):
    cfg = LbftConfig()
    cfg.num_nodes = num_nodes
    cfg.delay_model = network_delay.model
    cfg.mean = network_delay.mean
    cfg.variance = network_delay.variance
    cfg.uniform_lo = network_delay.lo
    cfg.uniform_hi = network_delay.hi
    cfg.commands_per_epoch = commands_per_epoch
    cfg.target_commit_interval = node_config.target_commit_interval
    cfg.delta = node_config.delta
    cfg.gamma = node_config.gamma
    cfg.lambda_ = node_config.lambda_
    cfg.quirks = int(quirks)
    cfg.equivocate_every = int(equivocate_every)
    cfg.drop_per_million = int(drop_per_million)
    cfg.rights_rotation = int(rights_rotation)  # extension: epoch e uses voting_rights[(i + e * rights_rotation) % n]
    if partition is not None:  # (size of the first side, start, end): nodes [0, size) are cut off during [start, end)
        cfg.partition_size, cfg.partition_start, cfg.partition_end = (int(v) for v in partition)
    cfg.queue_capacity = queue_capacity
    cfg.snapshot_capacity = snapshot_capacity
    cfg.block_capacity = block_capacity
    cfg.log_capacity = log_capacity
    if voting_rights is not None:
        arr = (C.c_uint64 * num_nodes)(*[int(w) for w in voting_rights])
        cfg._keepalive = arr
        cfg.voting_rights = C.cast(arr, C.POINTER(C.c_uint64))
    return cfg


def write_data_files(path, rows, messages, num_nodes):
    """DataWriter::write_to_file (bft-lib/src/data_writer.rs:62-97): ``round_switches.txt`` (header ``node i``, one
    row per round below the highest round reached, empty cells for rounds a node never entered) and
    ``number_of_messages.txt`` in directory ``path`` (created if missing, as DataWriter::new does)."""
    import os
    if not os.path.exists(path):
        os.mkdir(path)
    with open(os.path.join(path, "round_switches.txt"), "w") as f:
        f.write(",".join("node %d" % i for i in range(num_nodes)) + "\n")
        for row in rows:
            f.write(",".join("" if v is None else str(v) for v in row) + "\n")
    with open(os.path.join(path, "number_of_messages.txt"), "w") as f:
        f.write("%d\n" % messages)


def histogram_quantile(hist, width, q):
    """The q-quantile of the samples binned in ``hist`` (bin k = [k * width, (k + 1) * width)) by the inverted-CDF rule: the lower edge of
    the first bin whose cumulative count reaches ceil(q * N) (at least 1); None for an empty histogram."""
    cdf = np.cumsum(np.asarray(hist, dtype=np.uint64))
    n = int(cdf[-1]) if len(cdf) else 0
    if n == 0:
        return None
    target = max(1, int(np.ceil(q * n)))
    return int(np.searchsorted(cdf, target, side="left")) * int(width)


def _families(stats, families):
    """One group's device statistics -- (samples, sum, min, max) per family, in the order of ``families`` = ((name, count_key), ...) -- as
    ``{name: {count_key, mean, min, max}}``, ``None`` where a family has no samples."""
    out = {}
    for f, (name, count_key) in enumerate(families):
        n, total, lo, hi = (int(v) for v in stats[4 * f:4 * f + 4])
        out[name] = {count_key: n, "mean": total / n if n else None, "min": lo if n else None, "max": hi if n else None}
    return out


class BatchResult:
    """Results of ``BatchSimulator.loop_until`` (lazy device read-back through the C ABI)."""

    def __init__(self, sim):
        self._sim = sim
        self._cache = {}
        self._gen = getattr(sim, "_state_generation", 0)

    def _get(self, key, fn):
        # what was read back belongs to the device state it was read from: BatchSimulator.load_node rewrites a node's rows (pacemaker round,
        # epoch, certificates ...) after the run, and a result object created before it must not serve the pre-load values
        gen = getattr(self._sim, "_state_generation", 0)
        if gen != self._gen:
            self._cache.clear()
            self._gen = gen
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    @property
    def counters(self):
        def f():
            c = LbftCounters()
            check(_lib.lib().lbft_batch_counters(self._sim._h, C.byref(c)))
            return c.as_dict()
        return self._get("counters", f)

    def counters_allgather_reduce(self, nccl_comm):
        """The run's one collective, natively: ONE RCCL ncclAllGather of the fourteen counter words per rank over the caller's communicator
        (an ncclComm_t as an integer / ctypes pointer; every rank calls it), reduced locally -- sums and high-water marks.  Returns the
        aggregate as a dict."""
        c = LbftCounters()
        check(_lib.lib().lbft_batch_counters_allgather_reduce(self._sim._h, C.c_void_p(int(nccl_comm)), C.byref(c)))
        return c.as_dict()

    counters_allreduce = counters_allgather_reduce  # (the name through round 4)

    def _node_array(self, name, dtype):
        def f():
            out = np.zeros((self._sim.num_instances, self._sim.num_nodes), dtype=dtype)
            check(getattr(_lib.lib(), "lbft_batch_" + name)(self._sim._h, out.ctypes.data))
            return out
        return self._get(name, f)

    @property
    def commit_counts(self):
        """contexts.iter().map(|c| c.committed_history().len())  [instance, node]"""
        return self._node_array("commit_counts", np.uint32)

    @property
    def active_rounds(self):
        return self._node_array("active_rounds", np.uint64)

    @property
    def last_committed_states(self):
        return self._node_array("last_committed_states", np.uint64)

    @property
    def startup_times(self):
        return self._node_array("startup_times", np.int64)

    @property
    def epochs(self):
        return self._node_array("epochs", np.uint64)

    @property
    def faults(self):
        def f():
            out = np.zeros(self._sim.num_instances, dtype=np.uint32)
            check(_lib.lib().lbft_batch_faults(self._sim._h, out.ctypes.data))
            return out
        return self._get("faults", f)

    def committed_histories(self, cap_per_node=None):
        """[instance, node, k] structured array (proposer, index, time); entries past the node's
        commit count are zero."""
        if cap_per_node is None:
            cap_per_node = int(self.commit_counts.max()) if self._sim.num_instances else 0
        cap_per_node = max(int(cap_per_node), 1)
        out = np.zeros((self._sim.num_instances, self._sim.num_nodes, cap_per_node), dtype=COMMIT_DTYPE)
        check(_lib.lib().lbft_batch_committed_histories(self._sim._h, out.ctypes.data, cap_per_node))
        return out

    def committed_history(self, instance, node):
        n = int(self.commit_counts[instance, node])
        out = np.zeros(max(n, 1), dtype=COMMIT_DTYPE)
        ln = C.c_size_t()
        check(_lib.lib().lbft_batch_committed_history(self._sim._h, instance, node, out.ctypes.data, n, C.byref(ln)))
        return out[:n]

    def committed_record_hashes(self, instance, node):
        """(block_hash, state, qc_hash, num_votes, flags) of the Block_ / QuorumCertificate_ records behind
        committed_history(instance, node), hashed like the reference's SmrContext::hash (BCS + SipHash-1-3)."""
        n = int(self.commit_counts[instance, node])
        out = np.zeros(max(n, 1), dtype=RECORD_HASH_DTYPE)
        ln = C.c_size_t()
        check(_lib.lib().lbft_batch_committed_record_hashes(self._sim._h, instance, node, out.ctypes.data, n, C.byref(ln)))
        return out[:n]

    def chain_record_hashes(self, cap=None):
        """The record hashes of every instance's committed chain in one device call (lbft_batch_chain_record_hashes):
        ``(entries, heads, node_prefix)``.  An instance's chain is the log of its reference node, the lowest-numbered node with the most
        commits.  ``entries[instance, k]`` (RECORD_HASH_DTYPE) is entry k of ``committed_record_hashes(instance, ref_node)``, zero at and
        past the chain's length; ``heads[instance]`` (CHAIN_HEAD_DTYPE) the last entry with the chain's ``length`` and ``ref_node`` (all
        zero for an empty chain); ``node_prefix[instance, node]`` the number of leading entries of that node's history that are the
        chain's: where it equals ``commit_counts``, ``committed_record_hashes(instance, node)`` is ``entries[instance, :count]``.
        Instances with a fault are skipped (zeros).  ``cap=None``: as many entries as the longest chain has (at least 1)."""
        if cap is None:
            cap = int(self.commit_counts.max()) if self._sim.num_instances else 0
            cap = max(cap, 1)
        cap = int(cap)
        if cap < 1:
            raise ValueError("cap must be at least 1 (chain_heads() gives the heads alone)")
        m, n = self._sim.num_instances, self._sim.num_nodes
        entries = np.zeros((m, cap), dtype=RECORD_HASH_DTYPE)
        heads = np.zeros(m, dtype=CHAIN_HEAD_DTYPE)
        prefix = np.zeros((m, n), dtype=np.uint32)
        check(_lib.lib().lbft_batch_chain_record_hashes(self._sim._h, entries.ctypes.data, cap, heads.ctypes.data, prefix.ctypes.data))
        return entries, heads, prefix

    def chain_heads(self):
        """``heads`` of ``chain_record_hashes`` alone: 40 bytes per instance, whose ``qc_hash`` -- the hash of the last
        QuorumCertificate_ of the chain -- commits to every block, state and vote below it."""
        heads = np.zeros(self._sim.num_instances, dtype=CHAIN_HEAD_DTYPE)
        check(_lib.lib().lbft_batch_chain_record_hashes(self._sim._h, None, 0, heads.ctypes.data, None))
        return heads

    def save_node(self, instance, node):
        """ConsensusNode::save_node (librabft-v2/src/node.rs:233-238): bincode image of the node's NodeState (bytes), HashMaps in
        ascending key order; what the reference's load_node (node.rs:211-231) deserialises."""
        return self._sim.save_node(instance, node)

    def round_switches(self, instance=0, cap_rounds=None):
        """DataWriter output of one instance (bft-lib/src/data_writer.rs): (rows, number_of_messages) where
        rows[round][node] is the GlobalTime at which the node was first seen in that round or None (empty cell)."""
        cap = int(cap_rounds or 1 << 16)
        n = self._sim.num_nodes
        mr, msgs = C.c_uint64(), C.c_uint64()
        out = np.full((min(cap, 1 << 16), n), np.iinfo(np.int64).min, dtype=np.int64)
        check(_lib.lib().lbft_batch_round_switches(self._sim._h, int(instance), out.ctypes.data, out.shape[0], C.byref(mr), C.byref(msgs)))
        lo = np.iinfo(np.int64).min
        rows = [[None if v == lo else int(v) for v in out[r]] for r in range(min(int(mr.value), out.shape[0]))]
        return rows, int(msgs.value)

    def round_tables(self, cap_rounds=None):
        """The DataWriter tables of every instance in one read-back (lbft_batch_round_switches_all): ``(tables, max_rounds, messages)``,
        ``tables[instance, round, node]`` int64 = the GlobalTime at which the node was first seen in that round, ``INT64_MIN`` = empty
        cell; instance i's table is the rows below ``min(max_rounds[i], cap_rounds)``, everything past them is empty; ``messages[i]`` is
        its number_of_messages.  For every instance what ``round_switches(i)`` gives.  ``cap_rounds=None``: as many rows as the longest
        table has (at least 1).  Needs a run with the round trace (``loop_until(..., round_trace=N)``)."""
        if cap_rounds is not None and int(cap_rounds) < 0:
            raise ValueError("cap_rounds must be at least 0")
        m, n = self._sim.num_instances, self._sim.num_nodes
        max_rounds = np.zeros(m, dtype=np.uint64)
        messages = np.zeros(m, dtype=np.uint64)
        if cap_rounds is None:  # (a call without rows reads max_rounds alone: it sizes the tables)
            check(_lib.lib().lbft_batch_round_switches_all(self._sim._h, None, 0, max_rounds.ctypes.data, None))
            cap = max(int(max_rounds.max()) if m else 0, 1)
        else:
            cap = int(cap_rounds)
        tables = np.full((m, cap, n), np.iinfo(np.int64).min, dtype=np.int64)
        check(_lib.lib().lbft_batch_round_switches_all(self._sim._h, tables.ctypes.data, cap, max_rounds.ctypes.data, messages.ctypes.data))
        return tables, max_rounds, messages

    def round_histogram(self, bin_width=None, bins=None):
        """Round statistics computed on the device from the round trace (lbft_batch_round_stats), per group (the parameter sets of a
        ``with_param_sets`` batch, else one group): ``(stay_hist, skew_hist, stats)``.  ``stay_hist[group, min(stay // bin_width, bins - 1)]``
        counts, for every node, the times between consecutive rounds it was recorded in; ``skew_hist`` the span between the first and
        the last node entering a round, per (instance, round) that at least two nodes entered; ``stats[group]`` (16 uint64) holds
        ``(samples, sum, min, max)`` of four families: ``stay``, ``skipped`` (the rounds a node jumped over between two recorded
        rounds), ``skew`` and ``reach`` (the number of nodes that entered a round, per (instance, round >= 1)).  Rows are the rounds
        below the highest round an instance reached (the DataWriter's table); instances with a fault are skipped.  Groups and default
        binning as ``latency_histogram``.  Needs a run with the round trace (``loop_until(..., round_trace=N)``)."""
        bin_width, bins = self._binning(bin_width, bins)
        groups = self._groups()
        stay = np.zeros((groups, bins), dtype=np.uint64)
        skew = np.zeros((groups, bins), dtype=np.uint64)
        stats = np.zeros((groups, _lib.ROUND_STATS), dtype=np.uint64)
        check(_lib.lib().lbft_batch_round_stats(self._sim._h, bin_width, bins, stay.ctypes.data, skew.ctypes.data, stats.ctypes.data))
        return stay, skew, stats

    def rounds_by_param_set(self, quantiles=(0.5, 0.9, 0.99)):
        """Per group of ``round_histogram`` (default, exact binning), in set order: ``stay`` and ``skew`` = samples, mean, min, max and
        ``quantiles`` ({str(q): ticks}, the inverted-CDF rule of ``histogram_quantile``), ``skipped`` and ``reach`` = samples, mean, min,
        max.  ``None`` where there are no samples."""
        width, _ = self._binning(None, None)
        stay, skew, stats = self.round_histogram()
        out = []
        for g in range(stay.shape[0]):
            row = {"set": g, **_families(stats[g], (("stay", "samples"), ("skipped", "samples"), ("skew", "samples"), ("reach", "samples")))}
            row["stay"]["quantiles"] = {str(q): histogram_quantile(stay[g], width, q) for q in quantiles}
            row["skew"]["quantiles"] = {str(q): histogram_quantile(skew[g], width, q) for q in quantiles}
            out.append(row)
        return out

    def chain_stats(self, bin_width=None, bins=None):
        """Statistics of the committed chain computed on the device (lbft_batch_chain_stats), per group (the parameter sets of a
        ``with_param_sets`` batch, else one group): ``(interval_hist, author_blocks, stats)``.  An instance's chain is the log of its
        reference node, the lowest-numbered node with the most commits; a chain entry's proposal time is
        ``startup_times[proposer] + time``.  ``interval_hist[group, min(interval // bin_width, bins - 1)]`` counts the times between the
        proposals of consecutive chain entries; ``author_blocks[group, a]`` the chain entries proposed by node ``a``; ``stats[group]``
        (24 uint64) holds ``(samples, sum, min, max)`` of six families: ``interval``, ``length`` (chain entries, per instance), ``lag``
        (chain length - a node's commits, per (instance, node)), ``tenure`` (consecutive chain entries of one proposer, per run),
        ``differing`` (per instance, the entries of all its nodes' histories that are not the chain's entry at that place: a sum of 0
        means that every history is a prefix of the chain) and ``inversions`` (per instance, the chain entries proposed before their
        predecessor; their interval counts as 0).  Instances with a fault are skipped.  Needs nothing of the run: no commit times, no
        round trace.  Groups and default binning as ``latency_histogram``."""
        bin_width, bins = self._binning(bin_width, bins)
        groups = self._groups()
        hist = np.zeros((groups, bins), dtype=np.uint64)
        authors = np.zeros((groups, self._sim.num_nodes), dtype=np.uint64)
        stats = np.zeros((groups, _lib.CHAIN_STATS), dtype=np.uint64)
        check(_lib.lib().lbft_batch_chain_stats(self._sim._h, bin_width, bins, hist.ctypes.data, authors.ctypes.data, stats.ctypes.data))
        return hist, authors, stats

    def chain_by_param_set(self, quantiles=(0.5, 0.9, 0.99)):
        """Per group of ``chain_stats`` (default, exact binning), in set order: ``interval`` = samples, mean, min, max and ``quantiles``
        ({str(q): ticks}, the inverted-CDF rule of ``histogram_quantile``); ``length``, ``differing`` and ``inversions`` = instances, mean,
        min, max; ``lag`` = nodes, mean, min, max; ``tenure`` = runs, mean, min, max; ``authors``, the chain blocks per proposer, and
        ``author_share``, their fractions of the group's chain blocks (``None`` when it has none); ``agreement``: every history is a prefix
        of its instance's chain and no chain goes back in time.  ``None`` where there are no samples."""
        width, _ = self._binning(None, None)
        hist, authors, stats = self.chain_stats()
        out = []
        for g in range(hist.shape[0]):
            row = {"set": g, **_families(stats[g], (("interval", "samples"), ("length", "instances"), ("lag", "nodes"), ("tenure", "runs"),
                                                    ("differing", "instances"), ("inversions", "instances")))}
            row["interval"]["quantiles"] = {str(q): histogram_quantile(hist[g], width, q) for q in quantiles}
            counts = [int(v) for v in authors[g]]
            blocks = sum(counts)
            row["authors"] = counts
            row["author_share"] = [c / blocks for c in counts] if blocks else None
            row["agreement"] = int(stats[g, 4 * 4 + 1]) == 0 and int(stats[g, 4 * 5 + 1]) == 0
            out.append(row)
        return out

    def _load_call(self, family, bin_width, bins):
        groups = self._groups()
        hist = np.zeros((groups, bins), dtype=np.uint64)
        faults = np.zeros((groups, 32), dtype=np.uint64)
        stats = np.zeros((groups, _lib.LOAD_STATS), dtype=np.uint64)
        caps = np.zeros(len(_lib.LOAD_CAPS), dtype=np.uint32)
        check(_lib.lib().lbft_batch_load_stats(self._sim._h, family, bin_width, bins, hist.ctypes.data, faults.ctypes.data, stats.ctypes.data,
                                               caps.ctypes.data))
        return hist, faults, stats, caps

    def load_stats(self, family="queue", bin_width=None, bins=None):
        """The run load computed on the device (lbft_batch_load_stats), per group (the parameter sets of a ``with_param_sets`` batch, else
        one group): ``(hist, faults, stats, caps)``.  Every instance gives one sample to each of the sixteen families of
        ``LOAD_FAMILIES``: the events by kind (``notifications``, ``requests``, ``responses``, ``timers``), ``messages`` (the first three
        added), ``scheduled``, ``draws``, ``folded``, ``updates``, the high-water marks ``queue``, ``chunks`` (the calendar queue's pool; 0
        without it), ``snapshots``, the number of ``blocks``, ``log`` (the largest commit count of its nodes), ``commits`` and ``rounds``
        (the smallest).  ``stats[group]`` (64 uint64) holds ``(samples, sum, min, max)`` per family over the instances without a fault;
        ``hist[group, min(sample // bin_width, bins - 1)]`` bins ``family`` (a name or an index) of the same instances;
        ``faults[group, k]`` counts every instance of the group with fault bit ``k``; ``caps`` (5 uint32) are the capacities the batch
        runs with, in the order of ``LOAD_CAPS``: the denominators of ``queue``, ``chunks``, ``snapshots``, ``blocks`` and ``log``.  The
        defaults are exact: width 1, and as many bins as the family's largest sample needs (found by a first call with one bin).  Needs
        nothing of the run: no commit times, no round trace; serves every kind of batch."""
        names = _lib.LOAD_FAMILIES
        f = names.index(family) if family in names else family
        if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or not 0 <= int(f) < len(names):
            raise ValueError("family: one of %s, or its index" % ", ".join(names))
        if (bin_width is not None and int(bin_width) < 1) or (bins is not None and int(bins) < 1):
            raise ValueError("bin_width and bins must be at least 1")
        f, bin_width = int(f), 1 if bin_width is None else int(bin_width)
        if bins is None:
            bins = int(self._load_call(f, bin_width, 1)[2][:, 4 * f + 3].max()) // bin_width + 1
        return self._load_call(f, bin_width, int(bins))

    def instance_load(self):
        """``[instances, 16]`` uint32: the sixteen samples of ``load_stats`` (columns in the order of ``LOAD_FAMILIES``) of every instance,
        faulted ones included -- with ``faults``, the rows to size a capacity by (lbft_batch_instance_load)."""
        rows = np.zeros((self._sim.num_instances, len(_lib.LOAD_FAMILIES)), dtype=np.uint32)
        check(_lib.lib().lbft_batch_instance_load(self._sim._h, rows.ctypes.data))
        return rows

    def load_by_param_set(self, quantiles=(0.5, 0.9, 0.99)):
        """Per group of ``load_stats`` (parameter set, or the one group of a plain batch), in set order: ``instances`` and ``clean``
        (those without a fault); per family ``{mean, min, max}`` over the clean instances (``None`` without any);
        ``messages_per_commit`` = sum(messages) / sum(commits), and the same for ``notifications``, ``requests`` and ``responses``
        (``None`` without commits); ``headroom`` = {capacity name: largest high-water mark / capacity} for ``LOAD_CAPS`` over the clean
        instances (``None`` for a capacity of 0 -- ``chunks`` without the calendar queue -- and for a group without a clean instance); ``queue_quantiles`` ({str(q): slots}, exact, the inverted-CDF rule of
        ``histogram_quantile``); ``faults`` = {fault name: instances}, over every instance of the group; ``worst_seed`` = for ``queue``
        and ``chunks`` the seed of the group's instance with the largest value, faulted instances included (``None`` for an empty
        group): the seed to replay in ``Simulator.new``."""
        names = _lib.LOAD_FAMILIES
        hist, faults, stats, caps = self.load_stats("queue")
        rows = self.instance_load()
        set_of = getattr(self._sim, "set_of_instance", None) if self._sim.param_sets is not None else None
        seeds = np.asarray(self._sim.seeds, dtype=np.uint64)
        out = []
        for g in range(hist.shape[0]):
            members = np.arange(len(rows)) if set_of is None else np.flatnonzero(set_of == g)
            fam = _families(stats[g], tuple((name, "instances") for name in names))
            row = {"set": g, "instances": int(len(members)), "clean": int(stats[g, 0])}
            for name in names:
                row[name] = {k: fam[name][k] for k in ("mean", "min", "max")}
            commits = int(stats[g, 4 * names.index("commits") + 1])
            for name in ("messages", "notifications", "requests", "responses"):
                row[name + "_per_commit"] = int(stats[g, 4 * names.index(name) + 1]) / commits if commits else None
            row["headroom"] = {name: (int(stats[g, 4 * names.index(name) + 3]) / int(cap) if cap and row["clean"] else None)
                               for name, cap in zip(_lib.LOAD_CAPS, caps)}
            row["queue_quantiles"] = {str(q): histogram_quantile(hist[g], 1, q) for q in quantiles}
            row["faults"] = {_lib.FAULT_NAMES.get(1 << k, "bit_%d" % k): int(c) for k, c in enumerate(faults[g]) if c}
            row["worst_seed"] = {name: (int(seeds[members[np.argmax(rows[members, names.index(name)])]]) if len(members) else None)
                                 for name in ("queue", "chunks")}
            out.append(row)
        return out

    def vote_stats(self, bin_width=None, bins=None):
        """Vote statistics computed on the device (lbft_batch_vote_stats), per group (the parameter sets of a ``with_param_sets`` batch,
        else one group): ``(margin_hist, votes_hist, node_table, stats)``.  An instance's chain is that of ``chain_stats``; its pool is
        every block proposed.  ``stats[group]`` (32 uint64) holds ``(samples, sum, min, max)`` of the eight families of
        ``VOTE_FAMILIES``: per chain entry with a quorum certificate its ``votes``, their ``weight`` in the voting rights of the block's
        epoch and the ``margin`` of that weight over the quorum; per consecutive chain pair of one epoch the rounds ``skipped``; per
        instance the ``blocks`` of the pool, the ``orphaned`` ones (off the chain and not above its tip: they can never commit), the
        ``pending`` ones (off the chain, above the tip) and the ``certified_off_chain`` ones (off the chain with a certificate).
        ``margin_hist[group, min(margin // bin_width, bins - 1)]`` bins the margins, ``votes_hist[group, v]`` counts the certificates
        with ``v`` votes (``num_nodes + 1`` columns), ``node_table[group, node]`` holds, in the order of ``VOTE_NODE_COLUMNS``, the
        blocks the node ``proposed``, the ``orphaned`` ones among them and the chain's certificates it ``voted`` in.  Instances with a
        fault are skipped.  The defaults are exact while the margins allow: width 1 and ``min(total - quorum + 1, 4096)`` bins.  Needs
        nothing of the run: no commit times, no round trace; serves every kind of batch."""
        if (bin_width is not None and int(bin_width) < 1) or (bins is not None and int(bins) < 1):
            raise ValueError("bin_width and bins must be at least 1")
        bin_width = 1 if bin_width is None else int(bin_width)
        if bins is None:
            total, quorum = self._voting_totals()
            bins = min(total - quorum + 1, 4096)
        bins = int(bins)
        groups, n = self._groups(), self._sim.num_nodes
        margin = np.zeros((groups, bins), dtype=np.uint64)
        votes = np.zeros((groups, n + 1), dtype=np.uint64)
        nodes = np.zeros((groups, n, len(_lib.VOTE_NODE_COLUMNS)), dtype=np.uint64)
        stats = np.zeros((groups, _lib.VOTE_STATS), dtype=np.uint64)
        check(_lib.lib().lbft_batch_vote_stats(self._sim._h, bin_width, bins, margin.ctypes.data, votes.ctypes.data, nodes.ctypes.data, stats.ctypes.data))
        return margin, votes, nodes, stats

    def _voting_totals(self):
        """(total, quorum) of the batch's voting rights: quorum = 2 * total // 3 + 1 (every epoch's rotation has the same total)."""
        cfg, n = self._sim._cfg, self._sim.num_nodes
        total = sum(int(cfg.voting_rights[k]) for k in range(n)) if cfg.voting_rights else n
        return total, 2 * total // 3 + 1

    def votes_by_param_set(self, quantiles=(0.5, 0.9, 0.99)):
        """Per group of ``vote_stats`` (default binning), in set order: the eight families of ``VOTE_FAMILIES`` = samples (``entries``,
        ``pairs`` or ``instances``), mean, min, max; ``margin["quantiles"]`` ({str(q): weight}, exact, the inverted-CDF rule of
        ``histogram_quantile``; ``None`` when the histogram clamps: more than 4 096 possible margins); ``votes_hist``, the certificates by
        number of votes; ``nodes`` = per node ``proposed``, ``orphaned``, ``voted`` and ``participation`` = voted / certificates;
        ``orphan_rate`` = orphaned / (blocks - pending), the share of the decided blocks that were proposed in vain;
        ``round_utilisation`` = pairs / (pairs + skipped rounds).  ``None`` where a denominator is 0."""
        total, quorum = self._voting_totals()
        exact = total - quorum + 1 <= 4096
        margin, votes, nodes, stats = self.vote_stats()
        keys = ("entries", "entries", "entries", "pairs", "instances", "instances", "instances", "instances")
        out = []
        for g in range(margin.shape[0]):
            row = {"set": g, **_families(stats[g], tuple(zip(_lib.VOTE_FAMILIES, keys)))}
            row["margin"]["quantiles"] = {str(q): histogram_quantile(margin[g], 1, q) for q in quantiles} if exact else None
            row["votes_hist"] = [int(v) for v in votes[g]]
            qcs = int(stats[g, 0])
            row["nodes"] = [{"proposed": int(p), "orphaned": int(o), "voted": int(v), "participation": int(v) / qcs if qcs else None}
                            for p, o, v in nodes[g]]
            blocks, orphaned, pending = (int(stats[g, 4 * f + 1]) for f in (4, 5, 6))
            row["orphan_rate"] = orphaned / (blocks - pending) if blocks - pending else None
            pairs, skipped = int(stats[g, 4 * 3]), int(stats[g, 4 * 3 + 1])
            row["round_utilisation"] = pairs / (pairs + skipped) if pairs + skipped else None
            out.append(row)
        return out

    def _epoch_binning(self, bin_width, bins):
        """(bin_width, bins) of ``epoch_stats``: by default the handover histogram covers [0, max_clock] in at most 4 096 bins, one pass
        through the kernel's LDS -- width ceil((max_clock + 1) / 4096) and as many bins as that width needs."""
        span = int(self._sim._max_clock) + 1
        if bin_width is None:
            bin_width = -(-span // (int(bins) if bins else 4096))
        if bins is None:
            bins = -(-span // int(bin_width))
        return int(bin_width), int(bins)

    def epoch_stats(self, bin_width=None, bins=None, epoch_bins=64):
        """Epoch statistics computed on the device (lbft_batch_epoch_stats), per group (the parameter sets of a ``with_param_sets`` batch,
        else one group): ``(handover_hist, epoch_table, stats)``.  An instance's chain is that of ``vote_stats``; a *segment* is a maximal
        run of chain entries of one epoch, the last one *open*, the others *complete*; a *boundary* is a chain pair of two epochs.
        ``stats[group]`` (40 uint64) holds ``(samples, sum, min, max)`` of the ten families of ``EPOCH_FAMILIES``: per instance its
        ``segments``; per node its ``node_epoch`` and how far that lies ``behind`` the instance's foremost node; per complete segment its
        ``length`` in entries, its ``duration`` (last proposal - first) and its ``last_round``; per segment its ``first_round``; per
        boundary the ``handover`` (the later entry's proposal - the earlier one's); per instance the ``stranded`` blocks (off the chain,
        in an epoch below the tip's) and the ``blocks`` of its pool.  ``handover_hist[group, min(handover // bin_width, bins - 1)]`` bins
        the handovers; ``epoch_table[group, min(epoch, epoch_bins - 1)]`` holds, in the order of ``EPOCH_COLUMNS``, the epoch's
        ``segments``, the ``complete`` ones, its chain ``entries``, the sums of its segments' ``duration`` and of the ``handover`` into
        it, its ``stranded`` blocks and its pool ``blocks``.  Instances with a fault are skipped.  By default the histogram covers
        [0, max_clock] in at most 4 096 bins.  Needs nothing of the run: no commit times, no round trace; serves every kind of batch."""
        if (bin_width is not None and int(bin_width) < 1) or (bins is not None and int(bins) < 1):
            raise ValueError("bin_width and bins must be at least 1")
        if not 1 <= int(epoch_bins) <= _lib.EPOCH_MAX_BINS:
            raise ValueError("epoch_bins: 1 to %d" % _lib.EPOCH_MAX_BINS)
        bin_width, bins = self._epoch_binning(bin_width, bins)
        groups, epoch_bins = self._groups(), int(epoch_bins)
        hist = np.zeros((groups, bins), dtype=np.uint64)
        table = np.zeros((groups, epoch_bins, len(_lib.EPOCH_COLUMNS)), dtype=np.uint64)
        stats = np.zeros((groups, _lib.EPOCH_STATS), dtype=np.uint64)
        check(_lib.lib().lbft_batch_epoch_stats(self._sim._h, bin_width, bins, epoch_bins, hist.ctypes.data, table.ctypes.data, stats.ctypes.data))
        return hist, table, stats

    def epochs_by_param_set(self, epoch_bins=64, quantiles=(0.5, 0.9, 0.99)):
        """Per group of ``epoch_stats`` (default binning), in set order: the ten families of ``EPOCH_FAMILIES`` = samples (``instances``,
        ``nodes``, ``segments`` or ``boundaries``), mean, min, max; ``handover["quantiles"]`` ({str(q): ticks}, exact, the inverted-CDF
        rule of ``histogram_quantile``; ``None`` when the default bins are wider than one tick); ``handover_cost`` = the mean handover
        minus the mean interval inside an epoch, sum(duration) / (sum(length) - segments) over the complete segments: what an epoch
        change adds to a block interval; ``stranded_per_epoch`` = stranded blocks / complete segments; ``behind_share`` = the share of the
        clean instances' nodes that ended in an epoch below their instance's foremost node's; ``per_epoch``: the epoch table's rows up
        to the last one that is not empty, each ``{"epoch", *EPOCH_COLUMNS}`` (the row ``epoch_bins - 1`` also holds every epoch above
        it).  ``None`` where a denominator is 0."""
        width, _ = self._epoch_binning(None, None)
        hist, table, stats = self.epoch_stats(epoch_bins=epoch_bins)
        names = _lib.EPOCH_FAMILIES
        keys = ("instances", "nodes", "nodes", "segments", "segments", "segments", "segments", "boundaries", "instances", "instances")
        set_of = getattr(self._sim, "set_of_instance", None) if self._sim.param_sets is not None else None
        node_epochs, clean = self.epochs.astype(np.int64), self.faults == 0
        behind = node_epochs.max(axis=1, keepdims=True) - node_epochs > 0
        out = []
        for g in range(hist.shape[0]):
            row = {"set": g, **_families(stats[g], tuple(zip(names, keys)))}
            row["handover"]["quantiles"] = {str(q): histogram_quantile(hist[g], 1, q) for q in quantiles} if width == 1 else None
            total = lambda name, word: int(stats[g, 4 * names.index(name) + word])
            complete, inner = total("length", 0), total("length", 1) - total("length", 0)
            row["handover_cost"] = row["handover"]["mean"] - total("duration", 1) / inner if complete and inner else None
            row["stranded_per_epoch"] = total("stranded", 1) / complete if complete else None
            members = clean if set_of is None else clean & (set_of == g)
            row["behind_share"] = float(behind[members].mean()) if members.any() else None
            used = np.flatnonzero(table[g].any(axis=1))
            row["per_epoch"] = [{"epoch": x, **{c: int(v) for c, v in zip(_lib.EPOCH_COLUMNS, table[g, x])}}
                                for x in range(int(used[-1]) + 1 if len(used) else 0)]
            out.append(row)
        return out

    def by_param_set(self):
        """Per parameter set of a ``BatchSimulator.with_param_sets`` batch, in set order: the number of instances, of faulted instances,
        and mean / min / max over its instances of the commits and of the active round (each instance's minimum over its nodes)."""
        set_of = getattr(self._sim, "set_of_instance", None)
        if set_of is None:
            raise ValueError("by_param_set needs a batch created with BatchSimulator.with_param_sets")
        commits = self.commit_counts.min(axis=1)
        rounds = self.active_rounds.min(axis=1)
        faulted = self.faults != 0
        out = []
        for k in range(len(self._sim.param_sets)):
            sel = set_of == k
            row = {"set": k, "instances": int(sel.sum()), "faulted": int(faulted[sel].sum())}
            for name, v in (("commits", commits[sel]), ("rounds", rounds[sel])):
                row[name] = ({"mean": float(v.mean()), "min": int(v.min()), "max": int(v.max())} if len(v) else
                             {"mean": None, "min": None, "max": None})
            out.append(row)
        return out

    def commit_times(self, cap_per_node=None):
        """[instance, node, k] int64, aligned with ``committed_histories``: the simulator clock (a GlobalTime) of the event during which the
        node committed its k-th entry, -1 where nothing was recorded (past the commit count, or lost to a log overflow).  Needs a batch
        created with ``commit_times=True``.  ``cap_per_node=None``: the width ``committed_histories()`` gives (the largest commit count, at
        least 1); an explicit 0 gives an empty last axis."""
        if cap_per_node is None:
            cap_per_node = max(int(self.commit_counts.max()) if self._sim.num_instances else 0, 1)
        cap_per_node = int(cap_per_node)
        if cap_per_node < 0:
            raise ValueError("cap_per_node must be at least 0")
        out = np.full((self._sim.num_instances, self._sim.num_nodes, cap_per_node), -1, dtype=np.int64)
        check(_lib.lib().lbft_batch_commit_times(self._sim._h, out.ctypes.data, cap_per_node))
        return out

    def latency_histogram(self, bin_width=None, bins=None):
        """Commit-latency histogram computed on the device, per group (the parameter sets of a ``with_param_sets`` batch, else one group):
        ``(hist, stats)``, ``hist[group, min(latency // bin_width, bins - 1)]`` (uint64; the last bin also counts everything above it) and
        ``stats[group] = (samples, sum, min, max)`` (uint64).  One sample per (instance, node, committed entry) of the instances without a
        fault; latency = commit time - (startup_times[proposer] + time).  The defaults are exact: width 1 and max_clock + 1 bins while
        that is at most 65 536 bins, above that the smallest width that fits."""
        bin_width, bins = self._binning(bin_width, bins)
        groups = self._groups()
        hist = np.zeros((groups, bins), dtype=np.uint64)
        stats = np.zeros((groups, 4), dtype=np.uint64)
        check(_lib.lib().lbft_batch_commit_latency_histogram(self._sim._h, bin_width, bins, hist.ctypes.data, stats.ctypes.data))
        return hist, stats

    def latency_by_param_set(self, quantiles=(0.5, 0.9, 0.99)):
        """Per group of ``latency_histogram`` (parameter set, or the one group of a plain batch), in set order: ``samples``, ``mean``,
        ``min``, ``max`` and ``quantiles`` ({str(q): latency}), from the device histogram with its default (exact) binning.  Quantiles use
        the inverted-CDF rule -- the smallest L with count(<= L) >= ceil(q * samples), numpy's ``method="inverted_cdf"`` -- and are exact
        with bins of width 1; ``None`` without samples."""
        width, _ = self._binning(None, None)
        hist, stats = self.latency_histogram()
        out = []
        for g in range(hist.shape[0]):
            row = {"set": g, **_families(stats[g], (("latency", "samples"),))["latency"]}
            row["quantiles"] = {str(q): histogram_quantile(hist[g], width, q) for q in quantiles}
            out.append(row)
        return out

    def _binning(self, bin_width, bins):
        """(bin_width, bins) with ``latency_histogram``'s defaults: width 1 and max_clock + 1 bins while that is at most 65 536 bins,
        above that the smallest width that fits.  ValueError below 1, before any library call."""
        if (bin_width is not None and int(bin_width) < 1) or (bins is not None and int(bins) < 1):
            raise ValueError("bin_width and bins must be at least 1")
        span = int(self._sim._max_clock) + 1
        if bin_width is None:
            bin_width = -(-span // int(bins)) if bins else max(1, -(-span // (1 << 16)))
        if bins is None:
            bins = -(-span // int(bin_width))
        return int(bin_width), int(bins)

    def _groups(self):
        return len(self._sim.param_sets) if self._sim.param_sets is not None else 1

    def _since(self, since):
        """``since`` of ``stall_histogram`` as one int64 per group (None: every group from clock 0)."""
        groups, max_clock = self._groups(), int(self._sim._max_clock)
        if since is None:
            return None
        if isinstance(since, str):
            if since != "partition_end":
                raise ValueError("since: None, an int, one int per group or 'partition_end'")
            sets = self._sim.param_sets
            parts = [ps.partition for ps in sets] if sets is not None else [getattr(self._sim, "partition", None)]
            return np.array([0 if p is None or p[0] == 0 else min(max(int(p[2]), 0), max_clock) for p in parts], dtype=np.int64)
        if np.ndim(since) == 0:
            since = [since] * groups
        if len(since) != groups:
            raise ValueError("since needs one entry per group (%d)" % groups)
        out = np.array([int(v) for v in since], dtype=np.int64).reshape(groups)
        if ((out < 0) | (out > max_clock)).any():
            raise ValueError("since must lie in [0, max_clock]")
        return out

    def commit_series(self, bin_width=None, bins=None):
        """Commits over time, computed on the device from the recorded commit times: ``[groups, bins]`` uint64,
        ``series[group, min(commit time // bin_width, bins - 1)]`` counts every committed entry of every node of the group's instances
        without a fault (a row sums to ``latency_histogram``'s sample count).  Groups and default binning as ``latency_histogram``."""
        bin_width, bins = self._binning(bin_width, bins)
        series = np.zeros((self._groups(), bins), dtype=np.uint64)
        check(_lib.lib().lbft_batch_commit_series(self._sim._h, bin_width, bins, series.ctypes.data))
        return series

    def stall_histogram(self, since=None, bin_width=None, bins=None):
        """Commit-free intervals, computed on the device: ``(hist, stats)``.  A node's commit instants are its distinct commit times; they
        cut [0, max_clock] into intervals.  ``hist[group, min(gap // bin_width, bins - 1)]`` counts the gaps between consecutive instants
        of a node; ``stats[group]`` (16 uint64) holds ``(samples, sum, min, max)`` of four families: the gaps, ``first`` (per node, from
        ``since`` to its first instant at or after it, if any), ``tail`` (per node, max_clock - its last instant; max_clock without
        commits) and ``longest`` (per node, its longest interval, the leading one and the tail included).  ``since``: None (0), one
        int, one per group, or ``"partition_end"`` -- each set's (or the batch's) partition end clipped to [0, max_clock], 0 without a
        partition: ``first`` is then the recovery time.  Instances with a fault are skipped; binning as ``latency_histogram``."""
        bin_width, bins = self._binning(bin_width, bins)
        since = self._since(since)
        groups = self._groups()
        hist = np.zeros((groups, bins), dtype=np.uint64)
        stats = np.zeros((groups, _lib.STALL_STATS), dtype=np.uint64)
        check(_lib.lib().lbft_batch_commit_stalls(self._sim._h, None if since is None else since.ctypes.data, bin_width, bins,
                                                  hist.ctypes.data, stats.ctypes.data))
        return hist, stats

    def stalls_by_param_set(self, since=None, quantiles=(0.5, 0.9, 0.99)):
        """Per group of ``stall_histogram`` (default, exact binning), in set order: ``since``, ``gaps`` = samples, mean, min, max and
        ``quantiles`` ({str(q): gap}, the inverted-CDF rule of ``histogram_quantile``), and ``first`` / ``tail`` / ``longest`` = nodes,
        mean, min, max.  ``None`` where there are no samples."""
        width, _ = self._binning(None, None)
        since = self._since(since)
        hist, stats = self.stall_histogram(since)
        out = []
        for g in range(hist.shape[0]):
            row = {"set": g, "since": int(since[g]) if since is not None else 0,
                   **_families(stats[g], (("gaps", "samples"), ("first", "nodes"), ("tail", "nodes"), ("longest", "nodes")))}
            row["gaps"]["quantiles"] = {str(q): histogram_quantile(hist[g], width, q) for q in quantiles}
            out.append(row)
        return out

    def finality_histogram(self, bin_width=None, bins=None):
        """Commit finality computed on the device (lbft_batch_commit_finality), per group: ``(finality_hist, spread_hist, first_committer,
        stats)``.  For every entry of an instance's chain (the log of its reference node, as ``chain_stats``) the commit times of all
        its nodes give the time at which the ``first`` node had committed it, at which nodes holding ``valid`` (total - quorum + 1) and
        ``quorum`` voting rights had, and at which ``all`` had (only where every node committed it); the rights of an entry are those
        of its epoch (``rights_rotation``).  ``finality_hist[group, min(v // bin_width, bins - 1)]`` counts the quorum finality
        (quorum time - the entry's proposal time ``startup_times[proposer] + time``), ``spread_hist`` the spread (all - first);
        ``first_committer[group, j]`` the entries node ``j`` committed first (the lowest-numbered of a tie); ``stats[group]`` (24
        uint64) holds ``(samples, sum, min, max)`` of six families: ``first``, ``valid``, ``quorum``, ``all`` (each after the proposal
        time), ``spread`` and ``open`` (per instance, the entries at the chain's tip that no quorum had committed when the run ended).
        Instances with a fault are skipped.  Needs a batch created with ``commit_times=True``.  Groups and default binning as
        ``latency_histogram``."""
        bin_width, bins = self._binning(bin_width, bins)
        groups = self._groups()
        fin = np.zeros((groups, bins), dtype=np.uint64)
        spread = np.zeros((groups, bins), dtype=np.uint64)
        first = np.zeros((groups, self._sim.num_nodes), dtype=np.uint64)
        stats = np.zeros((groups, _lib.FINALITY_STATS), dtype=np.uint64)
        check(_lib.lib().lbft_batch_commit_finality(self._sim._h, bin_width, bins, fin.ctypes.data, spread.ctypes.data, first.ctypes.data,
                                                    stats.ctypes.data))
        return fin, spread, first, stats

    def finality_by_param_set(self, quantiles=(0.5, 0.9, 0.99)):
        """Per group of ``finality_histogram`` (default, exact binning), in set order: ``first``, ``valid``, ``quorum``, ``all`` and
        ``spread`` = samples, mean, min, max; ``quorum`` and ``spread`` also ``quantiles`` ({str(q): ticks}, the inverted-CDF rule of
        ``histogram_quantile``); ``open`` = instances, mean, min, max; ``first_committer``, the entries per node that committed them
        first, and ``first_share``, their fractions (``None`` without entries).  ``None`` where there are no samples."""
        width, _ = self._binning(None, None)
        fin, spread, first, stats = self.finality_histogram()
        out = []
        for g in range(fin.shape[0]):
            row = {"set": g, **_families(stats[g], (("first", "samples"), ("valid", "samples"), ("quorum", "samples"), ("all", "samples"),
                                                    ("spread", "samples"), ("open", "instances")))}
            row["quorum"]["quantiles"] = {str(q): histogram_quantile(fin[g], width, q) for q in quantiles}
            row["spread"]["quantiles"] = {str(q): histogram_quantile(spread[g], width, q) for q in quantiles}
            counts = [int(v) for v in first[g]]
            entries = sum(counts)
            row["first_committer"] = counts
            row["first_share"] = [c / entries for c in counts] if entries else None
            out.append(row)
        return out

    def instance_stats(self, since=None):
        """Per-instance statistics computed on the device (lbft_batch_instance_stats): ``[instances, 11, 4]`` uint64,
        ``(samples, sum, min, max)`` of the families ``_lib.INSTANCE_FAMILIES`` restricted to one instance -- what ``latency_histogram``
        (family 0), ``stall_histogram`` (families 1 to 4: gaps, first, tail, longest) and ``finality_histogram`` (families 5 to 10:
        first, valid, quorum, all, spread, open) would report if the instance were a group of its own; min = max = 0 without samples.
        ``since`` as ``stall_histogram``'s, applied to every instance of the group.  The row of an instance with a fault is all zero.
        Needs a batch created with ``commit_times=True``."""
        since = self._since(since)
        rows = np.zeros((self._sim.num_instances, len(_lib.INSTANCE_FAMILIES), 4), dtype=np.uint64)
        check(_lib.lib().lbft_batch_instance_stats(self._sim._h, None if since is None else since.ctypes.data, rows.ctypes.data))
        return rows

    def seed_spread(self, since=None):
        """The spread of the per-instance values across the seeds of a group, in set order: one dict per group (parameter set, or the
        one group of a plain batch) with ``set``, ``instances``, ``faulted`` and, per metric, ``{instances, mean, std, stderr, min, max,
        min_seed, max_seed}`` over the group's instances without a fault that have a value.  ``std`` is numpy's ``ddof=1`` and
        ``stderr = std / sqrt(instances)`` -- the error bar of ``mean`` (samples inside one instance are correlated: it cannot come from
        a pooled sample count); both ``None`` below two instances, everything ``None`` without any.  ``min_seed`` / ``max_seed`` are
        ``sim.seeds[i]`` of the lowest-numbered instance attaining the extreme: the seed to replay in ``Simulator.new``.  With
        ``S = instance_stats(since)`` in float64, per instance i:
          commits               commit_counts[i].min()
          latency_mean          S[i, 0, 1] / S[i, 0, 0]   (a value where S[i, 0, 0] > 0, as for every quotient and extreme below)
          latency_max           S[i, 0, 3]
          longest_stall         S[i, 4, 3]
          recovery              S[i, 2, 3]                (the slowest node's first commit at or after ``since``)
          finality_quorum_mean  S[i, 7, 1] / S[i, 7, 0]
          finality_quorum_max   S[i, 7, 3]
          spread_max            S[i, 9, 3]
          open                  S[i, 10, 1]"""
        S = self.instance_stats(since).astype(np.float64)
        m = self._sim.num_instances
        seeds = np.asarray(self._sim.seeds)
        faulted = np.asarray(self.faults) != 0
        set_of = np.asarray(self._sim.set_of_instance) if self._sim.param_sets is not None else np.zeros(m, dtype=np.int64)

        def quotient(f):
            have = S[:, f, 0] > 0
            return np.divide(S[:, f, 1], S[:, f, 0], out=np.zeros(m), where=have), have

        def extreme(f):
            return S[:, f, 3], S[:, f, 0] > 0
        metrics = (("commits", (np.asarray(self.commit_counts).min(axis=1).astype(np.float64), np.ones(m, dtype=bool))),
                   ("latency_mean", quotient(0)), ("latency_max", extreme(0)), ("longest_stall", extreme(4)), ("recovery", extreme(2)),
                   ("finality_quorum_mean", quotient(7)), ("finality_quorum_max", extreme(7)), ("spread_max", extreme(9)),
                   ("open", (S[:, 10, 1], S[:, 10, 0] > 0)))
        out = []
        for g in range(self._groups()):
            in_group = set_of == g
            row = {"set": g, "instances": int(in_group.sum()), "faulted": int((in_group & faulted).sum())}
            for name, (value, have) in metrics:
                idx = np.nonzero(in_group & ~faulted & have)[0]
                v = value[idx]
                k = len(v)
                std = float(v.std(ddof=1)) if k >= 2 else None
                row[name] = {"instances": k, "mean": float(v.mean()) if k else None, "std": std,
                             "stderr": std / float(np.sqrt(k)) if k >= 2 else None,
                             "min": float(v.min()) if k else None, "max": float(v.max()) if k else None,
                             "min_seed": int(seeds[idx[np.argmin(v)]]) if k else None, "max_seed": int(seeds[idx[np.argmax(v)]]) if k else None}
            out.append(row)
        return out

    def _phase_edges(self, edges):
        """``edges`` of ``phase_histogram`` as int64 ``[groups, phases - 1]``; ValueError before any library call."""
        groups, top = self._groups(), int(self._sim._max_clock) + 1
        if isinstance(edges, str):
            if edges != "partition":
                raise ValueError("edges: a sequence of ints, one sequence per group or 'partition'")
            sets = self._sim.param_sets
            parts = [ps.partition for ps in sets] if sets is not None else [getattr(self._sim, "partition", None)]
            rows = [[top, top] if p is None or p[0] == 0 else [min(max(int(p[1]), 0), top), min(max(int(p[1]), int(p[2]), 0), top)] for p in parts]
        else:
            rows = list(edges)
            if all(np.ndim(r) == 0 for r in rows):  # (also []: one phase)
                rows = [rows] * groups
            elif not all(np.ndim(r) == 1 for r in rows):
                raise ValueError("edges: a sequence of ints or one sequence of ints per group")
            elif len(rows) != groups:
                raise ValueError("edges needs one sequence per group (%d)" % groups)
            rows = [[int(v) for v in r] for r in rows]
        if len({len(r) for r in rows}) != 1:
            raise ValueError("every group needs the same number of edges")
        if len(rows[0]) > _lib.MAX_PHASES - 1:
            raise ValueError("at most %d edges (%d phases)" % (_lib.MAX_PHASES - 1, _lib.MAX_PHASES))
        out = np.array(rows, dtype=np.int64).reshape(groups, len(rows[0]))
        if ((out < 0) | (out > top)).any() or (np.diff(out, axis=1) < 0).any():
            raise ValueError("edges must lie in [0, max_clock + 1] and must not decrease")
        return out

    def phase_histogram(self, edges, bin_width=None, bins=None):
        """Commit latency and finality per proposal-time window, computed on the device (lbft_batch_commit_phases): ``(latency_hist,
        finality_hist, stats)`` with ``latency_hist[group, phase, min(v // bin_width, bins - 1)]``, ``finality_hist`` the same for the
        quorum finality, and ``stats[group, phase, family] = (samples, sum, min, max)`` of the families ``_lib.PHASE_FAMILIES``: the
        latency sample of ``latency_histogram`` and ``first``, ``valid``, ``quorum``, ``all``, ``spread`` of ``finality_histogram``
        (uint64; min = max = 0 without samples).  A group's edges ``e_0 <= e_1 <= ...`` in ``[0, max_clock + 1]`` cut the clock into
        phases, phase ``p`` covering ``[e_{p-1}, e_p)``; an entry belongs to the phase of its proposal time ``startup_times[proposer] +
        time`` however late it commits.  ``edges``: a sequence of ints (the same for every group; ``[]``: one phase), one sequence
        per group, or ``"partition"`` -- ``[start, end]`` of each set's (or the batch's) partition, and ``[max_clock + 1, max_clock +
        1]`` without one, so that everything is "before".  ``edges=[warm, max_clock - cool]`` sets a warm-up and a cool-down apart:
        phase 1 is the steady state.  With one phase the arrays are ``latency_histogram``'s and ``finality_histogram``'s; the phases
        of a group add up to them.  ``open`` and the first committers are not split.  Instances with a fault are skipped.  Needs a
        batch created with ``commit_times=True``.  Groups and default binning as ``latency_histogram``."""
        bin_width, bins = self._binning(bin_width, bins)
        edges = self._phase_edges(edges)
        groups, phases = edges.shape[0], edges.shape[1] + 1
        lat = np.zeros((groups, phases, bins), dtype=np.uint64)
        fin = np.zeros((groups, phases, bins), dtype=np.uint64)
        stats = np.zeros((groups, phases, len(_lib.PHASE_FAMILIES), 4), dtype=np.uint64)
        check(_lib.lib().lbft_batch_commit_phases(self._sim._h, edges.ctypes.data if phases > 1 else None, phases, bin_width, bins, lat.ctypes.data,
                                                  fin.ctypes.data, stats.ctypes.data))
        return lat, fin, stats

    def phases_by_param_set(self, edges, quantiles=(0.5, 0.9, 0.99)):
        """Per group of ``phase_histogram`` (default, exact binning), in set order: ``set`` and ``phases``, a list with one dict per
        phase: ``from`` and ``to`` (the phase covers ``[from, to)``; the first starts at 0, the last ends at ``max_clock + 1``), the six
        families ``latency``, ``first``, ``valid``, ``quorum``, ``all``, ``spread`` = samples, mean, min, max, and ``quantiles``
        ({str(q): ticks}, the inverted-CDF rule of ``histogram_quantile``) for ``latency`` and ``quorum``.  ``None`` where there are no
        samples."""
        width, _ = self._binning(None, None)
        bounds = self._phase_edges(edges)
        lat, fin, stats = self.phase_histogram(bounds)
        top = int(self._sim._max_clock) + 1
        out = []
        for g in range(lat.shape[0]):
            rows = []
            for p in range(lat.shape[1]):
                row = {"from": int(bounds[g, p - 1]) if p else 0, "to": int(bounds[g, p]) if p < bounds.shape[1] else top,
                       **_families(stats[g, p].reshape(-1), tuple((name, "samples") for name in _lib.PHASE_FAMILIES))}
                row["latency"]["quantiles"] = {str(q): histogram_quantile(lat[g, p], width, q) for q in quantiles}
                row["quorum"]["quantiles"] = {str(q): histogram_quantile(fin[g, p], width, q) for q in quantiles}
                rows.append(row)
            out.append({"set": g, "phases": rows})
        return out

    def contexts(self, instance=0):
        """The ``Vec<&Context>`` that ``Simulator::loop_until`` returns, for one instance."""
        return [SimulatedContextView(self, instance, n) for n in range(self._sim.num_nodes)]


class SimulatedContextView:
    """Read-only view with the accessors the reference's callers use (main.rs:47-53,
    tests/simulated_run.rs:45-94)."""

    def __init__(self, result, instance, node):
        self._r, self._i, self._n = result, instance, node

    def committed_history(self):
        h = self._r.committed_history(self._i, self._n)
        return [(Command(int(e["proposer"]), int(e["index"])), int(e["time"])) for e in h]

    def last_committed_state(self):
        out = C.c_uint64()
        check(_lib.lib().lbft_batch_last_committed_state(self._r._sim._h, self._i, self._n, C.byref(out)))
        return State(int(out.value))


class BatchSimulator:
    """Many independent ``Simulator``s (bft-lib/src/simulator.rs:26-33) advanced in lockstep on one GPU."""

    def __init__(self, rng_seeds, num_nodes, network_delay, node_config=None, commands_per_epoch=30000,
                 voting_rights=None, device=0, queue_capacity=0, snapshot_capacity=0, block_capacity=0,
                 log_capacity=0, max_steps_per_launch=0, lanes_per_wavefront=0, lds_queue_slots=-1, equivocate_every=0, drop_per_million=0, partition=None,
                 calendar_queue=True, quirks=0, rights_rotation=0, keep_retired_stores=False, commit_times=False, _param_sets=None,
                 _set_of_instance=None):
        seeds = np.ascontiguousarray(rng_seeds, dtype=np.uint64)
        self.seeds = seeds
        self.num_instances = int(seeds.shape[0])
        self.num_nodes = int(num_nodes)
        self.device = int(device)
        self._cfg = make_config(num_nodes, network_delay, node_config or NodeConfig(), commands_per_epoch, voting_rights,
                                queue_capacity, snapshot_capacity, block_capacity, log_capacity, equivocate_every, drop_per_million, partition, quirks,
                                rights_rotation)
        self._h = C.c_void_p()
        self.param_sets = None
        self.partition = None if partition is None else tuple(int(v) for v in partition)
        self._max_clock = 0
        if _param_sets is None:
            check(_lib.lib().lbft_batch_create(C.byref(self._cfg), seeds.ctypes.data, self.num_instances, self.device,
                                               C.byref(self._h)))
        else:
            self.param_sets = list(_param_sets)
            self.set_of_instance = np.ascontiguousarray(_set_of_instance, dtype=np.uint32)
            if self.set_of_instance.shape != seeds.shape:
                raise ValueError("set_of_instance needs one entry per seed")
            structs = (_lib.LbftParamSet * max(len(self.param_sets), 1))(*[ps.to_struct() for ps in self.param_sets])
            check(_lib.lib().lbft_batch_create_param_sets(C.byref(self._cfg), structs, len(self.param_sets), self.set_of_instance.ctypes.data,
                                                          seeds.ctypes.data, self.num_instances, self.device, C.byref(self._h)))
        if max_steps_per_launch:
            check(_lib.lib().lbft_batch_set_max_steps(self._h, max_steps_per_launch))
        if lanes_per_wavefront:
            check(_lib.lib().lbft_batch_set_lanes_per_wavefront(self._h, lanes_per_wavefront))
        if not calendar_queue:
            check(_lib.lib().lbft_batch_set_calendar_queue(self._h, 0))
        if lds_queue_slots != -1:
            check(_lib.lib().lbft_batch_set_lds_queue_slots(self._h, lds_queue_slots))
        if keep_retired_stores:  # past_record_stores (node.rs:43) in full: save_node then also serves nodes that have changed epoch
            check(_lib.lib().lbft_batch_keep_retired_stores(self._h, 1))
        if commit_times:  # the commit-time twin kernels (lbft_batch_record_commit_times): BatchResult.commit_times, latency_histogram
            check(_lib.lib().lbft_batch_record_commit_times(self._h, 1))

    @classmethod
    def new(cls, rng_seeds, num_nodes, network_delay, node_config=None, **kw):
        return cls(rng_seeds, num_nodes, network_delay, node_config, **kw)

    @classmethod
    def with_param_sets(cls, rng_seeds, num_nodes, param_sets, set_of_instance, **kw):
        """One batch over a grid of parameter sets (lbft_batch_create_param_sets): instance i runs ``param_sets[set_of_instance[i]]``
        (a ``ParamSet``) with seed ``rng_seeds[i]`` and gives what a plain batch of that set and seed gives.  ``kw`` as for ``new`` except
        the per-set ones (network_delay, node_config, drop_per_million, partition); the sets share one delay model.  At most 256 sets
        and 32 nodes; the node-level interface is not available on such a batch."""
        param_sets = list(param_sets)
        for k in ("network_delay", "node_config", "drop_per_million", "partition"):
            if k in kw:
                raise TypeError("%s is set per parameter set (ParamSet), not per batch" % k)
        if not param_sets:
            raise ValueError("at least one parameter set")
        models = {ps.network_delay.model for ps in param_sets}
        if len(models) != 1:
            raise ValueError("the parameter sets of one batch share one delay model")
        first = param_sets[0]
        return cls(rng_seeds, num_nodes, first.network_delay, first.node_config, _param_sets=param_sets, _set_of_instance=set_of_instance, **kw)

    def loop_until(self, max_clock, csv_path=None, allow_faults=False, round_trace=None):
        """Simulator::loop_until for every instance, ``0 <= max_clock <= 2**31 - 3`` (LBFT_MAX_CLOCK; LbftError -1 outside).  ``csv_path`` is the reference's ``Option<String>`` data-files
        directory (bft-lib/src/simulator.rs:380-381, data_writer.rs): when given, the round-switch trace is recorded on
        the device and ``round_switches.txt`` / ``number_of_messages.txt`` of instance 0 are written there in the
        reference's CSV format.  ``round_trace=N`` only records (N rounds per node) for ``BatchResult.round_switches``."""
        # The trace rows are allocated for EVERY instance of the batch (num_nodes x round_trace words each).  Left to this method, the
        # capacity starts from a realistic bound -- a round of >= 3 nodes takes two network hops, max_clock / 5 rounds is generous for
        # delays of mean >= 5 -- and only a run that overflows it (F_TRACE_OVERFLOW: tiny networks, near-zero delays) is repeated with
        # the worst case, one round per time unit (at most 65 536 rounds: longer horizons need an explicit round_trace).
        auto = csv_path is not None and round_trace is None
        worst = min(int(max_clock) + 64, 1 << 16)
        if auto:
            round_trace = min(int(max_clock) // 5 + 64, worst)
        if round_trace:
            check(_lib.lib().lbft_batch_enable_round_trace(self._h, int(round_trace)))
        self._mutated()
        self._max_clock = int(max_clock)
        rc = check(_lib.lib().lbft_batch_run_until(self._h, int(max_clock)), allow_fault=allow_faults or auto)
        if auto and rc == _lib.LBFT_ERR_FAULT:
            if round_trace < worst and (BatchResult(self).faults & _lib.LBFT_FAULT_TRACE_OVERFLOW).any():
                import warnings
                warnings.warn("loop_until(csv_path=...): a node passed the automatic round-trace capacity (%d rounds); the whole batch is run "
                              "AGAIN with the worst case (%d rounds per node = %d trace words per instance, every instance of the batch). "
                              "Pass round_trace=N to choose the capacity yourself." % (round_trace, worst, self.num_nodes * (worst + 1)))
                self.reset()
                check(_lib.lib().lbft_batch_enable_round_trace(self._h, worst))
                rc = check(_lib.lib().lbft_batch_run_until(self._h, int(max_clock)), allow_fault=True)
            if rc == _lib.LBFT_ERR_FAULT and not allow_faults:
                # (the text comes from the instances' fault words, not from lbft_last_error: that may be another call's)
                f = BatchResult(self).faults
                bits = int(np.bitwise_or.reduce(f)) if len(f) else 0
                names = [n for b, n in sorted(_lib.FAULT_NAMES.items()) if bits & b] or ["fault bits 0x%x" % bits]
                raise LbftError(rc, "%d instance(s) faulted: %s" % (int((f != 0).sum()), ", ".join(names)))
        res = BatchResult(self)
        if csv_path is not None:
            write_data_files(csv_path, *res.round_switches(0), self.num_nodes)
        return res

    def run_steps(self, max_clock, steps, allow_faults=False):
        """At most ``steps`` events per instance (first call = Simulator::new).  Returns (unfinished instances, BatchResult
        or None); the result is available once nothing is left to process."""
        left = C.c_uint64()
        self._mutated()
        self._max_clock = int(max_clock)
        check(_lib.lib().lbft_batch_run_steps(self._h, int(max_clock), int(steps), C.byref(left)), allow_fault=allow_faults)
        return int(left.value), (BatchResult(self) if left.value == 0 else None)

    def save_checkpoint(self, path):
        """Whole-batch checkpoint (the reference's save_node, node.rs:233-238, at batch granularity)."""
        nbytes = _lib.lib().lbft_batch_checkpoint_bytes(self._h)
        buf = np.zeros(nbytes, dtype=np.uint8)
        check(_lib.lib().lbft_batch_checkpoint_save(self._h, buf.ctypes.data, nbytes))
        buf.tofile(path)
        return nbytes

    def load_checkpoint(self, path):
        """load_node (node.rs:211-231) at batch granularity: into a batch created with the same configuration."""
        buf = np.fromfile(path, dtype=np.uint8)
        self._mutated()
        check(_lib.lib().lbft_batch_checkpoint_load(self._h, buf.ctypes.data, buf.size))

    def manual(self, max_clock=1000):
        """Node-level mode: initial node states only (NodeState::make_initial_state), no event loop.  Returns
        ``nodes[instance][author]`` -> NodeHandle."""
        self._mutated()
        check(_lib.lib().lbft_batch_manual_begin(self._h, int(max_clock)))
        return [[NodeHandle(self, i, n) for n in range(self.num_nodes)] for i in range(self.num_instances)]

    def node_calls(self, calls):
        """Many trait calls in ONE launch (lbft_node_calls): `calls` = iterable of (op, instance, node, peer, handle, node_time) with op
        one of _lib.CALL_*; every call on another instance.  Returns a list of dicts (actions / handle / should_sync per call)."""
        calls = list(calls)
        arr = (_lib.LbftNodeCall * len(calls))()
        for k, (op, inst, node, peer, handle, t) in enumerate(calls):
            arr[k] = _lib.LbftNodeCall(int(op), int(inst), int(node), int(peer), int(handle), 0, int(t))
        res = (_lib.LbftNodeResult * len(calls))()
        self._mutated()
        check(_lib.lib().lbft_node_calls(self._h, arr, len(calls), res))
        return [{"actions": r.actions.as_dict(), "handle": int(r.handle), "should_sync": bool(r.should_sync), "status": int(r.status)} for r in res]

    def release_notification(self, instance, notification):
        check(_lib.lib().lbft_node_release_notification(self._h, int(instance), notification[1]))

    def manual_finalize(self):
        """Makes commit counts / histories / States of a node-level session readable (BatchResult)."""
        self._mutated()
        check(_lib.lib().lbft_batch_manual_finalize(self._h), allow_fault=True)
        return BatchResult(self)

    def save_node(self, instance, node):
        ln = C.c_size_t()
        check(_lib.lib().lbft_batch_save_node(self._h, int(instance), int(node), None, 0, C.byref(ln)))
        buf = np.zeros(ln.value, dtype=np.uint8)
        check(_lib.lib().lbft_batch_save_node(self._h, int(instance), int(node), buf.ctypes.data, ln.value, C.byref(ln)))
        return buf.tobytes()

    def load_node(self, instance, node, image, node_time):
        """ConsensusNode::load_node (node.rs:211-231): the bincode NodeState ``image`` (bytes) into the device-resident node; raises
        LbftError (LBFT_ERR_STATE) for "saved state from the future" (``node_time`` before the image's own times), LBFT_ERR_UNSUPPORTED
        for an image naming records this instance's block pool does not hold.  The node is untouched when it raises."""
        buf = np.frombuffer(bytes(image), dtype=np.uint8)
        check(_lib.lib().lbft_batch_load_node(self._h, int(instance), int(node), buf.ctypes.data, len(buf), int(node_time)))
        self._mutated()

    def _mutated(self):
        """Every call that changes device state -- a run, a reset, a checkpoint / node load, a node-level call -- invalidates what BatchResult
        objects of this simulator read back before (they re-read on their next access; round-5 advisor: only load_node used to do this)."""
        self._state_generation = getattr(self, "_state_generation", 0) + 1

    def reset(self):
        self._mutated()
        check(_lib.lib().lbft_batch_reset(self._h))

    def stream_handle(self):
        return _lib.lib().lbft_batch_stream(self._h)

    def last_run_ms(self):
        a, b = C.c_float(), C.c_float()
        check(_lib.lib().lbft_batch_last_run_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def phase_cycles(self):
        """Diagnostic builds only (LBFT_PHASE_TIMERS): shader cycles per phase of the event loop."""
        out = np.zeros(32, dtype=np.uint64)
        check(_lib.lib().lbft_batch_phase_cycles(self._h, out.ctypes.data))
        return out

    def layout(self):
        """Struct sizes behind the roofline arithmetic (see include/lbft.h lbft_batch_layout)."""
        out = np.zeros(8, dtype=np.uint32)
        check(_lib.lib().lbft_batch_layout(self._h, out.ctypes.data))
        keys = ("node_bytes", "event_bytes", "snapshot_bytes", "block_bytes", "instance_bytes", "lds_queue_slots",
                "lanes_per_wavefront", "kernel_class")
        return dict(zip(keys, (int(v) for v in out)))

    def device_bytes(self):
        return int(_lib.lib().lbft_batch_device_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().lbft_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NodeHandle:
    """One node of one instance behind the reference's trait surface (bft-lib/src/interfaces.rs): ``ConsensusNode::
    update_node`` and ``DataSyncNode::{create_notification, handle_notification}``, each executed on the GPU by
    ``lbft_node_*``.  Obtained from ``BatchSimulator.manual(...)``; the caller owns time and message delivery (the role
    of ``Simulator::loop_until`` or of bft-driver's ``CoreDriver``).  The clocks of ``update_node`` and ``handle_response`` lie in
    ``[0, 2**31 - 3]`` (LBFT_MAX_CLOCK), also past the session's ``max_clock``: the device keeps clocks as 32 bits; outside that
    range the call raises LbftError -1 and leaves the node untouched."""

    def __init__(self, sim, instance, node):
        self._sim, self.instance, self.author = sim, int(instance), int(node)

    def update_node(self, clock):
        """ConsensusNode::update_node(clock: NodeTime) -> NodeUpdateActions (librabft-v2/src/node.rs:240-304); ``0 <= clock <= 2**31 - 3``."""
        a = LbftActions()
        self._sim._mutated()
        check(_lib.lib().lbft_node_update(self._sim._h, self.instance, self.author, int(clock), C.byref(a)))
        return a.as_dict()

    def create_notification(self):
        """DataSyncNode::create_notification (librabft-v2/src/data_sync.rs:82-111) -> opaque handle."""
        h = C.c_uint32()
        check(_lib.lib().lbft_node_create_notification(self._sim._h, self.instance, self.author, C.byref(h)))
        return (self.author, int(h.value))

    def handle_notification(self, notification):
        """DataSyncNode::handle_notification (data_sync.rs:113-177); True when the reference returns Some(request)."""
        sender, handle = notification
        sync = C.c_uint32()
        self._sim._mutated()
        check(_lib.lib().lbft_node_handle_notification(self._sim._h, self.instance, self.author, sender, handle, C.byref(sync)))
        return bool(sync.value)

    def create_request(self):
        """DataSyncNode::create_request (data_sync.rs:66-71,179-181) -> opaque handle (batches with quirks bit 0)."""
        h = C.c_uint32()
        check(_lib.lib().lbft_node_create_request(self._sim._h, self.instance, self.author, C.byref(h)))
        return (self.author, int(h.value))

    def handle_request(self, request):
        """DataSyncNode::handle_request (data_sync.rs:183-207): the records the requester lacks -> opaque response handle."""
        _, handle = request
        h = C.c_uint32()
        self._sim._mutated()
        check(_lib.lib().lbft_node_handle_request(self._sim._h, self.instance, self.author, handle, C.byref(h)))
        return (self.author, int(h.value))

    def handle_response(self, response, clock):
        """DataSyncNode::handle_response(response, clock) (data_sync.rs:209-240); ``0 <= clock <= 2**31 - 3``."""
        peer, handle = response
        self._sim._mutated()
        check(_lib.lib().lbft_node_handle_response(self._sim._h, self.instance, self.author, peer, handle, int(clock)))

    def release(self, message):
        """Drops a notification / request / response handle."""
        check(_lib.lib().lbft_node_release_notification(self._sim._h, self.instance, message[1]))

    def save_node(self):
        """ConsensusNode::save_node (node.rs:233-238) -> the bincode image of this node's NodeState."""
        return self._sim.save_node(self.instance, self.author)

    def load_node(self, image, clock):
        """ConsensusNode::load_node (node.rs:211-231): restore this node's NodeState from a save_node image; `clock` = the node's time
        (the reference refuses "saved state from the future"); only compared with the image's times, so any integer is accepted."""
        self._sim.load_node(self.instance, self.author, image, clock)

    def view(self):
        v = LbftNodeView()
        check(_lib.lib().lbft_node_view_get(self._sim._h, self.instance, self.author, C.byref(v)))
        return v.as_dict()


class Simulator:
    """``Simulator::new(rng_seed, num_nodes, network_delay, context_factory)`` for one network.

    The reference's ``context_factory`` closure (librabft-v2/src/main.rs:23-34) only carries
    ``commands_per_epoch`` and the ``NodeConfig``; pass them directly."""

    def __init__(self, rng_seed, num_nodes, network_delay, node_config=None, commands_per_epoch=30000, **kw):
        self._batch = BatchSimulator([rng_seed], num_nodes, network_delay, node_config, commands_per_epoch, **kw)

    @classmethod
    def new(cls, rng_seed, num_nodes, network_delay, node_config=None, commands_per_epoch=30000, **kw):
        return cls(rng_seed, num_nodes, network_delay, node_config, commands_per_epoch, **kw)

    def loop_until(self, max_clock, csv_path=None):
        self.result = self._batch.loop_until(max_clock, csv_path)
        return self.result.contexts(0)
