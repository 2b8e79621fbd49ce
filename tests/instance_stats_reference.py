"""TEST INFRASTRUCTURE: numpy reference of the per-instance statistics (include/lbft.h: lbft_batch_instance_stats).  Nothing new is
computed here: the definition says that row i is what the grouped calls would report if instance i were a group of its own, so this
module calls the existing numpy references of those calls with ``set_of = arange(m)`` and ``groups = m`` --
commit_times_oracle.numpy_histogram (family 0), commit_timeline_reference.stalls (families 1 to 4) and
commit_finality_reference.finality (families 5 to 10) -- and puts their statistics side by side."""
import numpy as np

import commit_finality_reference as fin_ref
import commit_timeline_reference as tl_ref
import commit_times_oracle as cto

FAMILIES = 11
INSTANCE_STATS = 44  # LBFT_INSTANCE_STATS
NAMES = ("latency", "gaps", "first", "tail", "longest", "finality_first", "finality_valid", "finality_quorum", "finality_all", "spread", "open")
LATENCY, GAPS, FIRST, TAIL, LONGEST, FIN_FIRST, FIN_VALID, FIN_QUORUM, FIN_ALL, SPREAD, OPEN = range(11)
SAMPLES, SUM, MIN, MAX = range(4)


class Readbacks:
    """What the references read of a BatchResult, for data that no batch produced: commit times [m, n, cap] (-1 = not recorded),
    histories [m, n, cap] of (proposer, index, time) records, commit counts and startup times [m, n], fault words [m]."""

    def __init__(self, commit_times, histories, commit_counts, startup_times, faults=None):
        self._ct = np.asarray(commit_times).astype(np.int64)
        self._hist = histories
        self.commit_counts = np.asarray(commit_counts)
        self.startup_times = np.asarray(startup_times).astype(np.int64)
        self.faults = np.zeros(self._ct.shape[0], dtype=np.uint32) if faults is None else np.asarray(faults, dtype=np.uint32)

    def commit_times(self, cap_per_node=None):
        return self._ct if cap_per_node is None else self._ct[:, :, :cap_per_node]

    def committed_histories(self, cap_per_node=None):
        return self._hist if cap_per_node is None else self._hist[:, :, :cap_per_node]


def instance_stats(res, max_clock, since=None, set_of=None, rights=None, rotation=0, commands_per_epoch=30000, log_capacity=None):
    """[m, 11, 4] uint64 from the read-backs of `res` (a BatchResult or a Readbacks).  since: None or one value per group of `set_of`
    (None: one group); it is applied to every instance of the group."""
    ct = res.commit_times()
    m = ct.shape[0]
    own = np.arange(m)
    if since is not None:
        since = np.asarray(since, dtype=np.int64).reshape(-1)
        since = since[np.zeros(m, dtype=np.int64) if set_of is None else np.asarray(set_of, dtype=np.int64)]
    _, latency, _, _ = cto.numpy_histogram(res, 1, 1, own, m)
    _, stalls = tl_ref.stalls(ct, res.commit_counts, res.faults, own, m, since, 1, 1, max_clock)
    _, _, _, finality = fin_ref.finality(ct, res.commit_counts, res.committed_histories(ct.shape[2]), res.startup_times, res.faults, rights,
                                         rotation, commands_per_epoch, own, m, 1, 1, log_capacity)
    out = np.concatenate([latency, stalls, finality], axis=1).astype(np.uint64)
    assert out.shape == (m, INSTANCE_STATS)
    return out.reshape(m, FAMILIES, 4)
