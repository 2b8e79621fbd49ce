"""TEST INFRASTRUCTURE: commit times derived from the CPU oracle, the reference answer for BatchResult.commit_times.

The oracle records no commit clock, so it is derived from fresh runs: the commit time of entry k of node j is the smallest t for which a
fresh run of the same seed to loop_until(t) leaves node j with more than k commits.  (Fresh runs: loop_until drops the first event past
max_clock, so repeated calls on one simulator are not a valid reference.)  Found by bisection on t, each step re-running only the
instances whose commit counts still change inside the interval."""
import numpy as np


def commit_times(oracle, cfg, seeds, max_clock, cap, threads=8):
    """[instance, node, cap] int64 commit times of the oracle runs of `cfg` with `seeds` to `max_clock`, -1 padded."""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    m, n = len(seeds), cfg.num_nodes
    out = np.full((m, n, cap), -1, dtype=np.int64)

    def counts(idx, t):
        return oracle.run_batch(cfg, seeds[idx], t, threads=threads)["commit_counts"].astype(np.int64)

    def assign(idx, lo_counts, hi_counts, t):
        for r, i in enumerate(idx):
            for j in range(n):
                a, b = int(lo_counts[r, j]), min(int(hi_counts[r, j]), cap)
                if b > a:
                    out[i, j, a:b] = t

    every = np.arange(m)
    c0 = counts(every, 0)
    assign(every, np.zeros_like(c0), c0, 0)
    stack = [(every, 0, int(max_clock), c0, counts(every, int(max_clock)))]
    while stack:
        idx, lo, hi, clo, chi = stack.pop()
        moving = (clo != chi).any(axis=1)
        idx, clo, chi = idx[moving], clo[moving], chi[moving]
        if not len(idx):
            continue
        if hi - lo == 1:
            assign(idx, clo, chi, hi)
            continue
        mid = (lo + hi) // 2
        cm = counts(idx, mid)
        stack.append((idx, lo, mid, clo, cm))
        stack.append((idx, mid, hi, cm, chi))
    return out


def param_set_commit_times(oracle, configs, set_of, seeds, max_clock, cap, threads=8):
    """The same for a parameter-set batch: `configs[k]` is the oracle configuration of set k, instance i runs configs[set_of[i]]."""
    set_of = np.asarray(set_of)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    out = np.full((len(seeds), configs[0].num_nodes, cap), -1, dtype=np.int64)
    for k, cfg in enumerate(configs):
        idx = np.nonzero(set_of == k)[0]
        if len(idx):
            out[idx] = commit_times(oracle, cfg, seeds[idx], max_clock, cap, threads)
    return out


def latencies(commit_times_, histories, startup_times, faults=None):
    """Flat int64 latencies commit_time - (startup[proposer] + time) of every recorded entry (instances with a fault skipped), and the
    instance of each sample."""
    ct = np.asarray(commit_times_)
    m, n, cap = ct.shape
    rec = ct >= 0
    if faults is not None:
        rec &= (np.asarray(faults) == 0)[:, None, None]
    inst = np.broadcast_to(np.arange(m)[:, None, None], ct.shape)[rec]
    proposer = histories["proposer"][:, :, :cap][rec].astype(np.int64)
    start = np.asarray(startup_times, dtype=np.int64)[inst, proposer]
    lat = ct[rec] - (start + histories["time"][:, :, :cap][rec].astype(np.int64))
    return lat, inst
