"""TEST INFRASTRUCTURE: commit times derived from the CPU oracle, the reference answer for BatchResult.commit_times.

The oracle records no commit clock, so it is derived from fresh runs: the commit time of entry k of node j is the smallest t for which a
fresh run of the same seed to loop_until(t) leaves node j with more than k commits.  (Fresh runs: loop_until drops the first event past
max_clock, so repeated calls on one simulator are not a valid reference.)  Found by bisection on t, each step re-running only the
instances whose commit counts still change inside the interval.  Also the numpy reference of the device latency histogram."""
import numpy as np
import pytest


def commit_times(oracle, cfg, seeds, max_clock, cap, threads=8):
    """[instance, node, cap] int64 commit times of the oracle runs of `cfg` with `seeds` to `max_clock`, -1 padded."""
    from concurrent.futures import ThreadPoolExecutor
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    m, n = len(seeds), cfg.num_nodes
    out = np.full((m, n, cap), -1, dtype=np.int64)

    def counts(idx, t, th=threads):
        return oracle.run_batch(cfg, seeds[idx], t, threads=th)["commit_counts"].astype(np.int64)

    def assign(idx, lo_counts, hi_counts, t):
        for r, i in enumerate(idx):
            for j in range(n):
                a, b = int(lo_counts[r, j]), min(int(hi_counts[r, j]), cap)
                if b > a:
                    out[i, j, a:b] = t

    every = np.arange(m)
    c0 = counts(every, 0)
    assign(every, np.zeros_like(c0), c0, 0)
    # breadth first: the midpoints of one level are independent runs, spread over `threads` single-threaded oracle calls
    level = [(every, 0, int(max_clock), c0, counts(every, int(max_clock)))]
    with ThreadPoolExecutor(max(1, threads)) as pool:
        while level:
            split = []
            for idx, lo, hi, clo, chi in level:
                moving = (clo != chi).any(axis=1)
                idx, clo, chi = idx[moving], clo[moving], chi[moving]
                if not len(idx):
                    continue
                if hi - lo == 1:
                    assign(idx, clo, chi, hi)
                    continue
                split.append((idx, lo, hi, clo, chi))
            mids = list(pool.map(lambda w: counts(w[0], (w[1] + w[2]) // 2, 1), split))
            level = []
            for (idx, lo, hi, clo, chi), cm in zip(split, mids):
                mid = (lo + hi) // 2
                level += [(idx, lo, mid, clo, cm), (idx, mid, hi, cm, chi)]
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


def numpy_histogram(res, width, bins, set_of=None, groups=1):
    """What BatchResult.latency_histogram(width, bins) must return for the BatchResult `res`, computed in numpy from its commit times,
    histories, startup times and fault words: (hist [groups, bins] uint64, stats [groups, 4] uint64, the latencies, their group)."""
    ct = res.commit_times()
    lat, inst = latencies(ct, res.committed_histories(ct.shape[2]), res.startup_times, res.faults)
    g = np.zeros(len(lat), dtype=np.int64) if set_of is None else np.asarray(set_of, dtype=np.int64)[inst]
    hist = np.zeros((groups, bins), dtype=np.uint64)
    stats = np.zeros((groups, 4), dtype=np.uint64)
    binned = np.minimum(lat // width, bins - 1)
    for k in range(groups):
        sel = g == k
        hist[k] = np.bincount(binned[sel], minlength=bins)
        if sel.any():
            stats[k] = (sel.sum(), lat[sel].sum(), lat[sel].min(), lat[sel].max())
    return hist, stats, lat, g


def same_results(a, b):
    """Two BatchResults of the same batch run two ways (timed and untimed, stepped and straight ...) agree on everything but commit times."""
    for name in ("commit_counts", "last_committed_states", "active_rounds", "startup_times", "faults", "epochs"):
        assert (getattr(a, name) == getattr(b, name)).all(), name
    cap = int(a.commit_counts.max())
    assert (a.committed_histories(cap) == b.committed_histories(cap)).all()
    ca, cb = a.counters, b.counters
    for name in ("events", "rng_draws", "rounds", "commits", "events_scheduled", "faulted_instances", "max_queue", "max_snapshots", "max_blocks"):
        assert ca[name] == cb[name], name


QUANTILES = (0.0, 0.1, 0.5, 0.9, 0.99, 1.0)


def check_default_latency(res, max_clock, set_of=None, groups=1):
    """latency_histogram() and latency_by_param_set() with their default binning -- width 1 up to 65 536 bins, above that the smallest
    width that fits -- against numpy.  Quantiles are then lower bin edges: (the inverted-CDF quantile // width) * width.  Returns the
    default (width, bins)."""
    span = max_clock + 1
    width = max(1, -(-span // (1 << 16)))
    bins = -(-span // width)
    hist, stats = res.latency_histogram()
    assert hist.shape == (groups, bins)
    h_np, s_np, lat, g = numpy_histogram(res, width, bins, set_of, groups)
    assert (hist == h_np).all() and (stats == s_np).all(), (width, bins)
    rows = res.latency_by_param_set(QUANTILES)
    assert len(rows) == groups
    for k, row in enumerate(rows):
        lk = lat[g == k]
        if not len(lk):
            assert row["samples"] == 0 and row["mean"] is None and row["min"] is None and row["max"] is None, row
            assert all(v is None for v in row["quantiles"].values()), row
            continue
        assert row["samples"] == len(lk) and row["min"] == lk.min() and row["max"] == lk.max(), (k, row)
        assert row["mean"] == pytest.approx(lk.mean(), rel=1e-12), (k, row)
        for q in QUANTILES:
            assert row["quantiles"][str(q)] == int(np.quantile(lk, q, method="inverted_cdf")) // width * width, (k, q, width)
    return width, bins
