#!/usr/bin/env python3
"""Cost of the commit timelines on the device against the read-back they replace (EXPERIMENTS.md "Commit timelines"; raw outputs in
profiles/commit_timeline/).  One JSON line per case.

    python tools/commit_timeline_timing.py                  # wall times, warm, in one process
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/commit_timeline_timing.py --calls 3 --no-readback
                                                           # for a kernel trace of lbft_k_ct_timeline

Per batch -- the headline one (65 536 x 4, clock 1000) and the 64-point grid x 1 024 --: (a) commit_series() + stall_histogram(), wall time
around the two calls; (b) commit_times() alone, the read-back without any numpy; and latency_histogram() for scale.  The first call of
each is dropped."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import librabft_simulator_amd as L  # noqa: E402
from librabft_simulator_amd import grid  # noqa: E402


def grid64():
    sets = [L.ParamSet(L.RandomDelay.new(m, 4.0), L.NodeConfig(100000, d, 2.0, lam)) for m in (5.0, 10.0, 20.0, 40.0) for d in (10, 20, 40, 80)
            for lam in (0.25, 0.5, 0.75, 1.0)]
    set_of, si = grid.set_assignment(len(sets), 1024, "blocked")
    return sets, set_of, (1 + si).astype(np.uint64)


def timed(fn, calls):
    ms = []
    for _ in range(calls + 1):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[1:], out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--no-readback", action="store_true", help="skip (b), the commit_times() read-back")
    args = ap.parse_args()
    d = L.RandomDelay.new(10.0, 4.0)
    cases = [("65536x4", L.BatchSimulator.new(np.arange(1, 65537, dtype=np.uint64), 4, d, commit_times=True))]
    sets, set_of, gseeds = grid64()
    cases.append(("64-point grid x 1024", L.BatchSimulator.with_param_sets(gseeds, 4, sets, set_of, commit_times=True)))
    for name, sim in cases:
        res = sim.loop_until(1000, allow_faults=True)
        cap = max(int(res.commit_counts.max()), 1)
        row = {"case": name, "groups": 1 if sim.param_sets is None else len(sim.param_sets)}
        both, (series, (hist, stats)) = timed(lambda: (res.commit_series(), res.stall_histogram()), args.calls)
        row["a_series_plus_stalls_ms"] = both
        row["series_ms"], _ = timed(res.commit_series, args.calls)
        row["stalls_ms"], _ = timed(res.stall_histogram, args.calls)
        row["latency_histogram_ms"], _ = timed(res.latency_histogram, args.calls)
        if not args.no_readback:
            row["b_commit_times_ms"], ct = timed(lambda: res.commit_times(cap), args.calls)
            row["read_back_int64_bytes"] = int(ct.nbytes)
            row["a_median_ms"], row["b_median_ms"] = float(np.median(both)), float(np.median(row["b_commit_times_ms"]))
            row["a_not_above_b"] = bool(row["a_median_ms"] <= row["b_median_ms"])
        row["entries"], row["gaps"], row["bins"] = int(series.sum()), int(stats[:, 0].sum()), int(hist.shape[1])
        print(json.dumps(row), flush=True)
        sim.close()


if __name__ == "__main__":
    main()
