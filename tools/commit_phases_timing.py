#!/usr/bin/env python3
"""Cost of the commit phases on the device against the two grouped calls whose samples they split and against the read-back they
replace (EXPERIMENTS.md "Commit phases"; raw outputs in profiles/commit_phases/).  One JSON line per case.

    python tools/commit_phases_timing.py                      # wall times, warm, in one process
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/commit_phases_timing.py --calls 3 --no-readback
                                                                # for a kernel trace of lbft_k_ct_phases and the two grouped kernels
    LBFT_HIP_LIB=<dir>/liblbft_hip.so python tools/commit_phases_timing.py --no-readback
                                                                # another build of the libraries (the other accumulation form)

Per batch -- the headline shape with commit times (65 536 x 4 nodes, clock 1000) and a lossy one of 32-node networks (4 096 x 32, 2 %
loss, clock 500) --: phase_histogram() with 1, 3 and 8 phases (edges spread evenly over the clock), then latency_histogram() and
finality_histogram() (each alone and the two in a row), then commit_times() + committed_histories() read back.  The first call of each
timed loop is dropped.  The result is checked in place: one phase equals the two grouped calls, and the phases add up to it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import librabft_simulator_amd as L  # noqa: E402


def timed(fn, calls):
    ms = []
    for _ in range(calls + 1):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[1:], out


def cases(which):
    d = L.RandomDelay.new(10.0, 4.0)
    if "headline" in which:
        yield "65536x4, clock 1000", L.BatchSimulator.new(np.arange(1, 65537, dtype=np.uint64), 4, d, commit_times=True), 1000
    if "lossy" in which:
        yield "4096x32 lossy, clock 500", L.BatchSimulator.new(np.arange(1, 4097, dtype=np.uint64), 32, d, drop_per_million=20000, commit_times=True), 500


def even_edges(phases, max_clock):
    return [(max_clock + 1) * q // phases for q in range(1, phases)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--cases", default="headline,lossy")
    ap.add_argument("--no-readback", action="store_true", help="skip the read-back")
    args = ap.parse_args()
    for name, sim, max_clock in cases(args.cases.split(",")):
        res = sim.loop_until(max_clock, allow_faults=True)
        layout = sim.layout()
        row = {"case": name, "library": os.environ.get("LBFT_HIP_LIB", "product"), "kernel_class": layout["kernel_class"],
               "faulted": int((res.faults != 0).sum()), "run_ms": sim.last_run_ms()[1]}

        def two():
            return res.latency_histogram(), res.finality_histogram()
        results = {}
        for key, fn in [("phases_%d" % k, (lambda k=k: res.phase_histogram(even_edges(k, max_clock)))) for k in (1, 3, 8)] + \
                       [("latency", res.latency_histogram), ("finality", res.finality_histogram), ("grouped_two", two)]:
            ms, results[key] = timed(fn, args.calls)
            row[key + "_ms"] = [round(v, 4) for v in ms]
            row[key + "_median_ms"] = float(np.median(ms))
        (l_hist, l_stats), (f_hist, _, _, f_stats) = results["grouped_two"]
        lat, fin, stats = results["phases_1"]
        row["one_phase_is_the_grouped_calls"] = bool((lat[:, 0] == l_hist).all() and (fin[:, 0] == f_hist).all() and (stats[:, 0, 0] == l_stats).all()
                                                     and (stats[:, 0, 1:].reshape(-1, 20) == f_stats[:, :20]).all())
        for k in (3, 8):
            lat_k, fin_k, stats_k = results["phases_%d" % k]
            have = stats_k[:, :, :, 0] > 0
            row["phases_%d_add_up" % k] = bool((lat_k.sum(axis=1) == lat[:, 0]).all() and (fin_k.sum(axis=1) == fin[:, 0]).all()
                                               and (stats_k[:, :, :, :2].sum(axis=1) == stats[:, 0, :, :2]).all()
                                               and (np.where(have, stats_k[:, :, :, 3], 0).max(axis=1) == stats[:, 0, :, 3]).all())
            row["phases_%d_samples" % k] = [int(v) for v in stats_k[0, :, 3, 0]]  # quorum samples per phase
        row["phases_3_over_grouped_two"] = row["phases_3_median_ms"] / row["grouped_two_median_ms"]
        if not args.no_readback:
            def readback():
                fresh = L.BatchResult(sim)  # (nothing cached)
                ct = fresh.commit_times()
                return ct, fresh.committed_histories(ct.shape[2])
            ms, out = timed(readback, min(args.calls, 3))
            row["readback_ms"] = [round(v, 3) for v in ms]
            row["readback_median_ms"] = float(np.median(ms))
            row["readback_bytes"] = int(out[0].nbytes + out[1].nbytes)
            row["readback_over_phases_3"] = row["readback_median_ms"] / row["phases_3_median_ms"]
        print(json.dumps(row), flush=True)
        sim.close()


if __name__ == "__main__":
    main()
