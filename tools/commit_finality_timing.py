#!/usr/bin/env python3
"""Cost of commit finality on the device against the read-back it replaces and against the other statistics of a timed batch
(EXPERIMENTS.md "Commit finality"; raw outputs in profiles/commit_finality/).  One JSON line per case.

    python tools/commit_finality_timing.py                      # wall times, warm, in one process
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/commit_finality_timing.py --calls 3 --no-readback
                                                                # for a kernel trace of lbft_k_ct_finality and its neighbours

Per batch -- the headline shape with commit times (65 536 x 4 nodes, clock 1000), a lossy one of 32-node networks (4 096 x 32, 2 % loss,
clock 500) and the partition scenario (a control set and nodes {0, 1} of 4 cut off during [300, 600), quirks = 3, 32 seeds each, clock
1500) --: finality_histogram(), latency_histogram(), commit_series(), stall_histogram(), then commit_times() + committed_histories()
read back.  The first call of each timed loop is dropped.  --check compares the device's arrays with the numpy reference
(tests/commit_finality_reference.py) on the read-back of the first --check instances."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

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
    if "scenario" in which:
        sets = [L.ParamSet(d, L.NodeConfig()), L.ParamSet(d, L.NodeConfig(), partition=(2, 300, 600))]
        set_of = np.repeat(np.arange(2), 32).astype(np.uint32)
        seeds = np.tile(np.arange(1, 33), 2).astype(np.uint64)
        yield "scenario 2 sets x 32 x 4, clock 1500", L.BatchSimulator.with_param_sets(seeds, 4, sets, set_of, quirks=3, commit_times=True), 1500


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--cases", default="headline,lossy,scenario")
    ap.add_argument("--no-readback", action="store_true", help="skip the read-back")
    ap.add_argument("--check", type=int, default=0, metavar="N", help="compare with the numpy reference on a batch of the first N seeds")
    args = ap.parse_args()
    for name, sim, max_clock in cases(args.cases.split(",")):
        res = sim.loop_until(max_clock, allow_faults=True)
        layout = sim.layout()
        groups = len(sim.param_sets) if sim.param_sets is not None else 1
        row = {"case": name, "kernel_class": layout["kernel_class"], "lanes_per_wavefront": layout["lanes_per_wavefront"],
               "faulted": int((res.faults != 0).sum()), "groups": groups, "run_ms": sim.last_run_ms()[1]}
        for key, fn in (("finality", res.finality_histogram), ("latency", res.latency_histogram), ("series", res.commit_series),
                        ("stalls", res.stall_histogram)):
            ms, out = timed(fn, args.calls)
            row[key + "_ms"] = [round(v, 4) for v in ms]
            row[key + "_median_ms"] = float(np.median(ms))
            if key == "finality":
                stats = out[3]
        row["samples"] = [int(v) for v in stats[:, 0::4].sum(axis=0)]
        row["sums"] = [int(v) for v in stats[:, 1::4].sum(axis=0)]
        row["max"] = [int(v) for v in stats[:, 3::4].max(axis=0)]
        row["stats_digest"] = int(np.bitwise_xor.reduce(stats.ravel() * np.arange(1, stats.size + 1, dtype=np.uint64)))
        if groups > 1:
            row["by_set"] = res.finality_by_param_set()
        if not args.no_readback:
            def readback():
                fresh = L.BatchResult(sim)  # (nothing cached)
                ct = fresh.commit_times()
                return ct, fresh.committed_histories(ct.shape[2])
            for part, fn in (("commit_times", lambda: L.BatchResult(sim).commit_times()), ("committed_histories", lambda: L.BatchResult(sim).committed_histories()),
                             ("readback", readback)):
                ms, out = timed(fn, min(args.calls, 3))
                row[part + "_ms"] = [round(v, 3) for v in ms]
                row[part + "_median_ms"] = float(np.median(ms))
            row["readback_bytes"] = int(out[0].nbytes + out[1].nbytes)
            row["readback_over_finality"] = row["readback_median_ms"] / row["finality_median_ms"]
        if args.check and groups == 1:
            import commit_finality_reference as ref
            kw = dict(drop_per_million=20000) if "lossy" in name else {}
            small = L.BatchSimulator.new(np.arange(1, args.check + 1, dtype=np.uint64), sim.num_nodes, L.RandomDelay.new(10.0, 4.0), commit_times=True, **kw)
            sres = small.loop_until(max_clock, allow_faults=True)
            want = ref.bin_finality(*ref.of_result(sres), 1, max_clock + 1)
            row["equals_numpy_on_%d" % args.check] = bool(all((a == b).all() for a, b in zip(sres.finality_histogram(), want)))
            small.close()
        print(json.dumps(row), flush=True)
        sim.close()


if __name__ == "__main__":
    main()
