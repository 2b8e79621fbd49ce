#!/usr/bin/env python3
"""Cost of the per-instance statistics on the device against the read-back they replace and against the three grouped calls whose
samples they keep per instance (EXPERIMENTS.md "Per-instance statistics"; raw outputs in profiles/instance_stats/).  One JSON line per
case.

    python tools/instance_stats_timing.py                      # wall times, warm, in one process
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/instance_stats_timing.py --calls 3 --no-readback
                                                                # for a kernel trace of lbft_k_ct_instances and the grouped kernels

Per batch -- the headline shape with commit times (65 536 x 4 nodes, clock 1000), a lossy one of 32-node networks (4 096 x 32, 2 % loss,
clock 500) and the partition scenario (a control set and nodes {0, 1} of 4 cut off during [300, 600), quirks = 3, 32 seeds each, clock
1500) --: instance_stats(), then latency_histogram(), stall_histogram() and finality_histogram() (each alone and the three in a row),
seed_spread(), then commit_times() + committed_histories() read back.  The first call of each timed loop is dropped.  The rows are
checked against the grouped calls (per group, the samples and sums of the rows add up to theirs); --check compares them with the numpy
reference (tests/instance_stats_reference.py) on a batch of the first --check seeds."""
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
        set_of = np.asarray(sim.set_of_instance) if groups > 1 else np.zeros(sim.num_instances, dtype=np.int64)
        row = {"case": name, "kernel_class": layout["kernel_class"], "lanes_per_wavefront": layout["lanes_per_wavefront"],
               "faulted": int((res.faults != 0).sum()), "groups": groups, "run_ms": sim.last_run_ms()[1]}

        def three():
            return res.latency_histogram()[1], res.stall_histogram("partition_end")[1], res.finality_histogram()[3]
        for key, fn in (("instance_stats", lambda: res.instance_stats("partition_end")), ("latency", res.latency_histogram),
                        ("stalls", lambda: res.stall_histogram("partition_end")), ("finality", res.finality_histogram), ("grouped_three", three),
                        ("seed_spread", lambda: res.seed_spread("partition_end"))):
            ms, out = timed(fn, args.calls)
            row[key + "_ms"] = [round(v, 4) for v in ms]
            row[key + "_median_ms"] = float(np.median(ms))
            if key == "instance_stats":
                rows = out
            if key == "grouped_three":
                whole = np.concatenate(out, axis=1).reshape(groups, 11, 4)
        row["grouped_over_instance_stats"] = row["grouped_three_median_ms"] / row["instance_stats_median_ms"]
        row["samples"] = [int(v) for v in rows[:, :, 0].sum(axis=0)]
        row["sums"] = [int(v) for v in rows[:, :, 1].sum(axis=0)]
        row["max"] = [int(v) for v in rows[:, :, 3].max(axis=0)]
        row["rows_digest"] = int(np.bitwise_xor.reduce(rows.ravel() * np.arange(1, rows.size + 1, dtype=np.uint64)))
        row["rows_add_up_to_the_grouped_calls"] = bool(all((rows[set_of == g][:, :, :2].sum(axis=0) == whole[g, :, :2]).all() for g in range(groups)))
        if not args.no_readback:
            def readback():
                fresh = L.BatchResult(sim)  # (nothing cached)
                ct = fresh.commit_times()
                return ct, fresh.committed_histories(ct.shape[2])
            ms, out = timed(readback, min(args.calls, 3))
            row["readback_ms"] = [round(v, 3) for v in ms]
            row["readback_median_ms"] = float(np.median(ms))
            row["readback_bytes"] = int(out[0].nbytes + out[1].nbytes)
            row["readback_over_instance_stats"] = row["readback_median_ms"] / row["instance_stats_median_ms"]
        if args.check and groups == 1:
            import instance_stats_reference as ref
            kw = dict(drop_per_million=20000) if "lossy" in name else {}
            small = L.BatchSimulator.new(np.arange(1, args.check + 1, dtype=np.uint64), sim.num_nodes, L.RandomDelay.new(10.0, 4.0), commit_times=True, **kw)
            sres = small.loop_until(max_clock, allow_faults=True)
            row["equals_numpy_on_%d" % args.check] = bool((sres.instance_stats() == ref.instance_stats(sres, max_clock)).all())
            small.close()
        print(json.dumps(row), flush=True)
        sim.close()


if __name__ == "__main__":
    main()
