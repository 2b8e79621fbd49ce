#!/usr/bin/env python3
"""Cost of the chain statistics on the device against what the same answer costs without them: reading every history and the startup
times back and walking them in numpy (EXPERIMENTS.md "Chain statistics"; raw outputs in profiles/chain_stats/).  One JSON line per case.

    python tools/chain_stats_timing.py                      # wall times, warm, in one process
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/chain_stats_timing.py --calls 3 --no-readback
                                                            # for a kernel trace of lbft_k_cs_chain

Per batch -- the headline one (65 536 x 4 nodes, clock 1000), the large one (8 192 x 100 nodes, clock 300) and a grid of 64 parameter
sets of 1 024 four-node networks each (clock 1000) --: chain_stats(), then committed_histories() + startup_times + commit_counts + faults
read back, then the numpy reference (tests/chain_stats_reference.py) on what was read back, once; its arrays are compared with the
device's.  The first call of each timed loop is dropped."""
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
        yield "65536x4, clock 1000", L.BatchSimulator.new(np.arange(1, 65537, dtype=np.uint64), 4, d), 1000
    if "large" in which:
        yield "8192x100, clock 300", L.BatchSimulator.new(np.arange(1, 8193, dtype=np.uint64), 100, d), 300
    if "grid" in which:
        sets = [L.ParamSet(L.RandomDelay.new(mean, 4.0), L.NodeConfig(100000, delta, 2.0, lam))
                for mean in (8.0, 10.0, 12.0, 14.0) for delta in (10, 15, 20, 30) for lam in (0.25, 0.5, 0.75, 1.0)]
        k = np.arange(64 * 1024)
        yield "64 sets x 1024 x 4, clock 1000", L.BatchSimulator.with_param_sets((1 + k // 64).astype(np.uint64), 4, sets, (k % 64).astype(np.uint32)), 1000


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--cases", default="headline,large,grid")
    ap.add_argument("--no-readback", action="store_true", help="skip the read-back and the numpy reference")
    args = ap.parse_args()
    for name, sim, max_clock in cases(args.cases.split(",")):
        res = sim.loop_until(max_clock, allow_faults=True)
        layout = sim.layout()
        groups = len(sim.param_sets) if sim.param_sets is not None else 1
        row = {"case": name, "kernel_class": layout["kernel_class"], "lanes_per_wavefront": layout["lanes_per_wavefront"],
               "faulted": int((res.faults != 0).sum()), "groups": groups}
        row["chain_stats_ms"], (hist, authors, stats) = timed(res.chain_stats, args.calls)
        row["chain_stats_median_ms"] = float(np.median(row["chain_stats_ms"]))
        row["samples"] = [int(v) for v in stats[:, 0::4].sum(axis=0)]
        row["sums"] = [int(v) for v in stats[:, 1::4].sum(axis=0)]
        row["max"] = [int(v) for v in stats[:, 3::4].max(axis=0)]
        if not args.no_readback:
            def readback():
                fresh = L.BatchResult(sim)  # (nothing cached)
                return fresh.committed_histories(), fresh.commit_counts, fresh.startup_times, fresh.faults
            row["readback_ms"], (histories, counts, startup, faults) = timed(readback, min(args.calls, 3))
            row["readback_median_ms"] = float(np.median(row["readback_ms"]))
            row["histories_bytes"] = int(histories.nbytes)
            import chain_stats_reference as ref
            set_of = getattr(sim, "set_of_instance", None) if sim.param_sets is not None else None
            t0 = time.perf_counter()
            want = ref.chain_stats(histories, counts, startup, faults, set_of, groups, 1, max_clock + 1)
            row["numpy_reference_ms"] = (time.perf_counter() - t0) * 1e3
            row["equals_numpy"] = bool(all((a == b).all() for a, b in zip((hist, authors, stats), want)))
            row["readback_plus_numpy_over_chain_stats"] = (row["readback_median_ms"] + row["numpy_reference_ms"]) / row["chain_stats_median_ms"]
            row["readback_over_chain_stats"] = row["readback_median_ms"] / row["chain_stats_median_ms"]
        print(json.dumps(row), flush=True)
        sim.close()


if __name__ == "__main__":
    main()
