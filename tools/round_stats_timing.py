#!/usr/bin/env python3
"""Cost of the round statistics on the device and of the bulk read-back, against the one-instance-per-call route they replace
(EXPERIMENTS.md "Round statistics"; raw outputs in profiles/round_stats/).  One JSON line per case.

    python tools/round_stats_timing.py                      # wall times, warm, in one process
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/round_stats_timing.py --calls 3 --no-readback
                                                            # for a kernel trace of lbft_k_rs_rounds

Per batch -- a mid-class one (4 096 x 16 nodes, 2 % loss, clock 1000; word-interleaved tiles) and a large-class one (1 024 x 40 nodes,
clock 300; instance-major rows) --: round_histogram(), round_tables(), and the loop of round_switches(i) over the first `--loop`
instances, scaled to the batch.  The first call of each is dropped.  With --check the device arrays are compared with the numpy
reference (tests/round_stats_reference.py) on round_tables()'s own tables."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--loop", type=int, default=1024, help="instances of the round_switches(i) loop")
    ap.add_argument("--no-readback", action="store_true", help="skip round_tables() and the round_switches(i) loop")
    ap.add_argument("--check", action="store_true", help="compare with the numpy reference on round_tables()'s tables")
    args = ap.parse_args()
    d = L.RandomDelay.new(10.0, 4.0)
    cases = [("4096x16 lossy, clock 1000", L.BatchSimulator.new(np.arange(1, 4097, dtype=np.uint64), 16, d, drop_per_million=20000), 1000, 264),
             ("1024x40, clock 300", L.BatchSimulator.new(np.arange(1, 1025, dtype=np.uint64), 40, d), 300, 128)]
    for name, sim, max_clock, trace in cases:
        res = sim.loop_until(max_clock, allow_faults=True, round_trace=trace)
        layout = sim.layout()
        row = {"case": name, "kernel_class": layout["kernel_class"] & 0xff, "lanes_per_wavefront": layout["lanes_per_wavefront"],
               "faulted": int((res.faults != 0).sum())}
        row["round_histogram_ms"], (stay, skew, stats) = timed(res.round_histogram, args.calls)
        row["round_histogram_median_ms"] = float(np.median(row["round_histogram_ms"]))
        row["samples"] = [int(v) for v in stats[0, 0::4]]
        if not args.no_readback:
            row["round_tables_ms"], (tables, max_rounds, _) = timed(res.round_tables, args.calls)
            row["round_tables_median_ms"] = float(np.median(row["round_tables_ms"]))
            row["tables_int64_bytes"], row["rows"] = int(tables.nbytes), int(tables.shape[1])
            k = min(args.loop, sim.num_instances)
            loop, _ = timed(lambda: [res.round_switches(i) for i in range(k)], 2)
            row["round_switches_loop_instances"] = k
            row["round_switches_loop_ms"] = loop
            row["round_switches_loop_scaled_to_batch_ms"] = float(np.median(loop)) * sim.num_instances / k
            if args.check:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import round_stats_reference as ref
                want = ref.round_stats(tables, max_rounds, res.faults, None, 1, 1, max_clock + 1)
                row["equals_numpy"] = bool(all((a == b).all() for a, b in zip((stay, skew, stats), want)))
        print(json.dumps(row), flush=True)
        sim.close()


if __name__ == "__main__":
    main()
