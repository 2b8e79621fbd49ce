#!/usr/bin/env python3
"""Cost of the record hashes of a whole batch on the device (chain_heads(), chain_record_hashes()) against the two ways there were to
the same data: the per-node call (committed_record_hashes, one launch per (instance, node)) over 256 strided nodes, extrapolated to
every node of the batch, and the read-back of every history (committed_histories()), which is what the State hashes cover
(EXPERIMENTS.md "Record hashes of whole batches"; raw outputs in profiles/record_hashes/).  One JSON line per case.

    python tools/record_hashes_timing.py                    # wall times, warm, in one process
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/record_hashes_timing.py --calls 3 --no-baselines
                                                            # for a kernel trace of lbft_k_rh_chain

Per batch -- the headline one (65 536 x 4 nodes, clock 1000) and the large one (8 192 x 100 nodes, clock 300).  The first call of each
timed loop is dropped.  The strided per-node answers are compared with the bulk call's."""
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
        yield "65536x4, clock 1000", L.BatchSimulator.new(np.arange(1, 65537, dtype=np.uint64), 4, d), 1000
    if "large" in which:
        yield "8192x100, clock 300", L.BatchSimulator.new(np.arange(1, 8193, dtype=np.uint64), 100, d), 300
    if "small" in which:  # (a quick check of the tool itself)
        yield "1024x4, clock 1000", L.BatchSimulator.new(np.arange(1, 1025, dtype=np.uint64), 4, d), 1000


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--cases", default="headline,large")
    ap.add_argument("--no-baselines", action="store_true", help="skip the per-node calls and the read-back of the histories")
    args = ap.parse_args()
    for name, sim, max_clock in cases(args.cases.split(",")):
        res = sim.loop_until(max_clock, allow_faults=True)
        layout = sim.layout()
        m, n = sim.num_instances, sim.num_nodes
        counts = res.commit_counts
        row = {"case": name, "kernel_class": layout["kernel_class"], "faulted": int((res.faults != 0).sum()),
               "longest_chain": int(counts.max()), "mean_chain": float(counts.max(axis=1).mean())}
        row["chain_heads_ms"], heads = timed(res.chain_heads, args.calls)
        row["chain_heads_median_ms"] = float(np.median(row["chain_heads_ms"]))
        row["chain_record_hashes_ms"], (entries, heads2, prefix) = timed(res.chain_record_hashes, args.calls)
        row["chain_record_hashes_median_ms"] = float(np.median(row["chain_record_hashes_ms"]))
        row["entries_bytes"] = int(entries.nbytes)
        row["heads_agree"] = bool((heads == heads2).all())
        row["qc_hash_xor"] = int(np.bitwise_xor.reduce(heads["qc_hash"]))  # (one word that changes with any entry of any chain)
        row["histories_are_prefixes"] = bool((prefix == np.minimum(counts, heads["length"][:, None]))[res.faults == 0].all())
        if not args.no_baselines:
            picks = np.linspace(0, m * n - 1, 256).astype(np.int64)  # 256 strided (instance, node) pairs

            def per_node():
                return [res.committed_record_hashes(int(p // n), int(p % n)) for p in picks]
            row["per_node_256_ms"], got = timed(per_node, 2)
            row["per_node_extrapolated_ms"] = float(np.median(row["per_node_256_ms"])) / len(picks) * m * n
            row["per_node_equal"] = bool(all(entries[int(p // n), :len(g)].tobytes() == g.tobytes() for p, g in zip(picks, got)))

            def readback():
                return L.BatchResult(sim).committed_histories()  # (nothing cached)
            row["histories_readback_ms"], histories = timed(readback, 3)
            row["histories_readback_median_ms"] = float(np.median(row["histories_readback_ms"]))
            row["histories_bytes"] = int(histories.nbytes)
            row["readback_over_chain_heads"] = row["histories_readback_median_ms"] / row["chain_heads_median_ms"]
            row["per_node_over_chain_record_hashes"] = row["per_node_extrapolated_ms"] / row["chain_record_hashes_median_ms"]
        print(json.dumps(row), flush=True)
        sim.close()


if __name__ == "__main__":
    main()
