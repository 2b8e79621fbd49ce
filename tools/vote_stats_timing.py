#!/usr/bin/env python3
"""Cost of the vote statistics on the device, beside the chain statistics in the same process: a kernel of the same shape over the same
chain plus a pass over the block pool (EXPERIMENTS.md "Vote statistics"; raw outputs in profiles/vote_stats/).  One JSON line per case.

    python tools/vote_stats_timing.py                       # wall times, warm, in one process
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/vote_stats_timing.py --calls 3 --cases headline
                                                            # for a kernel trace of lbft_k_ps_votes

Per batch -- the headline one (65 536 x 4 nodes, clock 1000), a weighted one (16 384 x 5 nodes, rights [5, 1, 1, 1, 1], clock 1000), the
large one (8 192 x 100 nodes, clock 300) and a grid of 64 parameter sets of 1 024 four-node networks each (clock 1000) --: vote_stats()
and chain_stats(), `--calls` warm calls each after one that is dropped, and the figures votes_by_param_set() reports (pooled over the
groups).  The identities of include/lbft.h are checked on what the device gave."""
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
    if "weighted" in which:
        yield "16384x5 rights [5,1,1,1,1], clock 1000", L.BatchSimulator.new(np.arange(1, 16385, dtype=np.uint64), 5, d, voting_rights=[5, 1, 1, 1, 1]), 1000
    if "large" in which:
        yield "8192x100, clock 300", L.BatchSimulator.new(np.arange(1, 8193, dtype=np.uint64), 100, d), 300
    if "grid" in which:
        sets = [L.ParamSet(L.RandomDelay.new(mean, 4.0), L.NodeConfig(100000, delta, 2.0, lam))
                for mean in (8.0, 10.0, 12.0, 14.0) for delta in (10, 15, 20, 30) for lam in (0.25, 0.5, 0.75, 1.0)]
        k = np.arange(64 * 1024)
        yield "64 sets x 1024 x 4, clock 1000", L.BatchSimulator.with_param_sets((1 + k // 64).astype(np.uint64), 4, sets, (k % 64).astype(np.uint32)), 1000


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--cases", default="headline,weighted,large,grid")
    args = ap.parse_args()
    for name, sim, max_clock in cases(args.cases.split(",")):
        res = sim.loop_until(max_clock, allow_faults=True)
        layout = sim.layout()
        groups = len(sim.param_sets) if sim.param_sets is not None else 1
        row = {"case": name, "kernel_class": layout["kernel_class"], "lanes_per_wavefront": layout["lanes_per_wavefront"],
               "faulted": int((res.faults != 0).sum()), "groups": groups}
        row["vote_stats_ms"], (margin, votes, nodes, stats) = timed(res.vote_stats, args.calls)
        row["chain_stats_ms"], (_, authors, chain) = timed(res.chain_stats, args.calls)
        row["vote_stats_median_ms"] = float(np.median(row["vote_stats_ms"]))
        row["chain_stats_median_ms"] = float(np.median(row["chain_stats_ms"]))
        row["vote_over_chain"] = row["vote_stats_median_ms"] / row["chain_stats_median_ms"]
        s = stats.astype(np.int64)
        row["samples"] = [int(v) for v in s[:, 0::4].sum(axis=0)]
        row["sums"] = [int(v) for v in s[:, 1::4].sum(axis=0)]
        row["max"] = [int(v) for v in s[:, 3::4].max(axis=0)]
        row["votes_hist"] = [int(v) for v in votes.sum(axis=0)]
        row["margin_hist_head"] = [int(v) for v in margin.sum(axis=0)[:8]]
        row["node_table"] = nodes.sum(axis=0).astype(np.int64).tolist()
        lengths = chain.astype(np.int64)[:, 4 * 1 + 1]  # chain_stats' family `length`, its sum: the chain entries of the group
        row["identities"] = bool((s[:, 17] == lengths + s[:, 21] + s[:, 25]).all() and (nodes[:, :, 0].sum(axis=1) == s[:, 17]).all() and
                                 (nodes[:, :, 1].sum(axis=1) == s[:, 21]).all() and (nodes[:, :, 2].sum(axis=1) == s[:, 1]).all() and
                                 (margin.sum(axis=1) == s[:, 8]).all() and (votes.sum(axis=1) == s[:, 0]).all() and (s[:, 0] <= lengths).all())
        row["chain_entries"], row["entries_with_a_certificate"] = int(lengths.sum()), int(s[:, 0].sum())
        decided = int(s[:, 17].sum() - s[:, 25].sum())
        row["orphan_rate"] = int(s[:, 21].sum()) / decided if decided else None
        pairs, skipped = int(s[:, 12].sum()), int(s[:, 13].sum())
        row["round_utilisation"] = pairs / (pairs + skipped) if pairs + skipped else None
        qcs = int(s[:, 0].sum())
        row["participation"] = [int(v) / qcs for v in nodes[:, :, 2].sum(axis=0)] if qcs and nodes.shape[1] <= 8 else None
        print(json.dumps(row), flush=True)
        sim.close()


if __name__ == "__main__":
    main()
