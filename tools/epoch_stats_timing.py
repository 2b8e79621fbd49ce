#!/usr/bin/env python3
"""Cost of the epoch statistics on the device, beside the vote and chain statistics in the same process -- kernels of the same shape
over the same chain and pool -- and beside the read-back they replace (EXPERIMENTS.md "Epoch statistics").  One JSON line per case.

    python tools/epoch_stats_timing.py                      # wall times, warm, in one process
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/epoch_stats_timing.py --calls 3 --cases headline,cpe5
                                                            # for a kernel trace of lbft_k_ps_epochs

Timed batches: the headline one (65 536 x 4 nodes, clock 1000: one segment per instance) and the same with an epoch every 5 commands
(quirks 3: five to six segments per instance); epoch_stats(), vote_stats() and chain_stats(), `--calls` warm calls each after one that
is dropped, and once the read-back: committed_histories + epochs (+ the block pools of `--pool-instances` instances through save_node,
scaled to the batch).  Figure batches (`figures`): 4 nodes, seeds 1..4, clock 1000 with an epoch every 30 000, 5 and 1 commands; rotating
rights [1, 2, 3, 4]; the stall after the first epoch change (quirks 0, an epoch every 50 commands, clock 2500); `large`: 64 x 100 nodes
with weighted rights and an epoch every 2 commands.  The identities of include/lbft.h are checked on what the device gave."""
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
    big, four = np.arange(1, 65537, dtype=np.uint64), np.arange(1, 5, dtype=np.uint64)
    if "headline" in which:
        yield "65536x4, clock 1000", L.BatchSimulator.new(big, 4, d), 1000, True
    if "cpe5" in which:
        yield "65536x4, epoch every 5, quirks 3, clock 1000", L.BatchSimulator.new(big, 4, d, commands_per_epoch=5, quirks=3), 1000, True
    if "figures" in which:
        for cpe in (30000, 5, 1):
            yield "4x4 seeds 1..4, epoch every %d, quirks 3, clock 1000" % cpe, L.BatchSimulator.new(four, 4, d, commands_per_epoch=cpe, quirks=3), 1000, False
        yield ("4x4 seeds 1..4, rights [1,2,3,4] rotating, epoch every 5, quirks 3, clock 1500",
               L.BatchSimulator.new(four, 4, d, commands_per_epoch=5, quirks=3, voting_rights=[1, 2, 3, 4], rights_rotation=1), 1500, False)
        yield "4x4 seeds 1..4, epoch every 50, quirks 0, clock 2500", L.BatchSimulator.new(four, 4, d, commands_per_epoch=50), 2500, False
    if "large" in which:
        rights = [1 + j % 4 for j in range(100)]
        yield ("64x100 weighted, epoch every 2, quirks 3, clock 300",
               L.BatchSimulator.new(np.arange(1, 65, dtype=np.uint64), 100, d, commands_per_epoch=2, quirks=3, voting_rights=rights), 300, False)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--cases", default="headline,cpe5,figures,large")
    ap.add_argument("--pool-instances", type=int, default=64, help="instances whose block pools are read back through save_node (scaled to the batch)")
    args = ap.parse_args()
    for name, sim, max_clock, time_it in cases(args.cases.split(",")):
        res = sim.loop_until(max_clock, allow_faults=True)
        layout = sim.layout()
        row = {"case": name, "kernel_class": layout["kernel_class"], "faulted": int((res.faults != 0).sum())}
        calls = args.calls if time_it else 1
        row["epoch_stats_ms"], (hist, table, stats) = timed(res.epoch_stats, calls)
        if time_it:
            row["vote_stats_ms"], _ = timed(res.vote_stats, calls)
            row["chain_stats_ms"], _ = timed(res.chain_stats, calls)
            for k in ("epoch", "vote", "chain"):
                row[k + "_stats_median_ms"] = float(np.median(row[k + "_stats_ms"]))
            row["epoch_over_vote"] = row["epoch_stats_median_ms"] / row["vote_stats_median_ms"]
            t0 = time.perf_counter()
            res.committed_histories()
            L.BatchResult(sim).epochs
            row["readback_histories_epochs_ms"] = (time.perf_counter() - t0) * 1e3
            k = min(args.pool_instances, sim.num_instances)
            t0 = time.perf_counter()
            try:
                for i in range(k):
                    for q in range(sim.num_nodes):
                        sim.save_node(i, q)
                row["readback_pools_ms_scaled"] = (time.perf_counter() - t0) * 1e3 * sim.num_instances / k
            except L.LbftError as e:  # (after an epoch change save_node needs a batch that keeps the retired record stores)
                row["readback_pools_ms_scaled"], row["readback_pools_refused"] = None, str(e)[:120]
        else:
            del row["epoch_stats_ms"]
        s, t = stats.astype(np.int64), table.astype(np.int64).sum(axis=1)
        clean = res.faults == 0
        row["identities"] = bool((hist.sum(axis=1) == s[:, 28]).all() and (t[:, 0] == s[:, 24]).all() and (t[:, 0] == s[:, 1]).all() and (t[:, 1] == s[:, 12]).all() and
                                 (t[:, 3] == s[:, 17]).all() and (t[:, 4] == s[:, 29]).all() and (t[:, 5] == s[:, 33]).all() and (t[:, 6] == s[:, 37]).all() and
                                 t[:, 2].sum() == int(res.commit_counts.max(axis=1)[clean].sum()) and
                                 s[:, 28].sum() == s[:, 24].sum() - int((res.commit_counts.max(axis=1)[clean] > 0).sum()))
        summary = res.epochs_by_param_set()[0]
        for key in ("segments", "length", "duration", "first_round", "last_round", "handover", "stranded", "behind", "blocks", "handover_cost",
                    "stranded_per_epoch", "behind_share"):
            row[key] = summary[key]
        row["per_epoch"] = summary["per_epoch"][:8]
        if sim.num_instances <= 4:
            row["node_epochs"] = res.epochs.tolist()
        print(json.dumps(row), flush=True)
        sim.close()


if __name__ == "__main__":
    main()
