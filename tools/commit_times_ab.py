#!/usr/bin/env python3
"""Cost of commit-time recording on the device (EXPERIMENTS.md "Commit times"; raw outputs in profiles/commit_times/).  One JSON line per case.

    python tools/commit_times_ab.py --part ab          # twins against their base kernels, alternated in one process (hipEvent run times)
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/commit_times_ab.py --part histogram
                                                       # latency_histogram() calls, for a kernel trace of lbft_k_ct_latency_hist

--part ab: each base / twin pair runs on the same seeds, alternated `--reps` + 1 times (the first pair dropped); the base kernel is chosen with the
tuning variables LBFT_NO_QUAD / LBFT_NO_LEAN, which the library reads at every launch.  The layout flag word of each run is printed, so the kernel
that ran is on record (include/lbft.h lbft_batch_layout)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import librabft_simulator_amd as L  # noqa: E402
from librabft_simulator_amd import _lib, grid  # noqa: E402


def flags(sim):
    out = np.zeros(8, dtype=np.uint32)
    _lib.check(_lib.lib().lbft_batch_layout(sim._h, out.ctypes.data))
    return int(out[7])


def run_ms(sim, max_clock):
    if getattr(sim, "_ab_ran", False):
        sim.reset()
    sim._ab_ran = True
    sim.loop_until(max_clock, allow_faults=True)
    return sim.last_run_ms()[1]


def ab(name, base, twin, env_base, max_clock, reps):
    tb, tt = [], []
    for r in range(reps + 1):
        os.environ.update(env_base)
        b = run_ms(base, max_clock)
        fb = flags(base)
        for k in env_base:
            os.environ.pop(k, None)
        t = run_ms(twin, max_clock)
        ft = flags(twin)
        if r:
            tb.append(b)
            tt.append(t)
    print(json.dumps({"case": name, "base_flags": hex(fb), "twin_flags": hex(ft), "base_ms": tb, "twin_ms": tt, "base_median": float(np.median(tb)),
                      "twin_median": float(np.median(tt)), "ratio": float(np.median(tt) / np.median(tb))}), flush=True)


def grid16():
    sets = [L.ParamSet(L.RandomDelay.new(m, 4.0), L.NodeConfig(100000, d, 2.0, 0.5)) for m in (5.0, 10.0, 20.0, 40.0) for d in (10, 20, 40, 80)]
    set_of, si = grid.set_assignment(len(sets), 1024, "blocked")
    return sets, set_of, (1 + si).astype(np.uint64)


def grid64():
    sets = [L.ParamSet(L.RandomDelay.new(m, 4.0), L.NodeConfig(100000, d, 2.0, lam)) for m in (5.0, 10.0, 20.0, 40.0) for d in (10, 20, 40, 80)
            for lam in (0.25, 0.5, 0.75, 1.0)]
    set_of, si = grid.set_assignment(len(sets), 1024, "blocked")
    return sets, set_of, (1 + si).astype(np.uint64)


def part_ab(reps):
    d = L.RandomDelay.new(10.0, 4.0)
    seeds = np.arange(1, 65537, dtype=np.uint64)
    base, twin = L.BatchSimulator.new(seeds, 4, d), L.BatchSimulator.new(seeds, 4, d, commit_times=True)
    ab("small 65536x4 lognormal(10,4) clock 1000: lbft_k_ct_run0 vs lbft_k_run0", base, twin, {"LBFT_NO_QUAD": "1"}, 1000, reps)
    ab("small 65536x4 lognormal(10,4) clock 1000: lbft_k_ct_run0 vs headline lbft_k_run0q", base, twin, {}, 1000, reps)
    base.close()
    twin.close()
    seeds = np.arange(1, 4097, dtype=np.uint64)
    base = L.BatchSimulator.new(seeds, 32, d, drop_per_million=10000)
    twin = L.BatchSimulator.new(seeds, 32, d, drop_per_million=10000, commit_times=True)
    ab("mid 4096x32 drop 10000 clock 500: lbft_k_ct_run1 vs lbft_k_run<1>", base, twin, {"LBFT_NO_LEAN": "1"}, 500, reps)
    base.close()
    twin.close()
    for label, (sets, set_of, gseeds) in (("16-point grid", grid16()), ("64-point grid", grid64())):
        base = L.BatchSimulator.with_param_sets(gseeds, 4, sets, set_of)
        twin = L.BatchSimulator.with_param_sets(gseeds, 4, sets, set_of, commit_times=True)
        ab("%s x 1024 (blocked) clock 1000: lbft_k_ct_ps_run0 vs lbft_k_ps_run0" % label, base, twin, {}, 1000, reps)
        print(json.dumps({"case": label + " faulted instances", "n": int((L.BatchResult(twin).faults != 0).sum())}), flush=True)
        base.close()
        twin.close()


def part_histogram(calls):
    d = L.RandomDelay.new(10.0, 4.0)
    seeds = np.arange(1, 65537, dtype=np.uint64)
    cases = [("65536x4", L.BatchSimulator.new(seeds, 4, d, commit_times=True))]
    sets, set_of, gseeds = grid64()
    cases.append(("64-point grid x 1024", L.BatchSimulator.with_param_sets(gseeds, 4, sets, set_of, commit_times=True)))
    for name, sim in cases:
        res = sim.loop_until(1000, allow_faults=True)
        lanes = sim.num_instances * sim.num_nodes
        for width in (1, 7):
            ms = []
            for _ in range(calls + 1):
                t0 = time.perf_counter()
                hist, stats = res.latency_histogram(width)
                ms.append((time.perf_counter() - t0) * 1e3)
            samples = int(stats[:, 0].sum())
            # what the kernel loads: per lane its fault word and commit count, per sample a log word, the block's B_LINK and B_TIME words,
            # the author's startup word and the commit time (4 bytes each; L2 hits included)
            print(json.dumps({"case": "latency_histogram %s width %d" % (name, width), "call_ms": ms[1:], "samples": samples, "groups": int(hist.shape[0]),
                              "bins": int(hist.shape[1]), "bytes_loaded": lanes * 8 + samples * 20}), flush=True)
        sim.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--part", choices=("ab", "histogram"), required=True)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.part == "ab":
        part_ab(args.reps)
    else:
        part_histogram(args.reps)


if __name__ == "__main__":
    main()
