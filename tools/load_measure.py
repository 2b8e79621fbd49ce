"""The measurements of EXPERIMENTS.md "Run load" (needs the GPU): `calls` times load_stats / instance_load against the read-back of commit
counts, active rounds and fault words reduced in numpy, on the 65 536 x 4 batch and on c4 of tools/configs.py; `grid` runs the README's 64-point
grid with --load (every line goes to profiles/run_load/grid_load.jsonl) and prints its extreme points; `sizing` runs DESIGN.md section 4's
sizing-gap case on the calendar at growing queue capacities and on the heap.
    python tools/load_measure.py calls|grid|sizing"""
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import librabft_simulator_amd as amd  # noqa: E402
from librabft_simulator_amd.simulator import BatchResult  # noqa: E402


def timed(fn, reps=7):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def calls():
    import configs
    c4 = configs.CONFIGS["c4_16384x64_longtail_equivocators"]
    for name, m, n, clock, delay, kw in (("65536x4", 65536, 4, 1000, amd.RandomDelay.new(10.0, 4.0), {}),
                                         ("c4_16384x64", c4["instances"], c4["nodes"], c4["max_clock"], amd.RandomDelay.new(10.0, c4["variance"]),
                                          dict(equivocate_every=c4["equivocate_every"]))):
        sim = amd.BatchSimulator.new(np.arange(1, m + 1, dtype=np.uint64), n, delay, **kw)
        res = sim.loop_until(clock, allow_faults=True)
        rows = res.instance_load()
        bins = int(rows[:, 9].max()) + 1

        def parent():
            r = BatchResult(sim)
            cc, ar, f = r.commit_counts, r.active_rounds, r.faults
            clean = f == 0
            return cc.max(axis=1)[clean].sum(), cc.min(axis=1)[clean].sum(), ar.min(axis=1)[clean].sum(), np.bincount(f & 1)

        def parent_readback_only():
            r = BatchResult(sim)
            return r.commit_counts, r.active_rounds, r.faults

        out = {"batch": name, "kernel": configs.kernel_name(sim.layout()), "run_ms": sim.last_run_ms()[1], "faulted": int(np.count_nonzero(res.faults)),
               "load_stats": timed(lambda: BatchResult(sim).load_stats("queue", 1, bins)), "bins": bins,
               "load_stats_1bin": timed(lambda: BatchResult(sim).load_stats("queue", 1, 1)),
               "instance_load": timed(lambda: BatchResult(sim).instance_load()),
               "parent_readback_numpy": timed(parent), "parent_readback_only": timed(parent_readback_only)}
        print(json.dumps(out), flush=True)
        sim.close()


def grid():
    from librabft_simulator_amd import grid as G
    buf = io.StringIO()
    t = time.perf_counter()
    with redirect_stdout(buf):
        G.main(["--mean", "5,10,20,40", "--delta", "10,20,40,80", "--lambda", "0.25,0.5,0.75,1.0", "--seeds-per-point", "1024", "--load"])
    wall = time.perf_counter() - t
    lines = [json.loads(s) for s in buf.getvalue().splitlines()]
    open(os.path.join(ROOT, "profiles", "run_load", "grid_load.jsonl"), "w").write(buf.getvalue())
    print("points", len(lines), "wall_s", round(wall, 2))
    key = lambda d: d["load"]["messages_per_commit"] or 0  # noqa: E731
    for what, d in (("min messages/commit", min(lines, key=key)), ("max messages/commit", max(lines, key=key)),
                    ("max queue headroom", max(lines, key=lambda d: d["load"]["headroom"]["queue"])),
                    ("min queue headroom", min(lines, key=lambda d: d["load"]["headroom"]["queue"]))):
        ld = d["load"]
        print(what, json.dumps({"mean": d["mean"], "delta": d["delta"], "lambda": d["lambda"], "messages_per_commit": ld["messages_per_commit"],
                                "notifications_per_commit": ld["notifications_per_commit"], "requests_per_commit": ld["requests_per_commit"],
                                "responses_per_commit": ld["responses_per_commit"], "commits": ld["commits"], "queue": ld["queue"],
                                "headroom": ld["headroom"], "queue_quantiles": ld["queue_quantiles"], "faults": ld["faults"], "worst_seed": ld["worst_seed"]}))


def sizing():
    seeds = np.arange(1, 33, dtype=np.uint64)
    delay = amd.RandomDelay.uniform(20, 120)
    for calendar in (True, False):
        for qcap in ((0, 4800, 6400, 9600, 12800, 19200) if calendar else (0,)):
            sim = amd.BatchSimulator.new(seeds, 20, delay, queue_capacity=qcap, calendar_queue=calendar)
            res = sim.loop_until(3000, allow_faults=True)
            row = res.load_by_param_set()[0]
            caps = res.load_stats("chunks")[3]
            rows = res.instance_load()
            print(json.dumps({"calendar": calendar, "queue_capacity": qcap, "caps": caps.tolist(), "run_ms": sim.last_run_ms()[1], "clean": row["clean"],
                              "instances": row["instances"], "faults": row["faults"], "headroom": row["headroom"], "queue": row["queue"], "chunks": row["chunks"],
                              "chunks_all_max": int(rows[:, 10].max()), "queue_all_max": int(rows[:, 9].max()), "worst_seed": row["worst_seed"]}), flush=True)
            sim.close()


if __name__ == "__main__":
    {"calls": calls, "grid": grid, "sizing": sizing}[sys.argv[1]]()
