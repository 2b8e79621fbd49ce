"""Grid of parameter sets in one batch: ``python -m librabft_simulator_amd.grid``.

Comma lists for the reference's study variables (librabft-v2/src/main.rs:73-140) -- ``--mean``, ``--variance``, ``--delta``, ``--gamma``,
``--lambda``, ``--target-commit-interval`` -- and ``--drop-per-million``; their cross product is the grid, at most 256 points.  Every point
runs ``--seeds-per-point`` networks of ``--nodes`` nodes to ``--max-clock``, all points in ONE batch (BatchSimulator.with_param_sets).
``--assign blocked`` gives point k the instances [k * seeds, (k + 1) * seeds); ``interleaved`` gives it instances k, k + points, ...
Seeds are first-seed .. first-seed + seeds-per-point - 1 for every point.  Prints one JSON line per grid point; with ``--latency`` the
batch records commit times and each line gains a ``"latency"`` object (BatchResult.latency_by_param_set: samples, mean, min, max and
the 0.5 / 0.9 / 0.99 quantiles of the commit latency over every node's commits of the point's instances).
``--partition SIZE:START:END[,SIZE:START:END...]`` is one more grid axis (nodes [0, SIZE) are cut off during [START, END); ``none`` is a
value too); the lines then carry a ``"partition"`` key.  ``--stalls`` records commit times and adds a ``"stalls"`` object
(BatchResult.stalls_by_param_set with ``since="partition_end"``: gaps between a node's commits, time from the partition's end to the next
commit, time since the last commit, longest commit-free interval); ``--series WIDTH`` adds ``"series"``, the point's commits per WIDTH
ticks (BatchResult.commit_series).
``--rounds`` records the round-switch trace (``--round-trace N`` rounds per node, by default max_clock / 5 + 64, at most 65 536; an
instance that passes it counts as faulted and gives no sample) and adds a ``"round_stats"`` object (BatchResult.rounds_by_param_set: how
long nodes stay in a round, how many rounds they jump, how far apart the nodes of a network enter a round and how many of them enter it);
``"rounds"``, the final active round's mean / min / max, stays as it is.
``--finality`` records commit times and adds a ``"finality"`` object (BatchResult.finality_by_param_set: how long after its proposal an
entry is committed by the first node, by a quorum of the voting rights and by every node, the spread between the first and the last
commit, which node commits first and how many entries no quorum had committed at the end).
``--chain`` adds a ``"chain"`` object (BatchResult.chain_by_param_set: the intervals between the proposals of consecutive blocks of the
committed chain, its length, the nodes' lag behind it, the leaders' tenure, the blocks per proposer and whether every node's history is
a prefix of the chain); it needs neither commit times nor the trace and leaves the batch on the kernel it would run anyway.
``--spread`` records commit times and adds a ``"spread"`` object (BatchResult.seed_spread with ``since="partition_end"``: per metric --
commits, latency, longest stall, recovery, quorum finality, spread, open entries -- the mean over the point's seeds with its standard
deviation and standard error, and the extremes with the seeds that attain them: the error bar of a point, and the seed to replay).
``--phases E1,E2,...|partition`` records commit times and adds a ``"phases"`` list (BatchResult.phases_by_param_set: the commit latency
and the finality of the entries PROPOSED in each window of the clock -- up to 7 edges in [0, max_clock + 1], not decreasing, or
``partition`` for before / during / after each point's own partition; per phase ``from``, ``to``, the six families and the quantiles
of the latency and of the quorum finality).  ``--phases WARM,END`` sets a warm-up and a cool-down apart.
``--load`` adds a ``"load"`` object (BatchResult.load_by_param_set: events by kind, messages per commit, the high-water marks of the
event queue, the calendar's chunk pool and the snapshot pool against their capacities, the fault census and the seeds that came closest
to a capacity); like ``--chain`` it needs neither commit times nor the trace and leaves the batch on the kernel it would run anyway.
``--votes`` adds a ``"votes"`` object (BatchResult.votes_by_param_set: the votes, weight and margin of the chain's quorum certificates,
the rounds the chain skipped, the blocks proposed, orphaned and pending, each node's participation, the orphan rate and the round
utilisation); it too needs neither commit times nor the trace.
``--epochs`` adds an ``"epochs"`` object (BatchResult.epochs_by_param_set: the chain's segments of one epoch -- length, duration, first
and last round --, the handover between two epochs and its cost against the interval inside an epoch, the blocks stranded in an epoch
the chain has left, how far the nodes' epochs lie behind the foremost, and the same per epoch); it goes with a small
``--commands-per-epoch`` and needs neither commit times nor the trace.
"""
import argparse
import itertools
import json
import sys

import numpy as np

from ._lib import MAX_PARAM_SETS
from .simulator import BatchSimulator, NodeConfig, ParamSet, RandomDelay


def _floats(text):
    return [float(v) for v in text.split(",") if v.strip()]


def _ints(text):
    return [int(v) for v in text.split(",") if v.strip()]


def _partitions(text):
    """``SIZE:START:END`` items or ``none``, comma separated: a list of (size, start, end) tuples and None."""
    out = []
    for item in text.split(","):
        item = item.strip()
        if not item:
            continue
        if item.lower() == "none":
            out.append(None)
            continue
        parts = item.split(":")
        if len(parts) != 3:
            raise argparse.ArgumentTypeError("a partition is SIZE:START:END or none, not %r" % item)
        try:
            out.append(tuple(int(v) for v in parts))
        except ValueError:
            raise argparse.ArgumentTypeError("a partition is SIZE:START:END or none, not %r" % item)
    if not out:
        raise argparse.ArgumentTypeError("--partition needs at least one value")
    return out


def _phases(text):
    """``partition`` or up to 7 comma-separated, non-negative, non-decreasing ints."""
    if text.strip().lower() == "partition":
        return "partition"
    try:
        edges = [int(v) for v in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("--phases takes E1,E2,... or partition, not %r" % text)
    if not 1 <= len(edges) <= 7 or min(edges) < 0 or any(b < a for a, b in zip(edges, edges[1:])):
        raise argparse.ArgumentTypeError("--phases takes 1 to 7 edges, none negative, none below its predecessor, not %r" % text)
    return edges


def grid_points(args):
    """The grid's points in output order (the last option varies fastest).  The partition is an axis, and a key, only when given."""
    keys = ("mean", "variance", "delta", "gamma", "lambda", "target_commit_interval", "drop_per_million")
    values = (args.mean, args.variance, args.delta, args.gamma, args.lambda_, args.target_commit_interval, args.drop_per_million)
    if getattr(args, "partition", None) is not None:
        keys, values = keys + ("partition",), values + (args.partition,)
    return [dict(zip(keys, combo)) for combo in itertools.product(*values)]


def set_assignment(points, seeds_per_point, assign):
    """set_of_instance for `points` points of `seeds_per_point` instances each, and the seed index of every instance."""
    k = np.arange(points * seeds_per_point)
    if assign == "blocked":
        return (k // seeds_per_point).astype(np.uint32), k % seeds_per_point
    return (k % points).astype(np.uint32), k // points


def round_trace_capacity(max_clock, explicit):
    """Rounds per node the trace of ``--rounds`` keeps: ``--round-trace``, else BatchSimulator.loop_until's own first guess."""
    return int(explicit) if explicit is not None else min(int(max_clock) // 5 + 64, 1 << 16)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m librabft_simulator_amd.grid", description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, default=4)
    ap.add_argument("--mean", type=_floats, default=[10.0])
    ap.add_argument("--variance", type=_floats, default=[4.0])
    ap.add_argument("--delta", type=_ints, default=[20])
    ap.add_argument("--gamma", type=_floats, default=[2.0])
    ap.add_argument("--lambda", dest="lambda_", type=_floats, default=[0.5])
    ap.add_argument("--target-commit-interval", type=_ints, default=[100000])
    ap.add_argument("--drop-per-million", type=_ints, default=[0])
    ap.add_argument("--commands-per-epoch", type=int, default=30000)
    ap.add_argument("--seeds-per-point", type=int, default=64)
    ap.add_argument("--first-seed", type=int, default=1)
    ap.add_argument("--max-clock", type=int, default=1000)
    ap.add_argument("--assign", choices=("blocked", "interleaved"), default="blocked")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--latency", action="store_true", help="record commit times and add each point's commit-latency summary")
    ap.add_argument("--partition", type=_partitions, default=None, help="grid axis: SIZE:START:END[,...], 'none' allowed as a value")
    ap.add_argument("--stalls", action="store_true", help="record commit times and add each point's stall / recovery summary")
    ap.add_argument("--series", type=int, default=None, metavar="WIDTH", help="record commit times and add each point's commits per WIDTH ticks")
    ap.add_argument("--finality", action="store_true", help="record commit times and add each point's commit-finality summary")
    ap.add_argument("--spread", action="store_true", help="record commit times and add each point's spread across its seeds (error bars, worst seeds)")
    ap.add_argument("--phases", type=_phases, default=None, metavar="E1,E2,...|partition",
                    help="record commit times and add each point's latency and finality per proposal-time window")
    ap.add_argument("--rounds", action="store_true", help="record the round-switch trace and add each point's round statistics")
    ap.add_argument("--chain", action="store_true", help="add each point's chain statistics (agreement, chain quality, block cadence)")
    ap.add_argument("--load", action="store_true", help="add each point's run load (message counts per commit, capacity headroom, worst seeds)")
    ap.add_argument("--votes", action="store_true", help="add each point's vote statistics (QC sizes and margins, participation, orphaned blocks)")
    ap.add_argument("--epochs", action="store_true", help="add each point's epoch statistics (handover cost, stranded blocks, nodes left behind)")
    ap.add_argument("--round-trace", type=int, default=None, metavar="N", help="with --rounds: rounds per node the trace keeps")
    args = ap.parse_args(argv)
    if args.round_trace is not None and (args.round_trace < 1 or not args.rounds):
        ap.error("--round-trace N goes with --rounds and must be at least 1")
    if args.series is not None and args.series < 1:
        ap.error("--series WIDTH must be at least 1")
    if args.phases is not None and args.phases != "partition" and args.phases[-1] > args.max_clock + 1:
        ap.error("--phases: an edge lies in [0, max_clock + 1]")
    points = grid_points(args)
    if not 1 <= len(points) <= MAX_PARAM_SETS:
        ap.error("the grid has %d points; 1 to %d fit one batch" % (len(points), MAX_PARAM_SETS))
    if args.seeds_per_point < 1:
        ap.error("--seeds-per-point must be at least 1")
    sets = [ParamSet(RandomDelay.new(pt["mean"], pt["variance"]),
                     NodeConfig(target_commit_interval=pt["target_commit_interval"], delta=pt["delta"], gamma=pt["gamma"], lambda_=pt["lambda"]),
                     drop_per_million=pt["drop_per_million"], partition=pt.get("partition")) for pt in points]
    set_of, seed_index = set_assignment(len(points), args.seeds_per_point, args.assign)
    seeds = (args.first_seed + seed_index).astype(np.uint64)
    kw = {"commit_times": True} if args.latency or args.stalls or args.finality or args.spread or args.phases is not None or args.series is not None else {}
    sim = BatchSimulator.with_param_sets(seeds, args.nodes, sets, set_of, commands_per_epoch=args.commands_per_epoch, device=args.device, **kw)
    try:
        res = sim.loop_until(args.max_clock, allow_faults=True, round_trace=round_trace_capacity(args.max_clock, args.round_trace) if args.rounds else None)
        latency = res.latency_by_param_set() if args.latency else None
        stalls = res.stalls_by_param_set(since="partition_end") if args.stalls else None
        series = res.commit_series(bin_width=args.series) if args.series is not None else None
        finality = res.finality_by_param_set() if args.finality else None
        spread = res.seed_spread(since="partition_end") if args.spread else None
        phases = res.phases_by_param_set(args.phases) if args.phases is not None else None
        round_stats = res.rounds_by_param_set() if args.rounds else None
        chain = res.chain_by_param_set() if args.chain else None
        load = res.load_by_param_set() if args.load else None
        votes = res.votes_by_param_set() if args.votes else None
        epochs = res.epochs_by_param_set() if args.epochs else None
        for k, (pt, row) in enumerate(zip(points, res.by_param_set())):
            line = dict(pt, nodes=args.nodes, max_clock=args.max_clock, seeds=args.seeds_per_point, assign=args.assign)
            line.update(instances=row["instances"], faulted=row["faulted"], commits=row["commits"], rounds=row["rounds"])
            if latency is not None:
                line["latency"] = latency[k]
            if stalls is not None:
                line["stalls"] = stalls[k]
            if series is not None:
                line["series"] = [int(v) for v in series[k]]
            if finality is not None:
                line["finality"] = finality[k]
            if spread is not None:
                line["spread"] = spread[k]
            if phases is not None:
                line["phases"] = phases[k]["phases"]
            if round_stats is not None:
                line["round_stats"] = round_stats[k]
            if chain is not None:
                line["chain"] = chain[k]
            if load is not None:
                line["load"] = load[k]
            if votes is not None:
                line["votes"] = votes[k]
            if epochs is not None:
                line["epochs"] = epochs[k]
            print(json.dumps(line), flush=True)
    finally:
        sim.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
