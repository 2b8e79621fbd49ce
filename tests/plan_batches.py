"""The batches whose geometry tests/golden/plan_layouts.json records: what the device library reported for each after a run (the eight
words of lbft_batch_layout, lbft_batch_device_bytes) and the free device memory just before it, recorded on the MI355X before the planner
moved into csrc/lbft_plan.h.  tests/test_plan.py asks the planner (oracle_ctypes.plan) for every entry, tests/test_edge_cases_gpu.py the
device library.

The table: BASELINE's configurations 2-5 of tools/configs.py (c2 in both delay models, c3, its 8 192-network shard, c4, c5, c4live,
c5live), 256 x 4, a forced lanes_per_wavefront, a lossy 32-node batch, a parameter-set, a commit-time and a commit-time parameter-set
batch of each class, and every accepted case of edge_cases.CASES that the device tier runs.  An entry is in the fixture only if free
memory was at least twice the batch's state / 0.85: then the calendar fallback cannot have been decided by the card's other users."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import edge_cases as ec  # noqa: E402
from configs import CONFIGS  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_layouts.json")
BASELINE = ("c2_1024x4_lognormal", "c2_1024x4_uniform", "c3_65536x4", "c3shard_8192x4", "c4_16384x64_longtail_equivocators",
            "c5_8192x100_weighted_epochs", "c4live_16384x64_longtail_equivocators_fixed", "c5live_8192x100_rotating_rights_epochs_fixed")


def _plain(n, m, max_clock, cfg=None, **kw):
    """A plain batch: `cfg` holds the configuration fields in edge_cases' spelling, `kw` the batch's own settings."""
    return dict(dict(n=n, m=m, max_clock=max_clock, cfg=dict(cfg or {}), weights=None, equivocate_every=0, rights_rotation=0, lpw=0,
                     commit_times=False, calendar_queue=True, block_capacity=0), **kw)


def _baseline(name):
    c = CONFIGS[name]
    cfg = dict(variance=c.get("variance", 4.0), quirks=c.get("quirks", 0), commands_per_epoch=c.get("commands_per_epoch", 30000))
    if "uniform" in c:
        cfg.update(delay_model=1, uniform_lo=c["uniform"][0], uniform_hi=c["uniform"][1])
    return _plain(c["nodes"], c["instances"], c["max_clock"], cfg, weights=c.get("weights"), equivocate_every=c.get("equivocate_every", 0),
                  rights_rotation=c.get("rights_rotation", 0))


def edge_batch(case, **kw):
    return _plain(case["n"], len(case["seeds"]), case["max_clock"], case["cfg"], seeds=case["seeds"],
                  calendar_queue=case.get("calendar_queue", True), block_capacity=case.get("block_capacity", 0), **kw)


BATCHES = {name: _baseline(name) for name in BASELINE}
BATCHES["256x4"] = _plain(4, 256, 1000)
BATCHES["forced_lpw_4096x4_at_64"] = _plain(4, 4096, 1000, lpw=64)
BATCHES["forced_lpw_8192x7_at_4"] = _plain(7, 8192, 300, ec.LOSSY, lpw=4)
BATCHES["lossy_32_nodes"] = _plain(32, 64, 300, dict(drop_per_million=20000))
BATCHES["commit_times_class0"] = _plain(4, 96, 1000, commit_times=True)
BATCHES["commit_times_class1"] = _plain(7, 96, 1000, ec.LOSSY, commit_times=True)
for _c in ec.PARAM_SET_CASES[:2]:
    BATCHES["param_" + _c["name"]] = dict(sets=_c["name"], commit_times=False)
    BATCHES["commit_times_param_" + _c["name"]] = dict(sets=_c["name"], commit_times=True)
for _c in ec.CASES:
    if ec.expected(_c)[0] != "refused" and not _c.get("host_only"):
        BATCHES["edge_" + _c["name"]] = edge_batch(_c)


def _sets_case(spec):
    return next(c for c in ec.PARAM_SET_CASES if c["name"] == spec["sets"])


def make_sim(m, spec):
    """The batch on the device (``m``: the librabft_simulator_amd package), not run yet."""
    if "sets" in spec:
        case = _sets_case(spec)
        sets = []
        for k in range(len(case["sets"])):
            f = ec.set_fields(case, k)
            delay = m.RandomDelay.uniform(f["uniform_lo"], f["uniform_hi"]) if case["delay_model"] == 1 else m.RandomDelay.new(f["mean"], f["variance"])
            sets.append(m.ParamSet(delay, m.NodeConfig(f["target_commit_interval"], f["delta"], f["gamma"], f["lambda_"]),
                                   drop_per_million=f["drop_per_million"]))
        set_of, seeds = ec.set_layout(case)
        return m.BatchSimulator.with_param_sets(np.array(seeds, dtype=np.uint64), case["n"], sets, np.array(set_of, dtype=np.uint32),
                                                commit_times=spec["commit_times"])
    f = dict(mean=10.0, variance=4.0, delay_model=0, uniform_lo=5, uniform_hi=15, target_commit_interval=100000, delta=20, gamma=2.0,
             lambda_=0.5, quirks=0, drop_per_million=0, commands_per_epoch=30000)
    f.update(spec["cfg"])
    delay = m.RandomDelay.uniform(f["uniform_lo"], f["uniform_hi"]) if f["delay_model"] == 1 else m.RandomDelay.new(f["mean"], f["variance"])
    seeds = np.array(spec.get("seeds") or range(1, spec["m"] + 1), dtype=np.uint64)
    return m.BatchSimulator.new(seeds, spec["n"], delay, m.NodeConfig(f["target_commit_interval"], f["delta"], f["gamma"], f["lambda_"]),
                                commands_per_epoch=f["commands_per_epoch"], voting_rights=spec["weights"], quirks=f["quirks"],
                                drop_per_million=f["drop_per_million"], equivocate_every=spec["equivocate_every"],
                                rights_rotation=spec["rights_rotation"], lanes_per_wavefront=spec["lpw"], commit_times=spec["commit_times"],
                                calendar_queue=spec["calendar_queue"], block_capacity=spec["block_capacity"])


def max_clock_of(spec):
    return _sets_case(spec)["max_clock"] if "sets" in spec else spec["max_clock"]


def planned(oc, spec, avail_bytes):
    """What the planner (``oc``: oracle_ctypes) chooses for the batch with ``avail_bytes`` of device memory free."""
    if "sets" in spec:
        case = _sets_case(spec)
        f = ec.set_fields(case, 0)  # the batch-wide configuration: set 0's fields and the loss of any set (config_of_sets)
        cfg = oc.make_config(num_nodes=case["n"], delay_model=case["delay_model"], **f)
        return oc.plan(cfg, len(case["sets"]) * case["per"], case["max_clock"], param_sets=len(case["sets"]), commit_times=spec["commit_times"],
                       avail_bytes=avail_bytes)
    cfg = oc.make_config(num_nodes=spec["n"], voting_rights=spec["weights"], equivocate_every=spec["equivocate_every"],
                         rights_rotation=spec["rights_rotation"], **spec["cfg"])
    return oc.plan(cfg, spec["m"], spec["max_clock"], block_capacity=spec["block_capacity"], lanes_per_wavefront=spec["lpw"],
                   commit_times=spec["commit_times"], calendar_queue=spec["calendar_queue"], avail_bytes=avail_bytes)


def recorded():
    """The fixture's entries: [{"name", "layout": the eight words, "device_bytes", "free_bytes"}]."""
    with open(FIXTURE) as f:
        return json.load(f)["entries"]


def dropped():
    """Names of the table's batches that were run but not kept: free memory was below twice their state / 0.85."""
    with open(FIXTURE) as f:
        return json.load(f)["dropped"]
