"""Edge cases of the network shape and fault-injection parameters of lbft_config -- num_nodes, voting_rights, rights_rotation,
commands_per_epoch, equivocate_every, drop_per_million, partition_size / _start / _end, the seeds: one table in the spelling of
tests/edge_cases.py, run by the CPU tier (tests/test_network_edges_host.py: the host build of the kernel logic and the fenced stand-alone
program against the oracle) and the device tier (tests/test_network_edges_gpu.py).

These fields are extensions whose only specification is the oracle, and they are where the kernels narrow types or branch: the partition
window is clamped to i32 (the oracle compares i64), a voting right has 24 bits and the vote sums 32, rights_rotation is taken modulo the
network size, node % equivocate_every picks the equivocators, and the loss draw is compiled out of class 0 and the lean kernels.  Every
case states its outcome as edge_cases does ("equal" | "fault:<bits>"); the refused configurations are in REFUSED and REFUSED_PARAM_SETS.
Optional fields: block_capacity; timed_max_clock; weighted (the device statistics that weigh commits run on it); kernel_class / calendar / lean / exchange pin the run kernel's family (lbft_batch_layout's flag word),
so that a case cannot silently move to another one.

This table is NOT part of edge_cases.CASES: tests/plan_batches.py turns every entry of that list into a batch of the recorded fixture
tests/golden/plan_layouts.json.
"""
from edge_cases import COMPARED, COMPARED_COUNTERS, HISTORY_CAP, LAYOUT_CALENDAR, expected, host_caps, oracle_config  # noqa: F401

F_BLOCK_OVERFLOW = 1 << 2
LBFT_ERR_INVALID, LBFT_ERR_UNSUPPORTED = -1, -3
LAYOUT_LEAN, LAYOUT_EXCHANGE = 1 << 10, 1 << 12  # lbft_batch_layout out[7]: LF_LEAN, LF_EXCHANGE (csrc/lbft_plan.h)

W = 0xffffff      # the largest voting right
U32 = 2 ** 32 - 1
# Heavy loss on 40 nodes.  Of 300 000 / 500 000 / 700 000 none is live in the oracle: no node commits at seeds 1..3 up to clock 1000, with
# or without the record exchange (a proposal that reaches 70 % of the nodes, whose votes arrive with 70 %, stays below the quorum of 27).
# The table keeps the smallest of them as a further zero-commit case and adds the heaviest live rates of the ladder 50 000 / 100 000 /
# 150 000 / 200 000 by clock 300: with the exchange (quirks bit 0) every node commits at every seed up to 150 000; without it some node
# commits at every seed up to 50 000 (tests/test_network_edges_host.py test_the_heavy_loss_rates_are_the_heaviest_live_ones).
DEAD_LOSS = 300000
LOSS_LADDER = (50000, 100000, 150000, 200000)
HEAVY_LOSS, HEAVY_LOSS_EXCHANGE = 50000, 150000
CUT = dict(partition_size=2, partition_start=100, partition_end=500)  # a cut the 4-node cases vary


def _seeds(k, first=1):
    return list(range(first, first + k))


def _case(name, n, cfg, seeds, max_clock, expect="equal", **kw):
    return dict(name=name, n=n, cfg=cfg, seeds=seeds, max_clock=max_clock, expect=expect, **kw)


CASES = [
    # ---- loss: the draw's threshold at its ends.  Loss excludes class 0; 4 nodes: class 1 on the array, 7: on the calendar ---------------
    _case("loss_1_per_million", 4, dict(drop_per_million=1), _seeds(3), 1000, kernel_class=1, calendar=False),
    _case("loss_999999", 4, dict(drop_per_million=999999), _seeds(3), 1000, kernel_class=1, calendar=False),
    _case("loss_1000000", 4, dict(drop_per_million=1000000), _seeds(3), 1000, kernel_class=1, calendar=False),
    _case("loss_2p32_minus_1", 4, dict(drop_per_million=U32), _seeds(3), 1000, kernel_class=1, calendar=False),
    _case("loss_total_7_nodes", 7, dict(drop_per_million=1000000), _seeds(3), 1000, kernel_class=1, calendar=True),
    _case("loss_total_40_nodes", 40, dict(drop_per_million=1000000), _seeds(2), 300, kernel_class=2, lean=False),
    _case("loss_total_40_nodes_quirks1", 40, dict(drop_per_million=1000000, quirks=1), _seeds(2), 300, kernel_class=2, lean=False),
    _case("loss_300000_40_nodes", 40, dict(drop_per_million=DEAD_LOSS), _seeds(2), 300, kernel_class=2, lean=False),
    _case("loss_300000_40_nodes_quirks1", 40, dict(drop_per_million=DEAD_LOSS, quirks=1), _seeds(2), 300, kernel_class=2, lean=False),
    _case("loss_heavy_40_nodes", 40, dict(drop_per_million=HEAVY_LOSS), _seeds(3), 300, kernel_class=2, lean=False),
    _case("loss_heavy_40_nodes_quirks1", 40, dict(drop_per_million=HEAVY_LOSS_EXCHANGE, quirks=1), _seeds(3), 300, kernel_class=2, lean=False),
    _case("loss_1_per_million_7_nodes", 7, dict(drop_per_million=1), _seeds(3), 1000, kernel_class=1, calendar=True),
    _case("loss_1_per_million_40_nodes", 40, dict(drop_per_million=1), _seeds(2), 300, kernel_class=2, lean=False),
    _case("loss_half_1_node", 1, dict(drop_per_million=500000), _seeds(3), 300),
    # ---- partition: sides that hold everybody, windows that are empty, reversed or outside i32 ------------------------------------------
    _case("partition_size_n", 4, dict(CUT, partition_size=4), _seeds(3), 1000, kernel_class=1),
    _case("partition_size_above_n", 4, dict(CUT, partition_size=9), _seeds(3), 1000, kernel_class=1),
    _case("partition_empty_window", 4, dict(CUT, partition_start=500, partition_end=500), _seeds(3), 1000, kernel_class=1),
    _case("partition_reversed_window", 4, dict(CUT, partition_start=600, partition_end=300), _seeds(3), 1000, kernel_class=1),
    _case("partition_window_past_2p40", 4, dict(CUT, partition_start=2 ** 40, partition_end=2 ** 41), _seeds(3), 1000, kernel_class=1),
    _case("partition_window_negative", 4, dict(CUT, partition_start=-10, partition_end=-1), _seeds(3), 1000, kernel_class=1),
    _case("partition_forever", 4, dict(CUT, partition_start=-5, partition_end=2 ** 40), _seeds(3), 1000, kernel_class=1),
    _case("partition_end_2p31_plus_5", 4, dict(CUT, partition_end=2 ** 31 + 5), _seeds(3), 1000, kernel_class=1),
    _case("partition_2_nodes_size_1", 2, dict(CUT, partition_size=1), _seeds(3), 1000, kernel_class=1),
    _case("partition_40_nodes_size_39", 40, dict(partition_size=39, partition_start=50, partition_end=200), _seeds(2), 300, kernel_class=2,
          lean=False),
    _case("partition_65_nodes_quirks3_size_64", 65, dict(quirks=3, partition_size=64, partition_start=50, partition_end=2 ** 62), _seeds(2),
          200, kernel_class=2, lean=False),
    # ---- equivocation: every node Byzantine; a period above every index (node 0 alone) ----------------------------------------------------
    _case("equivocate_all_4_nodes", 4, dict(equivocate_every=1), _seeds(3), 1000, block_capacity=2000, kernel_class=1),
    _case("equivocate_all_7_nodes_quirks3", 7, dict(equivocate_every=1, quirks=3), _seeds(3), 1000, block_capacity=2000, kernel_class=1),
    _case("equivocate_all_40_nodes", 40, dict(equivocate_every=1), _seeds(2), 300, block_capacity=2000, kernel_class=2, lean=True,
          exchange=False),
    _case("equivocate_all_40_nodes_quirks1", 40, dict(equivocate_every=1, quirks=1), _seeds(2), 300, block_capacity=2000, kernel_class=2,
          exchange=True),
    _case("equivocate_every_2p32_minus_1", 7, dict(equivocate_every=U32), _seeds(3), 1000, block_capacity=2000, kernel_class=1),
    # ---- voting rights: zeros, 24-bit rights, sums next to 2^32, a node that is a quorum by itself ----------------------------------------
    _case("rights_0_3_0_1_1", 5, dict(voting_rights=[0, 3, 0, 1, 1]), _seeds(3), 1000, weighted=True),
    _case("rights_2_1_0", 3, dict(voting_rights=[2, 1, 0]), _seeds(3), 1000, weighted=True),
    _case("rights_all_w_4_nodes", 4, dict(voting_rights=[W] * 4), _seeds(3), 1000, kernel_class=0, weighted=True),
    _case("rights_w_w_wm1_1", 4, dict(voting_rights=[W, W, W - 1, 1]), _seeds(3), 1000, kernel_class=0, weighted=True),
    _case("rights_w_1_w_1_w_0_w", 7, dict(voting_rights=[W, 1, W, 1, W, 0, W]), _seeds(3), 1000, weighted=True),
    _case("rights_w_1_alternating_20_nodes", 20, dict(voting_rights=[W, 1] * 10), _seeds(2), 300, kernel_class=1, weighted=True),
    _case("rights_w_1_alternating_40_nodes", 40, dict(voting_rights=[W, 1] * 20), _seeds(2), 300, kernel_class=2, lean=True),
    # (128 rights of 0xffffff: 2 * total_votes = 4 294 967 040, 256 below the u32 wrap)
    _case("rights_all_w_128_nodes", 128, dict(voting_rights=[W] * 128), _seeds(2), 120, kernel_class=2),
    _case("rights_w_0_1_w_2_rotating", 5, dict(voting_rights=[W, 0, 1, W, 2], rights_rotation=3, commands_per_epoch=3, quirks=3), _seeds(3),
          1000, weighted=True),
    # A node whose right alone reaches the quorum finishes several rounds per clock tick: 300 and more blocks by clock 300, against the
    # automatic block capacity max_clock / 10 + 64 = 94.  The sizing gap is recorded, not closed: explicit capacity -> equal,
    # automatic -> F_BLOCK_OVERFLOW and nothing else.
    _case("quorum_holder_4_nodes_explicit", 4, dict(voting_rights=[0, 0, 7, 0]), _seeds(3), 300, block_capacity=2048, weighted=True),
    _case("quorum_holder_4_nodes_automatic", 4, dict(voting_rights=[0, 0, 7, 0]), _seeds(3), 300, expect="fault:%d" % F_BLOCK_OVERFLOW),
    # (timed_max_clock: the horizon of this case's commit-time runs.  The oracle derives commit times by bisection over fresh runs, one
    # for every tick with a commit -- here every tick, 1 100 commits per node --, which takes a minute at clock 300 and a second at 100)
    _case("quorum_holder_7_nodes_quirks1_explicit", 7, dict(voting_rights=[0, 0, 0, 9, 0, 0, 0], quirks=1), _seeds(3), 300,
          block_capacity=2048, weighted=True, timed_max_clock=100),
    _case("quorum_holder_7_nodes_quirks1_automatic", 7, dict(voting_rights=[0, 0, 0, 9, 0, 0, 0], quirks=1), _seeds(3), 300,
          expect="fault:%d" % F_BLOCK_OVERFLOW),
    _case("rights_last_of_40_nodes", 40, dict(voting_rights=[0] * 39 + [1]), _seeds(2), 150, block_capacity=2048, kernel_class=2),
    # ---- rotation: taken modulo num_nodes; nothing to rotate with unit rights ------------------------------------------------------------
    _case("rotation_13_on_5_nodes", 5, dict(voting_rights=[3, 1, 2, 1, 1], rights_rotation=13, commands_per_epoch=3, quirks=3), _seeds(3),
          1000),
    _case("rotation_2p32_minus_1_on_7_nodes", 7, dict(voting_rights=[3, 1, 2, 1, 1, 2, 1], rights_rotation=U32, commands_per_epoch=3, quirks=3),
          _seeds(3), 1000),
    _case("rotation_of_unit_rights", 5, dict(rights_rotation=2, commands_per_epoch=3, quirks=3), _seeds(3), 1000),
    # ---- epochs: one command per epoch under every quirks mode; an epoch that never ends --------------------------------------------------
    _case("epoch_of_1_command_quirks0", 4, dict(commands_per_epoch=1, quirks=0), _seeds(3), 1000, kernel_class=0),
    _case("epoch_of_1_command_quirks1", 5, dict(commands_per_epoch=1, quirks=1), _seeds(3), 1000, kernel_class=1),
    _case("epoch_of_1_command_quirks2", 4, dict(commands_per_epoch=1, quirks=2), _seeds(3), 1000, kernel_class=0),
    _case("epoch_of_1_command_quirks3", 5, dict(commands_per_epoch=1, quirks=3), _seeds(3), 1000, kernel_class=1),
    _case("epoch_of_1_command_40_nodes_quirks1", 40, dict(commands_per_epoch=1, quirks=1), _seeds(2), 250, kernel_class=2, exchange=True),
    _case("epoch_of_1_command_40_nodes_quirks3", 40, dict(commands_per_epoch=1, quirks=3), _seeds(2), 250, kernel_class=2, exchange=True),
    _case("epoch_of_2p32_minus_1_commands", 4, dict(commands_per_epoch=U32), _seeds(3), 1000, kernel_class=0),
    _case("epoch_of_1_command_1_node_quirks3", 1, dict(commands_per_epoch=1, quirks=3), _seeds(3), 300),
    # ---- sizes and seeds: LBFT_MAX_NODES_SUPPORTED, the sizes around the wavefront and tile widths, the ends of the seed range -------------
    _case("size_128_nodes", 128, dict(), _seeds(2), 120, kernel_class=2, lean=True, exchange=False),
    _case("size_128_nodes_quirks3_lossy", 128, dict(quirks=3, drop_per_million=100000), _seeds(2), 100, kernel_class=2, lean=False),
    _case("size_17_nodes", 17, dict(), _seeds(3), 300, kernel_class=1),
    _case("size_32_nodes_quirks3", 32, dict(quirks=3), _seeds(2), 300, kernel_class=1),
    _case("size_33_nodes", 33, dict(), _seeds(2), 300, kernel_class=2, lean=True, exchange=False),
    _case("size_64_nodes_quirks1", 64, dict(quirks=1), _seeds(2), 200, kernel_class=2, exchange=True),
    _case("size_65_nodes", 65, dict(), _seeds(2), 200, kernel_class=2, lean=True, exchange=False),
    _case("seeds_0_2p63_2p64_minus_1", 4, dict(), [0, 2 ** 63, 2 ** 64 - 1], 1000, kernel_class=0),
]

# Identities of the oracle: the named case gives bit for bit the run of the same case with these configuration fields instead.
SAME_AS = {
    "loss_2p32_minus_1": dict(drop_per_million=1000000),
    "partition_size_n": dict(partition_size=0),
    "partition_size_above_n": dict(partition_size=0),
    "partition_empty_window": dict(partition_size=0),
    "partition_reversed_window": dict(partition_size=0),
    "partition_window_past_2p40": dict(partition_size=0),
    "partition_window_negative": dict(partition_size=0),
    "equivocate_every_2p32_minus_1": dict(equivocate_every=7),
    "rotation_13_on_5_nodes": dict(rights_rotation=3),
    "rotation_2p32_minus_1_on_7_nodes": dict(rights_rotation=3),
    "rotation_of_unit_rights": dict(rights_rotation=0),
}
# The cases in which no node ever commits: they must still do work (timers fire, messages are drawn and lost) for the counters to compare.
NO_COMMIT = ("loss_999999", "loss_1000000", "loss_2p32_minus_1", "loss_total_7_nodes", "loss_total_40_nodes", "loss_total_40_nodes_quirks1",
             "loss_300000_40_nodes", "loss_300000_40_nodes_quirks1", "partition_forever", "equivocate_all_4_nodes",
             "equivocate_all_7_nodes_quirks3", "equivocate_all_40_nodes", "equivocate_all_40_nodes_quirks1")
# The oracle's summed events (notify, request, response, timer) of whole cases, measured once and pinned.
ORACLE_EVENTS = {"loss_1000000": [0, 0, 0, 27], "partition_forever": [21, 1148, 1137, 2316]}


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def layout_flags(case):
    """{flag name: value} of what the case pins of lbft_batch_layout's flag word."""
    return {k: case[k] for k in ("kernel_class", "calendar", "lean", "exchange") if k in case}


def check_layout_flags(case, flags):
    for key, want in layout_flags(case).items():
        got = flags & 0xff if key == "kernel_class" else bool(flags & dict(calendar=LAYOUT_CALENDAR, lean=LAYOUT_LEAN, exchange=LAYOUT_EXCHANGE)[key])
        assert got == want, (case["name"], key, hex(flags))


def make_sim(m, case, commit_times=False):
    """The case's batch on the device (``m``: the librabft_simulator_amd package), not run yet."""
    import numpy as np
    f = dict(quirks=0, drop_per_million=0, commands_per_epoch=30000, equivocate_every=0, rights_rotation=0, voting_rights=None,
             partition_size=0, partition_start=0, partition_end=0)
    assert set(case["cfg"]) <= set(f), case["name"]
    f.update(case["cfg"])
    partition = (f["partition_size"], f["partition_start"], f["partition_end"]) if f["partition_size"] else None
    return m.BatchSimulator.new(np.array(case["seeds"], dtype=np.uint64), case["n"], m.RandomDelay.new(10.0, 4.0), m.NodeConfig(),
                                commands_per_epoch=f["commands_per_epoch"], voting_rights=f["voting_rights"], quirks=f["quirks"],
                                drop_per_million=f["drop_per_million"], equivocate_every=f["equivocate_every"], partition=partition,
                                rights_rotation=f["rights_rotation"], block_capacity=case.get("block_capacity", 0), commit_times=commit_times)


# ---- refused configurations: decided by validate() / fill_params / lbft_batch_create_param_sets before the first HIP call --------------------
REFUSED = [
    dict(name="refused_0_nodes", n=0, cfg=dict(), code=LBFT_ERR_INVALID),
    dict(name="refused_129_nodes", n=129, cfg=dict(), code=LBFT_ERR_UNSUPPORTED),
    dict(name="refused_quirks_4", n=4, cfg=dict(quirks=4), code=LBFT_ERR_UNSUPPORTED),
    dict(name="refused_delay_model_2", n=4, cfg=dict(delay_model=2), code=LBFT_ERR_INVALID),
    dict(name="refused_0_commands_per_epoch", n=4, cfg=dict(commands_per_epoch=0), code=LBFT_ERR_INVALID),
    dict(name="refused_right_of_2p24", n=4, cfg=dict(voting_rights=[1, W + 1, 1, 1]), code=LBFT_ERR_INVALID),
    dict(name="refused_all_rights_zero", n=4, cfg=dict(voting_rights=[0, 0, 0, 0]), code=LBFT_ERR_INVALID),
]
# lbft_batch_create_param_sets: (nodes, number of sets, set_of_instance, code)
REFUSED_PARAM_SETS = [
    dict(name="refused_0_sets", n=4, n_sets=0, set_of=[0, 0], code=LBFT_ERR_INVALID),
    dict(name="refused_257_sets", n=4, n_sets=257, set_of=[0, 256], code=LBFT_ERR_INVALID),
    dict(name="refused_set_index_n_sets", n=4, n_sets=3, set_of=[0, 1, 2, 3], code=LBFT_ERR_INVALID),
    dict(name="refused_sets_33_nodes", n=33, n_sets=2, set_of=[0, 1], code=LBFT_ERR_UNSUPPORTED),
]


def refused_config(case):
    """The refused case as the C ABI's lbft_config."""
    from librabft_simulator_amd import _lib
    import ctypes
    c = _lib.LbftConfig()
    f = dict(mean=10.0, variance=4.0, delay_model=0, uniform_lo=5, uniform_hi=15, target_commit_interval=100000, delta=20, gamma=2.0,
             lambda_=0.5, quirks=0, commands_per_epoch=30000)
    f.update({k: v for k, v in case["cfg"].items() if k != "voting_rights"})
    c.num_nodes = case["n"]
    for k, v in f.items():
        setattr(c, k, v)
    if "voting_rights" in case["cfg"]:
        c._keepalive = (ctypes.c_uint64 * case["n"])(*case["cfg"]["voting_rights"])
        c.voting_rights = ctypes.cast(c._keepalive, ctypes.POINTER(ctypes.c_uint64))
    return c


# ---- parameter-set batches: an ordinary set 0 beside sets at the ends of the loss and partition words, interleaved, three instances per set ----
ORDINARY = dict(mean=10.0, variance=4.0, uniform_lo=5, uniform_hi=15, delta=20, gamma=2.0, lambda_=0.5, target_commit_interval=100000)
NETWORK_SETS = [
    dict(),
    dict(drop_per_million=1),
    dict(drop_per_million=999999),
    dict(drop_per_million=1000000),
    dict(drop_per_million=U32),
    dict(partition=(2, -5, 2 ** 40)),        # cut forever
    dict(partition=(200, 100, 500)),         # a side that holds everybody
    dict(partition=(2, 500, 500)),           # an empty window
    dict(partition=(2, 600, 300)),           # a reversed window
    dict(partition=(2, 100, 2 ** 31 + 5)),   # a window past 2^31
    dict(drop_per_million=500000, partition=(2, 100, 500)),
]
# (32 nodes with quirks bit 0 are left out: the host harness's snapshot pool runs out there -- fault word 2, the sizing gap of ADVICE.md)
PARAM_SET_CASES = [
    dict(name="network_sets_4_nodes", n=4, base=dict(), sets=NETWORK_SETS, per=3, max_clock=1000, kernel_class=1),
    dict(name="network_sets_7_nodes", n=7, base=dict(), sets=NETWORK_SETS, per=3, max_clock=1000, kernel_class=1),
    dict(name="network_sets_4_nodes_all_equivocate", n=4, base=dict(equivocate_every=1, block_capacity=2000), sets=NETWORK_SETS, per=3,
         max_clock=1000, kernel_class=1),
    dict(name="network_sets_20_nodes", n=20, base=dict(), sets=NETWORK_SETS, per=3, max_clock=300, kernel_class=1),
    dict(name="network_sets_5_nodes_rotating_rights", n=5,
         base=dict(voting_rights=[W, 0, 1, W, 2], rights_rotation=3, commands_per_epoch=3, quirks=3), sets=NETWORK_SETS, per=3, max_clock=1000,
         kernel_class=1),
]


def set_layout(case):
    """(set_of_instance, seeds): `per` instances of every set, interleaved so that extreme and ordinary sets share wavefronts."""
    n_sets = len(case["sets"])
    m = n_sets * case["per"]
    return [i % n_sets for i in range(m)], [1000 + i for i in range(m)]


def set_as_case(case, k):
    """Set k of a parameter-set case as a plain case (for the oracle)."""
    s = case["sets"][k]
    cfg = {key: v for key, v in case["base"].items() if key != "block_capacity"}
    cfg["drop_per_million"] = s.get("drop_per_million", 0)
    if "partition" in s:
        cfg["partition_size"], cfg["partition_start"], cfg["partition_end"] = s["partition"]
    return dict(name="%s[%d]" % (case["name"], k), n=case["n"], cfg=cfg, max_clock=case["max_clock"], expect="equal")


def param_sets(m, case):
    """The sets as ParamSet objects (``m``: the package): Python accepts every value of the table."""
    return [m.ParamSet(m.RandomDelay.new(ORDINARY["mean"], ORDINARY["variance"]),
                       m.NodeConfig(ORDINARY["target_commit_interval"], ORDINARY["delta"], ORDINARY["gamma"], ORDINARY["lambda_"]),
                       drop_per_million=s.get("drop_per_million", 0), partition=s.get("partition")) for s in case["sets"]]


def base_kwargs(case):
    """The batch-wide settings of a parameter-set case, as keyword arguments of BatchSimulator."""
    return dict(case["base"])
