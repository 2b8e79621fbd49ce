"""TEST INFRASTRUCTURE: the shapes at which a wavefront of the grouped statistic kernels (lbft_k_cs_chain, lbft_k_ct_finality,
lbft_k_rs_rounds) takes more than one instance, in one place: tests/test_strided_shapes_host.py states on the CPU that they do, and
tests/test_grouped_stats_stride_gpu.py runs them on the device.

The kernels' grid is (workgroups per group, groups); the WAVES wavefronts of a workgroup stride over the instances of their group,

    for (q = blockIdx.x * WAVES + wave; q < cnt; q += gridDim.x * WAVES) { one instance }

and gs_workgroups() (csrc/lbft_group_stats.h) gives gridDim.x = min(max(1, 1024 / groups), ceil(largest group / WAVES)) while no
workgroup could count 2^32 samples.  A wavefront therefore makes a second trip only in a plain batch of more than 4096 instances, or
in a parameter-set batch whose largest group exceeds 4 * (1024 / groups) instances.

The layout: 256 parameter sets (the maximum: 4 workgroups per group, 16 instances per step).  Background group k holds k % 4
instances, set 255 none; six groups are special (SPECIAL).  set_of is a fixed-seed permutation, so a group's instances lie scattered
over the batch and grp_inst is a real gather.  The plain shapes (PLAIN, WEIGHTED) hold 4102 instances: 1026 steps > 1024 workgroups,
a stride of 4096 instances, grp_inst == NULL."""
import numpy as np

from librabft_simulator_amd.simulator import NodeConfig, ParamSet, RandomDelay

WAVES = 4  # LBFT_CS_WAVES, LBFT_FN_WAVES, LBFT_RS_WAVES: wavefronts per workgroup
TARGET = 1024  # LBFT_CS_WORKGROUPS, LBFT_FN_WORKGROUPS, LBFT_RS_WORKGROUPS
GROUPS = 256
MAX_CLOCK = 1000
ROUND_TRACE = 256

# group -> instances.  38: wavefront positions 0..5 make three trips and 6..15 two -- inside workgroup 1 (positions 4..7) waves 0 and 1
# three and waves 2 and 3 two; 33: position 0 alone makes a third trip; 17: one wavefront makes a second trip; 16: exactly one step.
FAST, DEFAULT, THIRD, G33, G17, G16 = 37, 102, 171, 214, 9, 250
SPECIAL = {FAST: 38, DEFAULT: 38, THIRD: 38, G33: 33, G17: 17, G16: 16}
STRIDED = (FAST, DEFAULT, THIRD, G33, G17)  # the groups in which a wavefront takes more than one instance
EMPTY_LAST = GROUPS - 1

PARTITION = (1, 300, 600)  # ends inside the horizon
# flavour -> what the batch runs.  "class0": lane-private class-0 rows (no partition, no quirks: the planner takes a batch with either
# to class 1); "partition": the third strided group's set cuts node 0 off during PARTITION, quirks = 3; "tiles": 7 nodes, quirks = 3 and
# 2 % loss in every set, 64-wide tiles.
FLAVOURS = {
    "class0": dict(n=4, quirks=0, drop=0, partition=None, background=True),
    "partition": dict(n=4, quirks=3, drop=0, partition=PARTITION, background=True),
    "tiles": dict(n=7, quirks=3, drop=20000, partition=PARTITION, background=False),
}

# (seeds 1 .. m, PLAIN's counted down: in that order a wavefront that makes two trips takes, in both shapes, a second instance whose
# round table is shorter than its first one's -- a row count kept from the first trip shows)
PLAIN = dict(m=4102, n=4, max_clock=300, descending=True, kw={})
WEIGHTED = dict(m=4102, n=5, max_clock=500, descending=False, kw=dict(voting_rights=[5, 1, 1, 1, 1], commands_per_epoch=3, rights_rotation=1, quirks=3))

_MEANS = ((3.0, 1.0), (5.0, 2.0), (10.0, 4.0), (20.0, 9.0))
_DELTAS = (20, 10, 40)


def gs_workgroups(target, n_groups, steps, max_samples):
    """csrc/lbft_group_stats.h gs_workgroups(), in Python."""
    gx = target // n_groups or 1
    gx = max(gx, (max_samples >> 31) + 1)
    return min(gx, steps)


def grid_x(n_groups, max_group, per_instance, target=TARGET, waves=WAVES):
    """gridDim.x of a launch over n_groups groups whose largest has max_group instances of at most per_instance samples a bin."""
    return gs_workgroups(target, n_groups, (max_group + waves - 1) // waves, max_group * per_instance)


def trips(group_size, gx, waves=WAVES):
    """The trips of the stride loop per wavefront position q0 = blockIdx.x * waves + wave, q0 < gx * waves."""
    return [len(range(q0, group_size, gx * waves)) for q0 in range(gx * waves)]


def group_sizes(background=True):
    sizes = np.array([k % 4 if background else 0 for k in range(GROUPS)])
    sizes[EMPTY_LAST] = 0
    for g, size in SPECIAL.items():
        sizes[g] = size
    return sizes


def assignment(background=True):
    """(set_of, seeds) of the layout: a fixed-seed permutation of the groups' instances, seeds 1 .. m."""
    set_of = np.random.default_rng(256).permutation(np.repeat(np.arange(GROUPS), group_sizes(background))).astype(np.uint32)
    return set_of, np.arange(1, len(set_of) + 1, dtype=np.uint64)


def members(set_of, g):
    """The instances of group g in instance order: the order in which GroupIndex lists them, position q of the stride loop."""
    return np.nonzero(np.asarray(set_of) == g)[0]


def kind_of_group(g):
    """What group g runs, as a hashable key: the oracle runs every kind once."""
    if g in (FAST, DEFAULT, THIRD):
        return {FAST: "fast", DEFAULT: "default", THIRD: "third"}[g]
    return ((g // 4) % 4, (g // 16) % 3)


def param_set(kind, flavour):
    f = FLAVOURS[flavour]
    if kind == "fast":
        return ParamSet(RandomDelay.new(3.0, 1.0), NodeConfig(), f["drop"])
    if kind == "default":
        return ParamSet(RandomDelay.new(10.0, 4.0), NodeConfig(), f["drop"])
    if kind == "third":  # (without the partition it still is a set of its own: delta 40)
        return ParamSet(RandomDelay.new(10.0, 4.0), NodeConfig(100000, 20 if f["partition"] else 40, 2.0, 0.5), f["drop"], f["partition"])
    (mean, variance), delta = _MEANS[kind[0]], _DELTAS[kind[1]]
    return ParamSet(RandomDelay.new(mean, variance), NodeConfig(100000, delta, 2.0, 0.5), f["drop"])


def param_sets(flavour):
    return [param_set(kind_of_group(g), flavour) for g in range(GROUPS)]


def per_kind(set_of, seeds, flavour, run):
    """run(param set, seeds) -> a tuple of arrays [instance, ...], once per kind; -> the tuples' arrays in the batch's instance order,
    last axes padded with zeros to the longest."""
    kinds = [kind_of_group(int(g)) for g in set_of]
    parts = []
    for kind in sorted(set(kinds), key=str):
        idx = np.array([i for i, k in enumerate(kinds) if k == kind])
        parts.append((idx, run(param_set(kind, flavour), seeds[idx])))
    out = []
    for a in range(len(parts[0][1])):
        arrays = [p[a] for _, p in parts]
        shape = tuple(max(x.shape[d] for x in arrays) for d in range(1, arrays[0].ndim))
        whole = np.zeros((len(set_of),) + shape, dtype=arrays[0].dtype)
        for (idx, _), x in zip(parts, arrays):
            whole[(idx,) + tuple(slice(0, s) for s in x.shape[1:])] = x
        out.append(whole)
    return tuple(out)


_ORACLE = {}


def oracle_layout(oracle, flavour):
    """(set_of, seeds, (histories, commit counts, startup times)) of the layout on the oracle; computed once per process."""
    if flavour not in _ORACLE:
        import chain_stats_reference as chain_ref
        from support import oracle_cfg
        f = FLAVOURS[flavour]
        set_of, seeds = assignment(f["background"])
        want = per_kind(set_of, seeds, flavour,
                        lambda ps, s: chain_ref.oracle_batch(oracle, oracle_cfg(oracle, f["n"], ps, quirks=f["quirks"]), s, MAX_CLOCK))
        _ORACLE[flavour] = (set_of, seeds, want)
    return _ORACLE[flavour]


def plain_seeds(shape):
    seeds = np.arange(1, shape["m"] + 1, dtype=np.uint64)
    return seeds[::-1].copy() if shape["descending"] else seeds


def oracle_plain(oracle, shape):
    """(seeds, (histories, commit counts, startup times)) of a plain shape (PLAIN, WEIGHTED) on the oracle; once per process."""
    key = ("plain", shape["n"])
    if key not in _ORACLE:
        import chain_stats_reference as chain_ref
        from support import oracle_cfg
        seeds = plain_seeds(shape)
        cfg = oracle_cfg(oracle, shape["n"], ParamSet(), **shape["kw"])
        _ORACLE[key] = (seeds, chain_ref.oracle_batch(oracle, cfg, seeds, shape["max_clock"]))
    return _ORACLE[key]


def fault_case(want, set_of):
    """Case B: the log capacity (the median chain length of the FAST group) and the fault words it gives -- an instance overflows its
    logs when a node commits more entries than they hold."""
    lengths = want[1].max(axis=1)
    lcap = int(np.median(lengths[members(set_of, FAST)]))
    return lcap, np.where(lengths > lcap, 1 << 3, 0).astype(np.uint32)  # LBFT_FAULT_LOG_OVERFLOW
