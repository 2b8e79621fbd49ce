"""The configurations the epoch-statistics tests share (tests/test_epoch_stats_host.py, tests/test_epoch_stats_gpu.py) and the oracle's
side of each, computed once per process: every seed run on the oracle with the reference CLI defaults and turned into samples by
epoch_stats_reference.instance.  Each case is the smallest shape at which one part of the kernel can go wrong.  Test infrastructure."""
import epoch_stats_reference as ref

Q3 = dict(num_nodes=4, quirks=3)
SEEDS = range(1, 5)
# name -> (configuration, max_clock, seeds, epoch_bins)
CASES = {
    "n4_default": (dict(num_nodes=4), 1000, SEEDS, 64),                                  # one open segment, no boundary, nothing stranded
    "n4_cpe5_q3": (dict(Q3, commands_per_epoch=5), 1000, SEEDS, 64),                      # 5-6 segments, an open one of one entry
    "n4_cpe1_q3": (dict(Q3, commands_per_epoch=1), 1000, SEEDS, 64),                      # every entry its own segment
    "n4_cpe32_q3": (dict(Q3, commands_per_epoch=32), 2500, SEEDS, 64),                    # a boundary at entry 64: the chunk edge
    "n4_cpe64_q3": (dict(Q3, commands_per_epoch=64), 2500, SEEDS, 64),                    # the only boundary at entry 64
    "n4_cpe21_q3": (dict(Q3, commands_per_epoch=21), 2500, SEEDS, 64),                    # a boundary at entry 63
    "n4_cpe13_q3": (dict(Q3, commands_per_epoch=13), 2500, SEEDS, 64),                    # a boundary at entry 65
    "n4_cpe70_q3": (dict(Q3, commands_per_epoch=70), 5000, SEEDS, 64),                    # a segment over two chunk edges, three chunks
    "n4_cpe50_q0": (dict(num_nodes=4, commands_per_epoch=50), 2500, SEEDS, 64),           # the stall after the first epoch change
    "n4_rotating_q3": (dict(Q3, voting_rights=[1, 2, 3, 4], commands_per_epoch=5, rights_rotation=1), 1500, SEEDS, 64),
    "n7_equivocators_lossy_cpe3_q3": (dict(num_nodes=7, equivocate_every=3, drop_per_million=50000, commands_per_epoch=3, quirks=3), 1000, SEEDS, 64),
    "n33_cpe4_q3": (dict(num_nodes=33, commands_per_epoch=4, quirks=3), 400, range(1, 3), 64),
    "n65_cpe4_q3": (dict(num_nodes=65, commands_per_epoch=4, quirks=3), 400, range(1, 3), 64),  # two node rounds
    "n4_empty_chain": (dict(num_nodes=4), 20, range(1, 4), 64),                          # L == 0: no segment, no tip
    "n4_three_epoch_bins": (dict(Q3, commands_per_epoch=5), 1000, SEEDS, 3),              # the last row of the table collects
    # 308 epochs: the time columns of rows 256 and above are added to the global table directly (lbft_k_ps_epochs' EP_LDS_SUM_ROWS)
    "n4_cpe1_q3_above_256_epochs": (dict(Q3, commands_per_epoch=1), 20000, range(1, 2), 512),
}

_instances = {}


def oracle_instances(oracle, kw, max_clock, seeds):
    """epoch_stats_reference.instance of every seed's oracle run (cached: a reference is computed once and left unchanged)."""
    key = (tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())), max_clock, tuple(seeds))
    if key not in _instances:
        cfg = oracle.make_config(**kw)
        out = []
        for seed in seeds:
            sim = oracle.OracleSim(cfg, int(seed)).run_until(max_clock)
            out.append(ref.instance(sim, kw["num_nodes"]))
            sim.close()
        _instances[key] = out
    return _instances[key]


def case_instances(oracle, name):
    kw, max_clock, seeds, _ = CASES[name]
    return oracle_instances(oracle, kw, max_clock, seeds)


def expected(instances, max_clock, epoch_bins=64, width=None, bins=None, faults=None, set_of=None, groups=1):
    """The call's three arrays for (width, bins) -- None: the default binning -- from the oracle's instances."""
    width, bins = ref.default_binning(max_clock, width, bins)
    return ref.bin_epochs(ref.group(instances, faults, set_of, groups), width, bins, epoch_bins)
