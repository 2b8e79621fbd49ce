"""The configurations the vote-statistics tests share (tests/test_vote_stats_host.py, tests/test_vote_stats_gpu.py) and the oracle's
side of each, computed once per process: every seed run on the oracle with the reference CLI defaults and turned into samples by
vote_stats_reference.instance.  Test infrastructure."""
import vote_stats_reference as ref

# name -> (configuration, max_clock, seeds)
CASES = {
    "n4": (dict(num_nodes=4), 1000, range(1, 17)),
    "n5_weighted": (dict(num_nodes=5, voting_rights=[5, 1, 1, 1, 1]), 1000, range(1, 9)),
    "n4_partition_q3": (dict(num_nodes=4, quirks=3, partition_size=1, partition_start=300, partition_end=600), 1500, range(1, 17)),
    "n4_rotating_q3": (dict(num_nodes=4, voting_rights=[1, 2, 3, 4], commands_per_epoch=5, quirks=3, rights_rotation=1), 1500, range(1, 9)),
    "n7_equivocators_lossy_q3": (dict(num_nodes=7, equivocate_every=3, drop_per_million=50000, quirks=3), 1000, range(1, 5)),
    "n4_longer_than_64": (dict(num_nodes=4), 2500, range(1, 4)),  # the chain and the pool both exceed one chunk of 64
    "n4_empty_chain": (dict(num_nodes=4), 20, range(1, 4)),       # L == 0: no tip, everything is pending
    "n33": (dict(num_nodes=33), 400, range(1, 3)),                # the second voter word
    "n65_q3": (dict(num_nodes=65, quirks=3), 400, range(1, 3)),   # two node rounds, a third voter word
}

_instances = {}


def oracle_instances(oracle, kw, max_clock, seeds):
    """vote_stats_reference.instance of every seed's oracle run (cached: a reference is computed once and left unchanged)."""
    key = (tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())), max_clock, tuple(seeds))
    if key not in _instances:
        cfg = oracle.make_config(**kw)
        out = []
        for seed in seeds:
            sim = oracle.OracleSim(cfg, int(seed)).run_until(max_clock)
            out.append(ref.instance(sim, kw["num_nodes"], kw.get("voting_rights"), kw.get("rights_rotation", 0)))
            sim.close()
        _instances[key] = out
    return _instances[key]


def case_instances(oracle, name):
    kw, max_clock, seeds = CASES[name]
    return oracle_instances(oracle, kw, max_clock, seeds)


def expected(instances, n, rights, width=None, bins=None, faults=None, set_of=None, groups=1):
    """The call's four arrays for (width, bins) -- None: the default binning -- from the oracle's instances."""
    w, b = ref.default_binning(rights, n)
    width, bins = (w if width is None else width), (b if bins is None else bins)
    return ref.bin_votes(ref.group(instances, faults, set_of, groups), n, width, bins)
