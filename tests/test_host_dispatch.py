"""The class the host models step a batch as.  They take it from the planner's kernel choice (csrc/lbft_plan.h pick_run_kernel and the
table of run kernels, through oracle/host_model_common.h run_instance); before the table existed each model derived it by a chain of
conditions of its own.  The expected words below are those chains' answers: recorded by running exactly these calls on a build of the
commit before the table, not by the code under test.  Only the class matters, so every run is one seed to clock 0: the nodes start up,
no event is processed."""
import numpy as np
import pytest

import switch_batches as sb
from test_dirty_state_host import last_class

# lbft_hostmodel_last_class after one network of every batch of tests/switch_batches.py with the planner's capacities and queue
# discipline: KernelClass of the step (lbft_core.h) | cooperative event loop << 8 | heap << 9 | calendar << 10
HOST_CLASS = {
    "headline": 9, "headline_cpe7": 9, "c0_n7": 0,
    "c1_n4_equiv": 6, "c1_n4_equiv4": 6, "c1_n7_equiv": 6 | 512 | 1024, "c1_n20": 6 | 512 | 1024,
    "c2_n40": 5 | 256 | 512 | 1024, "c2_n40_q1": 7 | 256 | 512 | 1024, "c2_n100": 5 | 256 | 512 | 1024, "c2_n100_q1": 7 | 256 | 512 | 1024,
    "c2_n40_epochs_q3": 7 | 256 | 512 | 1024, "c2_n40_lossy": 2 | 256 | 512 | 1024, "c2_n40_heap": 5 | 512,
}


def host_class(oracle, name, **more):
    """One network of batch ``name`` on the host model -> lbft_hostmodel_last_class."""
    b = sb.BATCHES[name]
    plan = sb.planned(oracle, name, 1)
    caps = dict({k: plan[k] for k in ("qcap", "scap", "bcap", "lcap", "qheap", "qcal", "ring", "ring_topup")}, ql=0 if plan["qcal"] else 16)
    res = oracle.hostmodel_run_batch(oracle.make_config(math_mode=1, **b["kw"]), np.array([7], dtype=np.uint64), 0, **dict(caps, **more))
    assert not res["faults"].any()
    return last_class(oracle)


@pytest.mark.parametrize("name", sorted(sb.BATCHES))
def test_host_model_steps_every_switch_batch_as_the_class_it_did_before_the_table(oracle, name):
    assert set(HOST_CLASS) == set(sb.BATCHES)
    assert host_class(oracle, name) == HOST_CLASS[name]
    # the run-time-generic step has no run kernel and never the cooperative loop: the queue bits stay, the class is K_GENERIC
    assert host_class(oracle, name, force_generic=1) == (HOST_CLASS[name] & ~0x1ff) | 3


def twin_batch(equivocate_every, n_sets):
    """Four nodes, honest (kernel class 0) or with an equivocator (class 1), as the twin host models take a batch: the base
    configuration, ``n_sets`` parameter sets, one instance of each (of the base alone: a plain batch) -> base, sets, set_of, seeds."""
    from librabft_simulator_amd import _lib
    base = _lib.LbftConfig()
    base.num_nodes, base.commands_per_epoch, base.equivocate_every = 4, 30000, equivocate_every
    base.mean, base.variance, base.delta, base.gamma, base.lambda_, base.target_commit_interval = 10.0, 4.0, 20, 2.0, 0.5, 100000
    sets = []
    for k in range(n_sets):
        s = _lib.LbftParamSet()
        s.mean, s.variance, s.delta, s.gamma, s.lambda_, s.target_commit_interval = 10.0 + 5 * k, 4.0, 20, 2.0, 0.5, 100000
        sets.append(s)
    m = max(n_sets, 1)
    return base, sets, np.arange(m, dtype=np.uint32), np.arange(1, m + 1, dtype=np.uint64)


# (equivocate_every, parameter sets) -> the value ps_hostmodel_run / ct_hostmodel_run returned before the table: K_SMALL or K_MID
# (tests/test_param_sets_host_model.py and tests/test_commit_times_host_model.py, which have the compiled models, assert it)
TWIN_CLASS = {(0, 0): 0, (0, 2): 0, (3, 0): 1, (3, 2): 1}
