"""bench.py's launch contract, the parts that need no GPU: `python bench.py --gpus N` without a launcher
re-executes itself under torch.distributed.run with N ranks; a launcher whose WORLD_SIZE disagrees with --gpus is an error.  Also --steps and
--dump-outputs DIR (the last timed step's outputs as .npy files; one gpu-marked test runs it for real)."""
import importlib.util
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gpus_without_launcher_reexecutes_under_torch_distributed_run(monkeypatch):
    bench = _bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and "--nnodes=1" in cmd
    # the launcher picks its own free port (--standalone: no bind-close-reuse race here) and rendezvouses on 127.0.0.1
    assert "--standalone" in cmd and cmd[cmd.index("--local-addr") + 1] == "127.0.0.1" and "--master-port" not in cmd
    k = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[k + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]  # the ranks see the same command line
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"  # (only a default: a caller's own setting is kept)


def test_hsa_ipc_setting_of_the_caller_is_kept(monkeypatch):
    bench = _bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["env"] = env
        return 0
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "1")
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 0
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "1"


def test_gpus_left_at_its_default_adopts_the_launchers_world_size():
    """`torchrun --nproc-per-node 3 bench.py` with no --gpus: the launcher's WORLD_SIZE is the number of ranks (round-4 advisor); the run then stops at
    the next check -- no GPU here -- instead of at a disagreement."""
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], env=env, capture_output=True, text=True, timeout=300)
    assert "--gpus" not in out.stderr and "rank(s)" not in out.stderr
    import torch
    if not torch.cuda.is_available():
        assert out.returncode != 0 and "needs a GPU" in out.stderr


def test_world_size_exported_without_a_launcher_does_not_block_the_self_launch(monkeypatch):
    """A scheduler that merely exports WORLD_SIZE (no RANK) is not a launcher: `python bench.py --gpus 2` still starts its own ranks."""
    bench = _bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"] = cmd
        return 0
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.setenv("WORLD_SIZE", "16")
    monkeypatch.delenv("RANK", raising=False)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 0
    assert seen["cmd"][seen["cmd"].index("--nproc-per-node") + 1] == "2"


def test_world_size_disagreeing_with_gpus_is_an_error():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--gpus 2" in out.stderr and "3 rank" in out.stderr


def test_one_gpu_never_relaunches(monkeypatch):
    bench = _bench()

    def fake_call(cmd, env=None):
        raise AssertionError("N = 1 must not start a launcher")
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    import torch
    if torch.cuda.is_available():
        return  # (on a GPU box the run itself is covered by the -m gpu tests)
    try:
        bench.main()
        raise AssertionError("expected the no-GPU exit")
    except SystemExit as e:
        assert "needs a GPU" in str(e.code)


def test_steps_below_one_are_refused(monkeypatch):
    """`--steps` is the number of timed steps and `ms_per_step` is divided by it: zero steps is an argument error, not a division by zero."""
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    try:
        bench.parse()
        raise AssertionError("expected an argument error")
    except SystemExit as e:
        assert e.code == 2


def test_only_full_or_an_explicit_count_turns_the_parity_gate_on(monkeypatch):
    """A plain run (the driver's `--gpus 1 --steps K --warmup W`) re-runs nothing on the oracle; --full gates 16 384 instances of the timed batch, and
    --parity-instances sets the count with or without --full."""
    bench = _bench()
    for argv, full, parity in ((["--gpus", "1", "--steps", "20", "--warmup", "5"], False, 0),
                               (["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"], True, 16384),
                               (["--full", "--parity-instances", "0"], True, 0),
                               (["--parity-instances", "256"], False, 256)):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        args = bench.parse()
        assert (args.full, args.parity_instances) == (full, parity), argv
        assert args.measure_traffic is None  # (decided in main(): on for a --full headline run on one GPU)


class _FakeResult:
    """The parts of BatchResult that bench.dump_outputs reads: n instances of `nodes` nodes, seeded."""

    def __init__(self, n, nodes):
        import numpy as np
        rng = np.random.default_rng(7)
        self.commit_counts = rng.integers(0, 80, (n, nodes)).astype(np.uint32)
        self.active_rounds = rng.integers(0, 300, (n, nodes)).astype(np.uint64)
        self.last_committed_states = rng.integers(0, 2 ** 64, (n, nodes), dtype=np.uint64, endpoint=False)
        self.startup_times = rng.integers(0, 50, (n, nodes)).astype(np.int64)
        self.epochs = np.zeros((n, nodes), dtype=np.uint64)
        self.faults = np.zeros(n, dtype=np.uint32)
        self.counters = {"events": [11, 12, 13, 14], "rounds": 15, "commits": 16, "rng_draws": 17, "faulted_instances": 0, "launches": 1}

    def committed_history(self, instance, node):
        import numpy as np
        from librabft_simulator_amd._lib import COMMIT_DTYPE
        k = int(self.commit_counts[instance, node])
        h = np.zeros(k, dtype=COMMIT_DTYPE)
        h["proposer"], h["index"], h["time"] = node, np.arange(k), 1000 * instance + np.arange(k)
        return h


def _load_dump(path):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_writes_exact_float64_arrays(tmp_path):
    import numpy as np
    bench = _bench()
    res = _FakeResult(300, 4)
    info = bench.dump_outputs(str(tmp_path), res)
    d = _load_dump(str(tmp_path))
    assert info["arrays"] == len(d) and info["bytes"] == sum(a.nbytes for a in d.values()) <= 64 << 20
    assert all(a.dtype == np.float64 for a in d.values())
    assert (d["instances"] == np.arange(300)).all()  # a small batch is written whole
    assert (d["commit_counts"] == res.commit_counts).all() and (d["active_rounds"] == res.active_rounds).all()
    states = d["last_committed_states_hi"].astype(np.uint64) << np.uint64(32) | d["last_committed_states_lo"].astype(np.uint64)
    assert (states == res.last_committed_states).all()  # the u64 hashes survive float64 exactly
    assert (d["counters"] == [11, 12, 13, 14, 15, 16, 17, 0]).all()
    hrows = d["history_instances"].astype(np.int64)
    assert len(hrows) == 300 and d["committed_history_index"].shape == (300, 4, 64)
    for i, inst in enumerate(hrows[:20]):
        for node in range(4):
            k = min(int(res.commit_counts[inst, node]), 64)
            assert (d["committed_history_index"][i, node, :k] == np.arange(k)).all() and not d["committed_history_index"][i, node, k:].any()
            assert (d["committed_history_time"][i, node, :k] == 1000 * inst + np.arange(k)).all()


def test_dump_outputs_samples_a_large_batch_the_same_way_every_time(tmp_path):
    import numpy as np
    bench = _bench()
    res = _FakeResult(1 << 20, 4)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert bench.dump_outputs(a, res)["bytes"] <= 64 << 20
    bench.dump_outputs(b, res)
    da, db = _load_dump(a), _load_dump(b)
    rows = da["instances"].astype(np.int64)
    assert 0 < len(rows) < 1 << 20 and (np.diff(rows) > 0).all()
    assert (da["commit_counts"] == res.commit_counts[rows]).all()
    assert da.keys() == db.keys() and all((da[k] == db[k]).all() for k in da)


def test_traffic_children_do_not_dump_outputs(monkeypatch):
    """The rocprofv3 child runs of --measure-traffic rebuild the command line: they must not write the parent's outputs (nor see the flag), and
    they are plain runs (no --full, no parity gate)."""
    import shutil
    bench = _bench()
    seen = []

    class Done:
        returncode, stdout, stderr = 1, "", "stop"

    def fake_run(cmd, **kw):
        seen.append(cmd)
        return Done()
    monkeypatch.setattr(shutil, "which", lambda name: "/bin/" + name)
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.delenv("LBFT_BENCH_CHILD", raising=False)
    for argv in (["--steps", "3", "--dump-outputs", "outdir", "--measure-traffic"], ["--dump-outputs=outdir", "--steps", "3", "--full", "--parity-instances", "64"]):
        seen.clear()
        assert "error" in bench.traffic_measured_here(argv)
        child = seen[0][seen[0].index("--") + 1:]
        assert child[2:4] == ["--steps", "3"] and "outdir" not in child and not any(a.startswith("--dump-outputs") for a in child)
        assert "--measure-traffic" not in child and "--full" not in child
        monkeypatch.setattr(sys, "argv", ["bench.py"] + child[2:])
        assert bench.parse().parity_instances == 0


@pytest.mark.gpu
def test_a_plain_headline_run_prints_the_line_and_nothing_of_full():
    """The driver's plain command on the headline workload: the result line with its headline keys, and none of what --full adds (parity gate, CPU
    baseline, config 3's strong split, traffic measured in child runs)."""
    import json
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["unit"] == "rounds/s" and line["higher_is_better"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["metric"].startswith("simulated consensus rounds/sec") and line["dtype"] and (line["steps"], line["warmup"]) == (2, 1)
    assert line["faulted_instances"] == 0 and line["config"]["instances_per_gpu"] == 65536
    assert not {"parity", "cpu_baseline", "config3_strong"} & line.keys() and line["roofline"]["traffic_measured_here"] is None


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_exactly_and_equal_the_oracle(tmp_path, oracle):
    """Two runs with other step counts compute the same thing in their last timed step: the dumps are equal array for array, and the dumped
    histories are the oracle's on the same seeds (seed_i = base_seed + i)."""
    import json
    import numpy as np
    dumps = []
    for steps, warmup in ((1, 0), (3, 1)):
        d = str(tmp_path / ("s%d" % steps))
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--instances", "2048",
                              "--no-cpu-baseline", "--no-measure-traffic", "--parity-instances", "256", "--dump-outputs", d],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["dumped_outputs"]["dir"] == d
        dumps.append(_load_dump(d))
    a, b = dumps
    assert a.keys() == b.keys() and all((a[k] == b[k]).all() for k in a)
    assert (a["instances"] == np.arange(2048)).all()
    hrows = a["history_instances"].astype(np.int64)
    ref = oracle.run_batch(oracle.make_config(num_nodes=4, math_mode=1), (hrows + 1).astype(np.uint64), 1000, threads=8, history_cap=64)
    assert (a["commit_counts"][hrows] == ref["commit_counts"]).all()
    for field in ("proposer", "index", "time"):
        assert (a["committed_history_" + field] == ref["histories"][field]).all()
