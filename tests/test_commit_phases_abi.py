"""CPU-side checks of the commit phases (lbft_batch_commit_phases): the entry point is declared, exported and bound, the constants are
what the header defines, the launcher lives in liblbft_commit_times.so alone, the arguments that need no batch are refused before any
HIP call with nothing written, the Python methods check `edges` before any library call, the grid tool knows the option, and the kernel
is in the side library's code object exactly once, under a name the other ABI tests do not pick up, without scratch or spilled
registers and with an LDS footprint that lets two workgroups share a compute unit."""
import ctypes
import os
import re

import numpy as np
import pytest

import commit_phases_reference as ref
from support import Stub, hiplib, other_libs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "librabft_simulator_amd", "csrc")
NAME = "lbft_batch_commit_phases"
LAUNCHER = "lbft_ct_launch_phases"
KERNEL = "lbft_k_ct_phases"


def test_symbol_is_declared_exported_and_bound(hiplib):
    from librabft_simulator_amd import build
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    assert NAME in declared and NAME in hiplib.ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(hiplib.LIB_PATH), NAME)
    assert len(getattr(hiplib.lib(), NAME).argtypes) == 8
    assert re.search(r"#define LBFT_MAX_PHASES 8\b", header) and re.search(r"#define LBFT_PHASE_FAMILIES 6\b", header)
    assert re.search(r"#define LBFT_PHASE_STATS 24\b", header)
    assert hiplib.MAX_PHASES == 8 == ref.MAX_PHASES and hiplib.PHASE_STATS == 24 == ref.PHASE_STATS == 4 * len(hiplib.PHASE_FAMILIES)
    assert tuple(hiplib.PHASE_FAMILIES) == ref.NAMES and len(set(ref.NAMES)) == 6 == ref.FAMILIES
    assert "open" in header[header.index("Commit phases:"):header.index("#define LBFT_MAX_PHASES")]  # the header says that `open` is not split
    # the launcher: in the commit-time library, in no other, in the table and in the typedefs
    assert LAUNCHER in build.TABLE[2].launchers and build.TABLE[2].tag == "commit_times"
    assert hasattr(ctypes.CDLL(build.CT_OUT), LAUNCHER)
    for other in (hiplib.LIB_PATH, *other_libs("commit_times")):
        assert not hasattr(ctypes.CDLL(other), LAUNCHER), other
    assert "lbft_ct_phases_fn" in open(os.path.join(CSRC, "lbft_commit_times.h")).read()
    rules = os.path.join(CSRC, "lbft_commit_phases.h")
    assert rules in build.CT_DEPS and rules not in build.DEPS  # liblbft_hip.so includes nothing of it: its device code stays as it is
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", open(rules).read())
    assert sorted(includes) == ["lbft_group_stats.h", "stdint.h"]
    main = open(os.path.join(CSRC, "lbft_hip.hip")).read()
    assert main.count("load_side_lib(") == 6 and len(build.TABLE) == 6  # its definition and five calls; six libraries


def test_bad_arguments_are_refused_without_a_gpu(hiplib):
    """Step 1 of the refusals needs no batch: with a NULL batch every call is LBFT_ERR_INVALID and writes nothing."""
    L = hiplib.lib()
    call = getattr(L, NAME)
    lat, fin, stats = (np.full(16 * 8, 7, dtype=np.uint64) for _ in range(3))
    edges = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.int64)
    out = (lat.ctypes.data, fin.ctypes.data, stats.ctypes.data)
    for e, phases, width, bins in ((None, 1, 1, 16), (edges.ctypes.data, 3, 1, 16), (edges.ctypes.data, 8, 1, 16), (edges.ctypes.data, 0, 1, 16),
                                   (edges.ctypes.data, 9, 1, 16), (None, 2, 1, 16), (None, 1, 0, 16), (None, 1, 1, 0), (None, 1, 1, 2 ** 32 - 1)):
        assert call(None, e, phases, width, bins, *out) == hiplib.LBFT_ERR_INVALID, (phases, width, bins)
        for k in range(3):
            holed = list(out)
            holed[k] = None
            assert call(None, e, phases, width, bins, *holed) == hiplib.LBFT_ERR_INVALID
    assert (lat == 7).all() and (fin == 7).all() and (stats == 7).all()


def test_python_methods_refuse_bad_edges_before_the_device():
    from librabft_simulator_amd.simulator import BatchResult, ParamSet
    res = BatchResult(Stub())  # one group, max_clock 1000
    bad = ([5, 3], [0, 10, 9], [-1], [1002], [0, 1002], [[1, 2], [3, 4]], [1, 2, 3, 4, 5, 6, 7, 8], "partition_end", "during", [[1, 2], 3], [[[1]]])
    for edges in bad:
        with pytest.raises(ValueError):
            res.phase_histogram(edges)
        with pytest.raises(ValueError):
            res.phases_by_param_set(edges)
    with pytest.raises(ValueError):
        res.phase_histogram([10], bin_width=0)
    assert res._phase_edges([]).shape == (1, 0) and res._phase_edges([0, 0, 1001]).tolist() == [[0, 0, 1001]]
    assert res._phase_edges([[300, 600]]).tolist() == [[300, 600]] and res._phase_edges(np.array([[5, 5]])).tolist() == [[5, 5]]
    assert res._phase_edges("partition").tolist() == [[1001, 1001]]  # no partition: everything is "before"

    class Sets(Stub):
        param_sets = [ParamSet(), ParamSet(partition=(2, 300, 600)), ParamSet(partition=(0, 300, 600)), ParamSet(partition=(1, 900, 5000))]
    sets = BatchResult(Sets())
    assert sets._phase_edges("partition").tolist() == [[1001, 1001], [300, 600], [1001, 1001], [900, 1001]]
    assert sets._phase_edges([10, 20]).tolist() == [[10, 20]] * 4 and sets._phase_edges([[1], [2], [3], [4]]).tolist() == [[1], [2], [3], [4]]
    for edges in ([[1], [2], [3]], [[1], [2], [3], [4, 5]], [[1, 2]], [[1], [2], [3], [1002]], [[2, 1], [2, 3], [2, 3], [2, 3]]):
        with pytest.raises(ValueError):  # wrong number of groups, ragged, out of range, decreasing in one group
            sets.phase_histogram(edges)


def test_grid_phases_option_is_parsed(capsys):
    from librabft_simulator_amd import grid
    assert grid._phases("300,600") == [300, 600] and grid._phases("partition") == "partition" and grid._phases(" 7 ") == [7]
    for bad in ("x", "5,3", "1,2,3,4,5,6,7,8", "-1", "", "3,,4", "1.5", "partitions"):
        with pytest.raises(SystemExit):  # a malformed value ends the tool before it creates a batch
            grid.main(["--phases", bad] if not bad.startswith("-") else ["--phases=" + bad])
    with pytest.raises(SystemExit):
        grid.main(["--phases", "10,2000", "--max-clock", "1000"])  # an edge past max_clock + 1
    with pytest.raises(SystemExit):
        grid.main(["--phases", "partition", "--seeds-per-point", "0"])
    with pytest.raises(SystemExit):
        grid.main(["--phases"])
    capsys.readouterr()
    assert "--phases" in grid.__doc__


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_kernel_is_in_the_commit_time_library_without_scratch(hiplib):
    """LDS: the tile of 4 wavefronts x 32 nodes x 64 entries x 4 B = 32 KiB, two histograms of 4096 u32 bins, 32 rights, 8 edges and
    8 phases x 24 words of statistics: 67 232 B; a compute unit has 160 KiB, so two workgroups share it when each takes at most 80 KiB."""
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    ct = _kernel_metadata(build.CT_OUT)
    mine = [(k, v) for k, v in ct.items() if KERNEL in k]
    assert len(mine) == 1 and len([k for k in ct if re.search(r"\d+%sN" % KERNEL, k)]) == 1, sorted(ct)
    name, meta = mine[0]
    for word in ("run", "finality", "timeline", "latency_hist", "instances"):  # the substrings the other ABI tests pick their kernels by
        assert word not in name, name
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta.get("sgpr_spill_count", 0) == 0, meta
    assert meta["group_segment_fixed_size"] == 4 * 32 * 64 * 4 + 2 * 4 * ref.LDS_BINS + 32 * 4 + 8 * 4 + 8 * 24 * 8 <= 80 * 1024, meta
    assert meta["vgpr_count"] <= 128, meta  # four wavefronts per SIMD: the two workgroups a unit's LDS admits at the very least
    for other in other_libs("commit_times"):
        assert not any(KERNEL in k for k in _kernel_metadata(other)), other
    regs = open(os.path.join(ROOT, "profiles", "commit_phases", "kernel_regs.txt")).read()
    assert KERNEL in regs
