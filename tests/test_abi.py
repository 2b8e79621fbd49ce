"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/lbft.h declares, and fails loudly (no fallback) when there is no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from support import hiplib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_exported(hiplib):
    header = open(os.path.join(ROOT, "include", "lbft.h")).read()
    declared = set(re.findall(r"\b(lbft_[a-z_0-9]+)\s*\(", header))
    declared -= {"lbft_batch"}
    assert declared == set(hiplib.ABI_SYMBOLS), declared ^ set(hiplib.ABI_SYMBOLS)
    raw = ctypes.CDLL(hiplib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(raw, name), name
    assert b"gfx950" in hiplib.lib().lbft_build_info()


def test_config_struct_matches_header_layout(hiplib):
    # lbft_config: 2*u32, 2*f64, 2*i64, u64, 2*i64, 2*f64, 2*u32, ptr, 4*u32
    assert ctypes.sizeof(hiplib.LbftConfig) == 8 + 16 + 16 + 8 + 16 + 16 + 8 + 8 + 16 + 8 + 16 + 8  # + lossy-network fields + rights_rotation (padded)
    assert ctypes.sizeof(hiplib.LbftCounters) == 8 * 15
    assert hiplib.COMMIT_DTYPE.itemsize == 24


def test_library_has_no_oracle_or_host_fallback(hiplib):
    # the product library must not link the oracle or the host build of the model
    import subprocess
    out = subprocess.run(["ldd", hiplib.LIB_PATH], capture_output=True, text=True).stdout
    assert "lbft_oracle" not in out and "hostmodel" not in out
    syms = subprocess.run(["nm", "-D", "--defined-only", hiplib.LIB_PATH], capture_output=True, text=True).stdout
    assert "lbft_oracle" not in syms and "lbft_hostmodel" not in syms


def test_argument_validation_needs_no_gpu(hiplib):
    L = hiplib.lib()
    h = ctypes.c_void_p()
    cfg = hiplib.LbftConfig()
    cfg.num_nodes = 0
    seeds = np.arange(4, dtype=np.uint64)
    assert L.lbft_batch_create(ctypes.byref(cfg), seeds.ctypes.data, 4, 0, ctypes.byref(h)) == hiplib.LBFT_ERR_INVALID
    cfg.num_nodes = 4
    cfg.mean, cfg.variance, cfg.commands_per_epoch = 10.0, 4.0, 30000
    cfg.quirks = 4  # bits 0 (Q1 fixed) and 1 (Q2 fixed) exist; anything else does not
    assert L.lbft_batch_create(ctypes.byref(cfg), seeds.ctypes.data, 4, 0, ctypes.byref(h)) == hiplib.LBFT_ERR_UNSUPPORTED
    cfg.quirks = 0
    cfg.num_nodes = 129  # LBFT_MAX_NODES_SUPPORTED is 128
    assert L.lbft_batch_create(ctypes.byref(cfg), seeds.ctypes.data, 4, 0, ctypes.byref(h)) == hiplib.LBFT_ERR_UNSUPPORTED
    assert L.lbft_batch_run_until(None, 10) == hiplib.LBFT_ERR_INVALID


def test_fails_loudly_without_gpu(hiplib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from librabft_simulator_amd import LbftError, RandomDelay, Simulator
    with pytest.raises(LbftError) as e:
        Simulator.new(52, 3, RandomDelay.new(10.0, 4.0)).loop_until(1000)
    assert e.value.code == hiplib.LBFT_ERR_HIP


def _kernel_metadata(so_path):
    """name -> {private_segment_fixed_size, group_segment_fixed_size, vgpr_count, vgpr_spill_count, sgpr_count} of every gfx950 kernel in the library
    (the code object is unbundled from .hip_fatbin and its AMDGPU metadata note read with llvm-readelf)."""
    import struct
    import subprocess
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so_path, fat])
        blob = open(fat, "rb").read()
        assert blob.startswith(b"__CLANG_OFFLOAD_BUNDLE__")
        n = struct.unpack_from("<Q", blob, 24)[0]
        off, code = 32, None
        for _ in range(n):
            o, s, ts = struct.unpack_from("<QQQ", blob, off)
            off += 24
            triple = blob[off:off + ts].decode()
            off += ts
            if "gfx950" in triple:
                code = blob[o:o + s]
        assert code is not None, "no gfx950 code object in the library"
        co = os.path.join(d, "dev.co")
        open(co, "wb").write(code)
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co]).decode()
    kernels = {}
    for chunk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", chunk).group(1)
        kernels[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, chunk).group(1))
                         for k in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_count")}
    return kernels


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_run_kernels_keep_their_state_in_registers(hiplib):
    """The event loop is one fully inlined function whose per-lane state (node cache, block cache, RNG) must be promoted
    to registers.  Two innocent-looking source patterns have silently moved it to scratch memory before (conditional
    stores to cache entries sunk into a phi of addresses; two table lookups merged into a load through a phi of `this`
    and the kernel-argument block), costing 15 % and 3x: the headline kernel may spill a handful of registers (the state
    itself is > 160 bytes) and must fit two wavefronts per SIMD (<= 256 registers)."""
    kernels = _kernel_metadata(hiplib.LIB_PATH)
    run0 = [v for k, v in kernels.items() if "lbft_k_run0" in k and "lbft_k_run0s" not in k and "lbft_k_run0q" not in k and "lbft_k_run0u" not in k]
    run0q = [v for k, v in kernels.items() if "lbft_k_run0q" in k]  # the headline network fixed at compile time
    assert len(run0q) == 1 and run0q[0]["vgpr_count"] <= 256 and run0q[0]["private_segment_fixed_size"] <= 384, run0q
    assert len(run0) == 1, sorted(kernels)
    # (round 3, instance-major rows: the wide node / snapshot loads need register tuples, and ~46 loop-INVARIANT values -- kernel
    # arguments, LDS bases -- are parked in scratch before the loop and reloaded after it: 188 bytes, two reloads inside the loop on
    # the rare propose path; the whole per-lane state in scratch would be > 600 bytes)
    # (+ ~25 more since the retired record stores can be archived, SimT::retire_store: parked loop-invariants again -- measured
    # 21.80 ms with it, 21.88 ms compiled out)
    assert run0[0]["private_segment_fixed_size"] <= 384 and run0[0]["vgpr_spill_count"] <= 96, run0
    run0s = [v for k, v in kernels.items() if "lbft_k_run0s" in k]  # the small-batch form (wavefront-wide pop)
    assert len(run0s) == 1 and run0s[0]["vgpr_count"] <= 256 and run0s[0]["private_segment_fixed_size"] <= 384, run0s
    assert run0[0]["vgpr_count"] <= 256, run0
    big = [v for k, v in kernels.items() if "lbft_k_runILi" in k]
    assert len(big) == 2, sorted(kernels)
    for v in big:  # large-network classes: a handful of spilled registers at most, never the whole state
        assert v["private_segment_fixed_size"] <= 128, big
    lean = [v for k, v in kernels.items() if "lbft_k_run1l" in k]  # class 1 without record exchange / trace / loss: two wavefronts per SIMD as well
    assert len(lean) == 1 and all(v["vgpr_count"] <= 256 and v["private_segment_fixed_size"] <= 160 for v in lean), lean
    # large networks, two wavefronts per SIMD: without (run2l) and with (run2q) the record exchange of quirks bit 0.  They only pay while the
    # trimmed loop keeps its state in registers: 4 / 24 spilled registers as built; 118 (staged sets) and 325 (a second inlined copy of
    # update_node's tail inside handle_response) were slower than one wavefront per SIMD
    # (round 3: 38 / 70 with SimT::retire_store compiled in -- values parked around the loop: 362 vs 365 ms and 3.03 vs 2.98 s against the
    # build without it)
    # (round 6: 37 / 60 after the runs and the packed shuffle; 62 / 119 with the lane-parallel shuffle, whose eight 64-bit masks are live for 7 ballots --
    # measured FASTER than the serial shuffle's 37 / 60 at the same ring top-up where the shuffle is long (c5 640 -> 613 ms, c5live 1 282 -> 1 209 ms) and
    # within 1 % elsewhere: profiles/r06/parallel_shuffle_and_ring_topup_ab.txt.  The exact counts are pinned by tests/golden/kernel_manifest.json; these
    # caps only catch the state itself moving to scratch: hundreds)
    for name, cap in (("lbft_k_run2l", 72), ("lbft_k_run2q", 128)):
        lean2 = [v for k, v in kernels.items() if name in k]
        assert len(lean2) == 1 and lean2[0]["vgpr_count"] <= 256 and lean2[0]["vgpr_spill_count"] <= cap, (name, lean2)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_uniform_kernel_compiles_to_scalar_code(hiplib):
    """lbft_k_run0u (SimT<K_SMALL_UNIFORM>: batches with one network per wavefront; round 5: 1 024 x 4 networks 4.88 ms against 5.27 on lbft_k_run0s): nothing in
    its event loop depends on the lane, so that the compiler keeps the step on the scalar unit.  One source of divergence slipping in -- an
    inline-asm pin, a flat load, the return value of an out-of-line helper -- silently turns the whole loop back into masked vector code:
    the register budget tells (162 VGPRs in the product build -- most of them lanes that park scalar state --, 215+ as vector code: lbft_k_run0s)."""
    from librabft_simulator_amd import build
    k = [v for name, v in _kernel_metadata(build.OUT).items() if "lbft_k_run0u" in name]
    assert len(k) == 1 and k[0]["vgpr_count"] <= 176 and k[0]["private_segment_fixed_size"] == 0, k


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_built_kernels_match_the_committed_codegen_manifest(hiplib):
    """tests/golden/kernel_manifest.json pins, per kernel, the machine code (bytes + sha256), VGPRs, SGPRs, spilled registers and scratch bytes of the
    library the round's numbers were measured on, and the hipcc that built it.  The large-network kernels sit on a register-allocation knife's edge
    (round 5: deleting a DEAD struct member grew lbft_k_run2l from 135 to 142 KB and cost 14 % on the device): any deviation -- a source edit, a
    toolchain change -- fails here on the CPU box instead of costing time on the GPU unnoticed.  A deliberate kernel change regenerates the manifest
    in the same commit, after measuring it: python tools/kernel_manifest.py --write."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_manifest
    committed = json.load(open(kernel_manifest.MANIFEST))
    built = kernel_manifest.manifest(hiplib.LIB_PATH)
    for k in ("lbft_k_run0q", "lbft_k_run0", "lbft_k_run0s", "lbft_k_run0u", "lbft_k_run1l", "lbft_k_run2l", "lbft_k_run2q", "lbft_k_run<1>", "lbft_k_run<2>",
              "lbft_k_init", "lbft_k_finalize"):
        assert k in built["kernels"], (k, sorted(built["kernels"]))
    d = kernel_manifest.diff(committed, built)
    toolchain = committed["hipcc"] != built["hipcc"]
    assert not d, ("the built kernels deviate from tests/golden/kernel_manifest.json%s:\n  %s\nre-measure (tools/gpu_configs_profile.sh) and regenerate it in "
                   "the same commit: python tools/kernel_manifest.py --write" % (" (DIFFERENT hipcc: every kernel needs re-measuring)" if toolchain else "", "\n  ".join(d)))


def test_launchers_are_exported_by_their_own_library_alone(hiplib):
    """build.TABLE: every launcher liblbft_hip.so looks up lives in its side library and in none of the other five."""
    from librabft_simulator_amd import build
    assert [lib.tag for lib in build.TABLE] == ["hip", "paramsets", "commit_times", "round_stats", "chain_stats", "record_hashes"]
    assert build.TABLE[0].out == build.OUT and not build.TABLE[0].launchers and all(lib.launchers for lib in build.TABLE[1:])
    assert build.LIBS == tuple((lib.src, lib.out, build.include_closure(lib.src)) for lib in build.TABLE)
    loaded = {lib.tag: ctypes.CDLL(lib.out) for lib in build.TABLE}
    for lib in build.TABLE:
        for name in lib.launchers:
            for tag, raw in loaded.items():
                assert hasattr(raw, name) == (tag == lib.tag), (name, tag)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_side_kernels_carry_their_prefix_and_stay_out_of_every_other_library(hiplib):
    from librabft_simulator_amd import build
    kernels = {lib.tag: sorted(_kernel_metadata(lib.out)) for lib in build.TABLE}
    for lib in build.TABLE[1:]:
        assert kernels[lib.tag] and all(lib.prefix in k for k in kernels[lib.tag]), (lib.tag, kernels[lib.tag])
        for tag, names in kernels.items():
            assert tag == lib.tag or not any(lib.prefix in k for k in names), (lib.prefix, tag, names)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
def test_table_of_run_kernels_names_the_run_kernels_of_the_built_libraries(hiplib, oracle):
    """csrc/lbft_plan.h's table against the binaries: every row's name is a kernel of the row's library, and no library holds a run
    kernel the table lacks."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_manifest
    from librabft_simulator_amd import build
    rows = oracle.run_kernels()
    for k, lib in enumerate(build.TABLE):
        built = {kernel_manifest.short(name) for name in _kernel_metadata(lib.out)}
        in_table = {r["name"] for r in rows if r["lib"] == k}
        assert in_table == {name for name in built if "_run" in name}, (lib.tag, sorted(in_table), sorted(built))
    assert len({r["name"] for r in rows}) == len(rows) == 15 and {r["lib"] for r in rows} == {0, 1, 2}


def test_table_names_the_files_and_launchers_the_host_code_opens():
    """The Python table cannot drift from csrc: the side libraries' file names are the LBFT_*_LIB macros of their headers, the launchers
    the strings lbft_hip.hip passes to load_side_lib."""
    from librabft_simulator_amd import build
    csrc = os.path.join(ROOT, "librabft_simulator_amd", "csrc")
    macros = {}
    for f in sorted(os.listdir(csrc)):
        macros.update(re.findall(r'^#define (LBFT_\w+_LIB) "([^"]+)"', open(os.path.join(csrc, f)).read(), re.M))
    table = {os.path.basename(lib.out): lib.launchers for lib in build.TABLE[1:]}
    assert sorted(macros.values()) == sorted(table) and len(macros) == 5, macros
    calls = re.findall(r'load_side_lib\((LBFT_\w+_LIB),\s*"[^"]*",\s*\{(.*?)\}\);', open(build.SRC).read(), re.S)
    opened = {macros[macro]: tuple(re.findall(r'\{"(\w+)"', body)) for macro, body in calls}
    assert len(calls) == 5 and opened == table, (opened, table)
    for lib in build.TABLE:
        assert os.path.dirname(lib.src) == csrc and os.path.isfile(lib.src), lib.src


def test_a_newer_header_makes_exactly_the_libraries_that_include_it_stale(tmp_path):
    """On a copy of the sources with built libraries older than all of them: one header at a time made newer."""
    import shutil
    from librabft_simulator_amd import build
    shutil.copytree(os.path.join(ROOT, "librabft_simulator_amd", "csrc"), tmp_path / "librabft_simulator_amd" / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    libs = {}
    for lib in build.TABLE:
        deps = build.include_closure(str(tmp_path / os.path.relpath(lib.src, ROOT)))
        out = str(tmp_path / os.path.basename(lib.out))
        assert build._stale(out, deps)  # not built yet
        open(out, "wb").close()
        os.utime(out, (1000, 1000))
        libs[lib.tag] = (out, deps)
        assert [os.path.relpath(d, tmp_path) for d in deps] == [os.path.relpath(d, ROOT) for d in build.LIBS[build.TABLE.index(lib)][2]]
    files = sorted(set(d for _out, deps in libs.values() for d in deps))
    for f in files:
        os.utime(f, (900, 900))
    assert not any(build._stale(out, deps) for out, deps in libs.values())
    for f in files:
        os.utime(f, (1100, 1100))
        assert {tag: build._stale(out, deps) for tag, (out, deps) in libs.items()} == {tag: f in deps for tag, (_out, deps) in libs.items()}, f
        os.utime(f, (900, 900))
    # an include that does not resolve is an error, not a dependency nobody watches
    (tmp_path / "lost.hip").write_text('#include "include/lbft.h"\n  #  include "no_such_header.h"\n')
    with pytest.raises(FileNotFoundError):
        build.include_closure(str(tmp_path / "lost.hip"))


def test_kernel_hash_reads_the_code_object(hiplib):
    """build.kernel_hash(): the stamp that ties profiles/current/pmc_traffic.json to the kernels bench.py runs (sha256 of the
    gfx950 machine code in the built library; parsed without binutils so that it works on the GPU box)."""
    import json
    from librabft_simulator_amd import build
    h = build.kernel_hash()
    assert re.fullmatch(r"[0-9a-f]{16}", h) and h == build.source_hash()
    stamp = json.load(open(os.path.join(ROOT, "profiles", "current", "pmc_traffic.json"))).get("source_hash")
    assert re.fullmatch(r"[0-9a-f]{16}", stamp)  # (equal to h while the committed profile belongs to the built kernels; bench.py reports null otherwise)


def test_kernel_names_from_the_layout_flag_word():
    """bench.py and tools/configs.py name the run kernel of a batch from lbft_batch_layout's flag word (include/lbft.h:
    class | heap << 8 | calendar << 9 | two-wavefront kernel << 10 | cooperative sends << 11 | ... with record exchange << 12)."""
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    import configs
    for kc, name in ((0, "lbft_k_run0"), (8192, "lbft_k_run0s"), (8192 | 32768, "lbft_k_run0u"), (16384, "lbft_k_run0q"), (1 | 1024, "lbft_k_run1l"), (1, "lbft_k_run<1>"), (2 | 256 | 512 | 2048, "lbft_k_run<2>"),
                     (2 | 256 | 512 | 1024 | 2048, "lbft_k_run2l"), (2 | 256 | 512 | 1024 | 2048 | 4096, "lbft_k_run2q")):
        assert bench.run_kernel_name(kc) == name
        assert configs.kernel_name({"kernel_class": kc}) == name
    # ... and every row of csrc/lbft_plan.h's table of run kernels, its word put together from the size class in its name and its flag
    # bits: the decoders know the main library's kernels; a twin (bits 16 / 17) reads as the plain kernel whose geometry it borrows
    import oracle_ctypes
    for r in oracle_ctypes.run_kernels():
        size = int(re.search(r"run<?(\d)", r["name"]).group(1))
        want = r["name"] if r["lib"] == 0 else ("lbft_k_run0", "lbft_k_run<1>")[size]
        assert bench.run_kernel_name(size | r["flags"]) == configs.kernel_name({"kernel_class": size | r["flags"]}) == want, r


def test_hip_soname_reader_reads_only_the_dynamic_section_and_refuses_garbage(hiplib, tmp_path):
    """_lib._needed_hip_soname: the HIP runtime this library was linked against / the soname of torch's bundled copy, read with seeks (not
    by slurping tens of MB); a file that is not an ELF object raises instead of letting the caller guess (round-4 advisor)."""
    assert hiplib._needed_hip_soname(hiplib.LIB_PATH).startswith("libamdhip64.so")
    junk = tmp_path / "junk.so"
    junk.write_bytes(b"not an elf file" * 100)
    with pytest.raises(ValueError):
        hiplib._needed_hip_soname(str(junk))


def test_one_hip_runtime_whichever_of_torch_and_the_library_comes_first(hiplib):
    """PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64; two ROCr runtimes in one process leave the second without devices
    (torch.cuda.is_available() False after the library was used first).  _lib._one_hip_runtime maps torch's copy first."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import librabft_simulator_amd as L\n"
            "L.lib()\n"
            "import torch\n"
            "libs = sorted(set(l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l or 'libhsa-runtime64' in l))\n"
            "print(len(libs), libs)\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[0] == "2", out.stdout  # one libamdhip64, one libhsa-runtime64
