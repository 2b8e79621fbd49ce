"""Build the HIP libraries (hand-written HIP for gfx950) in-tree with hipcc: `python -m librabft_simulator_amd.build` or `build()`.
The libraries are git-ignored build products; TABLE below names them, and what each depends on is read from its sources:
"""
import collections
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))

# One library: its tag, source and output file, the prefix of its kernels' names (None: the main library, which holds every other
# kernel), the launchers it exports for liblbft_hip.so to look up (load_side_lib in lbft_hip.hip), and what it holds in one line.
Lib = collections.namedtuple("Lib", "tag src out prefix launchers holds")


def _lib(tag, prefix, launchers, holds):
    return Lib(tag, os.path.join(HERE, "csrc", "lbft_%s.hip" % tag), os.path.join(HERE, "liblbft_%s.so" % tag), prefix, launchers, holds)


TABLE = (
    _lib("hip", None, (), "the C ABI of include/lbft.h and its kernels; opens the others beside itself on first use, so that its own "
                          "code object stays as it is"),
    _lib("paramsets", "lbft_k_ps_", ("lbft_ps_launch_init", "lbft_ps_launch_run", "lbft_ps_launch_counters", "lbft_ps_launch_load",
                                     "lbft_ps_launch_votes", "lbft_ps_launch_epochs"),
         "the kernels of parameter-set batches (lbft_batch_create_param_sets) and the counters, run-load, vote-statistics and "
         "epoch-statistics kernels behind every finished run"),
    _lib("commit_times", "lbft_k_ct_", ("lbft_ct_launch_run", "lbft_ct_launch_histogram", "lbft_ct_launch_timeline", "lbft_ct_launch_finality",
                                        "lbft_ct_launch_instances", "lbft_ct_launch_phases"),
         "the kernels of batches that record commit times (lbft_batch_record_commit_times)"),
    _lib("round_stats", "lbft_k_rs_", ("lbft_rs_launch_rounds",), "the kernel of lbft_batch_round_stats"),
    _lib("chain_stats", "lbft_k_cs_", ("lbft_cs_launch_chain",), "the kernel of lbft_batch_chain_stats"),
    _lib("record_hashes", "lbft_k_rh_", ("lbft_rh_launch_chain",), "the kernel of lbft_batch_chain_record_hashes"),
)
__doc__ = (__doc__ or "") + "".join("%s: %s.\n" % (os.path.basename(lib.out), lib.holds) for lib in TABLE)

_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def include_closure(src):
    """`src` and every file its quoted #include lines reach, each resolved relative to the file that includes it.  An include
    that does not resolve raises: a header nobody watches would let a stale library be served."""
    seen, todo = [], [os.path.normpath(src)]
    while todo:
        path = todo.pop(0)
        if path in seen:
            continue
        seen.append(path)
        with open(path) as f:
            text = f.read()
        for inc in _INCLUDE.findall(text):
            dep = os.path.normpath(os.path.join(os.path.dirname(path), inc))
            if not os.path.isfile(dep):
                raise FileNotFoundError('%s: #include "%s" does not resolve (%s)' % (path, inc, dep))
            todo.append(dep)
    return seen


LIBS = tuple((lib.src, lib.out, include_closure(lib.src)) for lib in TABLE)
(SRC, OUT, DEPS), (PS_SRC, PS_OUT, PS_DEPS), (CT_SRC, CT_OUT, CT_DEPS), (RS_SRC, RS_OUT, RS_DEPS), (CS_SRC, CS_OUT, CS_DEPS), \
    (RH_SRC, RH_OUT, RH_DEPS) = LIBS

# -ffp-contract=off: Rust never fuses; every fused multiply-add in lbft_math.h is explicit.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unused-value"]


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build the HIP library (there is no CPU fallback)")


def kernel_hash(so_path=None):
    """sha256 (16 hex digits) of the gfx950 code object inside the built library: profiles/current/pmc_traffic.json is stamped
    with it, and bench.py only reports that traffic while the stamp matches the kernels it is running (host-side edits of the C
    ABI do not change it; any kernel edit does).  Pure-Python ELF / offload-bundle parsing: no binutils needed on the GPU box."""
    import hashlib
    import struct
    blob = open(so_path or OUT, "rb").read()
    assert blob[:4] == b"\x7fELF" and blob[4] == 2, "not a 64-bit ELF"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", blob, 0x3A)

    def section(i):
        name, _type, _flags, _addr, off, size = struct.unpack_from("<IIQQQQ", blob, shoff + i * shentsize)
        return name, off, size
    _, stroff, strsize = section(shstrndx)
    strtab = blob[stroff:stroff + strsize]
    fat = None
    for i in range(shnum):
        name, off, size = section(i)
        if strtab[name:strtab.index(b"\0", name)] == b".hip_fatbin":
            fat = blob[off:off + size]
    assert fat is not None and fat.startswith(b"__CLANG_OFFLOAD_BUNDLE__"), "no offload bundle in the library"
    n, = struct.unpack_from("<Q", fat, 24)
    pos = 32
    for _ in range(n):
        o, sz, ts = struct.unpack_from("<QQQ", fat, pos)
        pos += 24
        triple = fat[pos:pos + ts].decode()
        pos += ts
        if "gfx950" in triple:
            co = fat[o:o + sz]
            # the machine code only (.text of the code object): the object as a whole also carries a per-translation-unit id
            # (__hip_cuid_*) that changes with any edit of the file, host code included
            cshoff, = struct.unpack_from("<Q", co, 0x28)
            centsize, cnum, cstrndx = struct.unpack_from("<HHH", co, 0x3A)

            def csection(i):
                name, _type, _flags, _addr, off, size = struct.unpack_from("<IIQQQQ", co, cshoff + i * centsize)
                return name, off, size
            _, cstroff, cstrsize = csection(cstrndx)
            cstr = co[cstroff:cstroff + cstrsize]
            for i in range(cnum):
                name, off, size = csection(i)
                if cstr[name:cstr.index(b"\0", name)] == b".text":
                    return hashlib.sha256(co[off:off + size]).hexdigest()[:16]
            raise RuntimeError("code object without .text")
    raise RuntimeError("no gfx950 code object in the library")


def source_hash():
    """(kept as the stamp's name in profiles/ and bench.py) = kernel_hash() of the built library."""
    return kernel_hash()


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def is_stale():
    return any(_stale(out, deps) for _src, out, deps in LIBS)


def build(force=False, verbose=False):
    """The libraries of TABLE, each with exactly HIPCC_FLAGS (they compile in parallel)."""
    jobs = [(src, out) for src, out, deps in LIBS if force or _stale(out, deps)]
    procs = []
    for src, out in jobs:
        cmd = [hipcc_path()] + HIPCC_FLAGS + [src, "-o", out]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
    failed = [cmd for cmd, proc in procs if proc.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])
    return OUT


def build_variant(tag, defines, verbose=False):
    """Diagnostic / tuning builds of the same sources (e.g. ("prof", ["-DLBFT_PHASE_TIMERS"])): written next to
    the product library as liblbft_hip_<tag>.so and selected with LBFT_HIP_LIB=<path>."""
    out = os.path.join(HERE, "liblbft_hip_%s.so" % tag)
    cmd = [hipcc_path()] + HIPCC_FLAGS + list(defines) + [SRC, "-o", out]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    print(build(force=True, verbose=True))
