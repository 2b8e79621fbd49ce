#!/usr/bin/env python3
"""Register budget of the run kernels and of the side libraries' kernels (the prefixes of build.TABLE) in a built library: VGPRs, SGPRs, spilled
registers, scratch and LDS bytes per kernel, read from
the AMDGPU metadata note of the gfx950 code object (no GPU needed).  The register-pressure work of DESIGN.md section 4 is
this loop: build one kernel class alone with a piece of source disabled (seconds instead of minutes)
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -DLBFT_DEV_ONLY_CLASS=7 [-D...] \\
          librabft_simulator_amd/csrc/lbft_hip.hip -o /tmp/dev7.so
    python tools/kernel_regs.py /tmp/dev7.so
and read what the piece costs; then measure the candidates on the GPU (tools/gpu_variants.sh).
    python tools/kernel_regs.py                      # the product library"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from test_abi import _kernel_metadata
    from librabft_simulator_amd import build
    # the run kernels and the side libraries' (build.TABLE); liblbft_paramsets.so's have never been listed, and listing them would change the output
    listed = ("lbft_k_run",) + tuple(lib.prefix for lib in build.TABLE if lib.prefix and lib.tag != "paramsets")
    libs = sys.argv[1:] or [build.OUT]
    for path in libs:
        for name, v in sorted(_kernel_metadata(path).items()):
            if any(prefix in name for prefix in listed) and v["vgpr_count"]:
                print("%-28s %-44s vgprs %3d  sgprs %3d  spilled %3d  scratch %4d B  lds %5d B" % (
                    os.path.basename(path), name[:44], v["vgpr_count"], v["sgpr_count"], v["vgpr_spill_count"], v["private_segment_fixed_size"],
                    v["group_segment_fixed_size"]))


if __name__ == "__main__":
    main()
