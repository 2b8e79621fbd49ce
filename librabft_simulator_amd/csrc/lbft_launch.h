// lbft_launch.h -- launch geometry and LDS layout of the run kernels (their body: lbft_run_body.h) and the host's launch of one, shared by
// liblbft_hip.so (lbft_hip.hip), the parameter-set kernels of liblbft_paramsets.so (lbft_paramsets.hip) and the commit-time kernels of
// liblbft_commit_times.so (lbft_commit_times.hip), so that the host code of the first sizes the LDS of all three alike.
#ifndef LBFT_LAUNCH_H
#define LBFT_LAUNCH_H
#define LBFT_BLOCK 64  // one wavefront per workgroup: wavefronts retire independently

// Simulator::loop_until for every instance (simulator.rs:380-475).
//
// Workgroup = LBFT_RUN_WAVES (8) wavefronts = both wavefront slots of a CU's four SIMDs (256 registers per lane: two per SIMD);
// wavefront w of workgroup g advances instances [(g * 8 + w) * lpw, +lpw).  LDS (dynamic, up to the CU's whole 160 KiB):
//   [zig_x 257][zig_f 257][exp_tab 256]  u64   read-only tables of the delay sampler, one copy per workgroup
//   [dur 128] i64, [leader 1024] u8            pacemaker duration / leader tables (first rounds)
//   keys  [wave][slot][lane]              u64   event-queue keys, lane-private columns: class 0 one packed word per event
//                                               (time | 3-kind | stamp | node | sender | slot), other classes (time, 3-kind, stamp)
//   metas [wave][slot][lane]              u32   classes 1-2 only: (node, sender, snapshot slot)
//   [diagnostic phase counters], then      --   n > 16: one 128-byte receiver list per instance; class 0 with n <= 4: the nodes'
//                                               hcbr buffers, 32 words per instance ([wave][word][lane])
// A lane only ever touches its own column (address = slot * lpw + lane), so data-dependent slot
// indices are bank-conflict free and no workgroup barrier is needed after the table fill.
// (round 3: 8 instead of 4.  Equal for every batch that fills the chip -- 65 536 x 4: 21.61 vs 21.67 ms, 32 768: 18.4 vs 18.6, 16 384: 15.7 vs
// 15.5 -- but a batch of <= 1 024 networks then packs two wavefronts on every SIMD of half the CUs instead of one on each SIMD of all
// of them, and a wavefront that shares its SIMD runs FASTER per step (phase timers, one network per wavefront: 13.2 k cycles per step
// with a partner, 17.3 k alone): 1 024 x 4 nodes 9.8 -> 7.0 ms.)
#ifndef LBFT_RUN_WAVES
#define LBFT_RUN_WAVES 8
#endif
#define LBFT_RUN_BLOCK (64 * LBFT_RUN_WAVES)
#define LBFT_RUN_WAVES_FULL 4  // the kernels that use the whole register file (lbft_k_run<1>, <2>): one wavefront per SIMD = 4 per workgroup
                               // (a 512-thread launch bound would cap them at 256 registers)
#define LBFT_LDS_HCBR_WORDS 32  // class 0, n <= 4: hcbr[node][2][4] per instance
#ifndef LBFT_PACKED_QL_MAX
#define LBFT_PACKED_QL_MAX 64  // LDS slots per instance of the packed (class 0) queue: the 4-node bench workload peaks at 53 pending events
#endif
#define LBFT_LDS_LEADERS 1024  // rounds of the leader table kept in LDS (bytes)
#define LBFT_LDS_DURS 128      // entries of the duration table kept in LDS (i64)
#define LBFT_LDS_WEIGHTS LBFT_MAX_NODES  // voting rights (u32)
#define LBFT_TABLE_U64 (257 + 257 + 256 + LBFT_LDS_DURS + LBFT_LDS_LEADERS / 8 + LBFT_LDS_WEIGHTS / 2)

// (the host's sizing of this layout: run_lds_bytes, lbft_plan.h)
#if defined(__HIPCC__)
__device__ __forceinline__ size_t run_lds_bytes_dev(u32 ql, u32 lpw, u32 slot_bytes, u32 nwaves) {  // = run_lds_bytes(ql, lpw, 0, ..): where the receiver lists start
  return (size_t)LBFT_TABLE_U64 * 8 + (size_t)nwaves * ql * lpw * slot_bytes + (size_t)nwaves * LBFT_NPHASES * 8 + 8;
}
// One launch of run kernel `kernel` with `lds_bytes` of dynamic LDS (more than the default limit: the attribute is set first)
template <typename... KArgs, typename... Args>
inline hipError_t launch_run_kernel(void (*kernel)(KArgs...), u32 grid, u32 block, size_t lds_bytes, hipStream_t stream, const Args&... args) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return e;
  kernel<<<grid, block, lds_bytes, stream>>>(args...);
  return hipGetLastError();
}
#endif
#ifndef LBFT_RUN_WAVES_PER_SIMD
#define LBFT_RUN_WAVES_PER_SIMD 2  // register budget of the class-0 run kernel: 512 / 2 = 256 VGPRs + AGPRs per lane (the
                                   // large-network classes run one 8- or 16-lane wavefront per SIMD and may use all 512)
#endif
// the launch bounds of a run kernel compiled for two wavefronts per SIMD (lbft_plan.h's table of run kernels says which are)
#define LBFT_TWO_WAVE_BOUNDS __launch_bounds__(LBFT_RUN_BLOCK) __attribute__((amdgpu_waves_per_eu(LBFT_RUN_WAVES_PER_SIMD, LBFT_RUN_WAVES_PER_SIMD)))
#ifndef LBFT_BIG_WAVES_PER_SIMD
#define LBFT_BIG_WAVES_PER_SIMD 1  // classes 1-2: wavefronts per SIMD the kernels are compiled for (1 = the whole register file;
                                   // measured with 2 -- half the lanes per wavefront, 167 spilled registers: 16384 x 64 nodes
                                   // 1.23 s instead of 1.01 s, 8192 x 100 nodes 7.0 s instead of 5.5 s)
#endif
#endif  // LBFT_LAUNCH_H
