// lbft_commit_times.hip -- HIP kernels (gfx950) of batches that record commit times (lbft_batch_record_commit_times).
//
// The run kernels are the commit-time twins of the lane-private run kernels: lbft_core.h's step instantiated for K_SMALL / K_MID (and
// their K_PARAM_SETS forms) with K_COMMIT_TIMES added, where commit_block also stores the clock of every commit into the batch's
// commit-time buffer ([instance][node][lcap] i32, the log's index).  Their run body (lbft_lane_run.h) and LDS layout (lbft_launch.h) are
// those of lbft_k_run0 / lbft_k_run<1> and the parameter-set kernels, so the host side of liblbft_hip.so sizes them as those.
// The histogram kernel turns a finished run's logs and commit times into commit-latency histograms per group (parameter set).
// Built as a library of its own (build.py): the code object of liblbft_hip.so, whose kernels are pinned byte for byte by the codegen
// manifest, does not change.
#include <hip/hip_runtime.h>

#include "../../include/lbft.h"
#include "lbft_core.h"
#include "lbft_commit_times.h"

using namespace lbft;

#include "lbft_launch.h"
#include "lbft_lane_run.h"  // ps_run_body

// Small class (lbft_k_run0's geometry: two wavefronts per SIMD) and mid class (lbft_k_run<1>'s: one wavefront per SIMD, the whole register
// file), each plain and with parameter sets.
__global__ __launch_bounds__(LBFT_RUN_BLOCK) __attribute__((amdgpu_waves_per_eu(LBFT_RUN_WAVES_PER_SIMD, LBFT_RUN_WAVES_PER_SIMD)))
void lbft_k_ct_run0(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, i32* __restrict__ ctimes) {
  ps_run_body<K_SMALL_TIMED>(p, state, unfinished, nullptr, nullptr, ctimes);
}
__global__ __launch_bounds__(64 * LBFT_RUN_WAVES_FULL)
void lbft_k_ct_run1(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, i32* __restrict__ ctimes) {
  ps_run_body<K_MID_TIMED>(p, state, unfinished, nullptr, nullptr, ctimes);
}
__global__ __launch_bounds__(LBFT_RUN_BLOCK) __attribute__((amdgpu_waves_per_eu(LBFT_RUN_WAVES_PER_SIMD, LBFT_RUN_WAVES_PER_SIMD)))
void lbft_k_ct_ps_run0(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of,
                       i32* __restrict__ ctimes) {
  ps_run_body<K_SMALL_SETS_TIMED>(p, state, unfinished, sets, set_of, ctimes);
}
__global__ __launch_bounds__(64 * LBFT_RUN_WAVES_FULL)
void lbft_k_ct_ps_run1(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of,
                       i32* __restrict__ ctimes) {
  ps_run_body<K_MID_SETS_TIMED>(p, state, unfinished, sets, set_of, ctimes);
}

// Commit-latency histogram: grid = (lanes of the largest group / LBFT_HIST_BLOCK, groups); one lane per (instance, node) of the
// workgroup's group walks the node's log -- block id -> author (B_LINK) and proposer time (B_TIME), the author's startup time, the commit
// time -- and bins latency = commit time - (startup[author] + block time) into the workgroup's LDS histogram with integer atomics.  The
// LDS histogram is then added into the group's global one, one atomic per non-zero bin per workgroup; samples / sum / min / max likewise
// (once per workgroup).  Histograms wider than LBFT_HIST_LDS_BINS are binned in passes of that many bins.  Instances with a non-zero
// fault word are skipped.  Every accumulation is an integer add / max: the result does not depend on the order of the atomics.
#define LBFT_HIST_BLOCK 256
#define LBFT_HIST_LDS_BINS 8192  // 32 KiB of u32 counts (a workgroup counts at most 256 lanes x lcap <= 65 534 samples: no overflow)
__global__ __launch_bounds__(LBFT_HIST_BLOCK) void lbft_k_ct_latency_hist(Params p, const u32* __restrict__ state, const i32* __restrict__ ctimes,
                                                                          const u32* __restrict__ grp_inst, const u32* __restrict__ grp_off,
                                                                          u32 bin_width, u32 bins, unsigned long long* __restrict__ hist,
                                                                          unsigned long long* __restrict__ stats) {
  __shared__ u32 h[LBFT_HIST_LDS_BINS];
  __shared__ unsigned long long s_cnt, s_sum, s_nmin, s_max;
  const u32 g = blockIdx.y;
  const u32 first = grp_inst ? grp_off[g] : 0u, cnt = grp_inst ? grp_off[g + 1] - first : p.m;
  const u32 lanes = cnt * p.n;  // (< 2^31: lbft_batch_create bounds instances x nodes)
  if (blockIdx.x * LBFT_HIST_BLOCK >= lanes) return;  // (the whole workgroup: its group has fewer lanes)
  const u32 t = blockIdx.x * LBFT_HIST_BLOCK + threadIdx.x;
  u32 node = 0, i = grp_inst ? grp_inst[first] : 0u, nc = 0;
  if (t < lanes) {
    node = t / cnt;  // consecutive lanes -> consecutive instances of one node
    i = grp_inst ? grp_inst[first + t % cnt] : t % cnt;
  }
  Sim s(p, const_cast<u32*>(state), i);
  if (t < lanes && s.ld(I_FAULT) == 0) nc = s.nfm(node, NF_NCOMMITS);
  if (nc > p.lcap) nc = p.lcap;
  const i32* ct = ctimes + ((size_t)i * p.n + node) * p.lcap;
  if (threadIdx.x == 0) { s_cnt = 0; s_sum = 0; s_nmin = 0; s_max = 0; }
  for (u32 base = 0; base < bins; base += LBFT_HIST_LDS_BINS) {
    const u32 span = bins - base < LBFT_HIST_LDS_BINS ? bins - base : LBFT_HIST_LDS_BINS;
    for (u32 k = threadIdx.x; k < span; k += LBFT_HIST_BLOCK) h[k] = 0;
    __syncthreads();
    unsigned long long cnt_l = 0, sum_l = 0, nmin_l = 0, max_l = 0;
    for (u32 k = 0; k < nc; k++) {
      const i32 c = ct[k];
      if (c < 0) continue;  // (not recorded)
      const u32 b = s.ld(p.off_log + node * p.lcap + k);
      const u32 a = s.blk_author(b);
      const i64 lat = (i64)c - ((i64)(i32)s.nfm(a, NF_STARTUP) + (i64)(i32)s.bf(b, B_TIME));  // in [0, max_clock]
      const u64 l = (u64)lat;
      const u64 q = l / bin_width;
      const u32 bin = q < bins - 1u ? (u32)q : bins - 1u;
      if (bin >= base && bin - base < span) atomicAdd(&h[bin - base], 1u);
      cnt_l++; sum_l += l;
      nmin_l = ~l > nmin_l ? ~l : nmin_l;
      max_l = l > max_l ? l : max_l;
    }
    if (base == 0 && cnt_l) { atomicAdd(&s_cnt, cnt_l); atomicAdd(&s_sum, sum_l); atomicMax(&s_nmin, nmin_l); atomicMax(&s_max, max_l); }
    __syncthreads();
    for (u32 k = threadIdx.x; k < span; k += LBFT_HIST_BLOCK)
      if (h[k]) atomicAdd(&hist[(size_t)g * bins + base + k], (unsigned long long)h[k]);
    if (base == 0 && threadIdx.x == 0 && s_cnt) {
      atomicAdd(&stats[g * 4 + 0], s_cnt); atomicAdd(&stats[g * 4 + 1], s_sum);
      atomicMax(&stats[g * 4 + 2], s_nmin); atomicMax(&stats[g * 4 + 3], s_max);
    }
    __syncthreads();  // (before the next pass clears h)
  }
}

extern "C" {

__attribute__((visibility("default"))) hipError_t lbft_ct_launch_run(int cls, const Params* p, u32* state, u32* unfinished, const ParamSetDev* sets,
                                                                    const u8* set_of, i32* ctimes, u32 grid, u32 block, size_t lds_bytes,
                                                                    hipStream_t stream) {
  if (cls != K_SMALL && cls != K_MID) return hipErrorInvalidValue;
  const void* fn = sets ? (cls == K_SMALL ? reinterpret_cast<const void*>(lbft_k_ct_ps_run0) : reinterpret_cast<const void*>(lbft_k_ct_ps_run1))
                        : (cls == K_SMALL ? reinterpret_cast<const void*>(lbft_k_ct_run0) : reinterpret_cast<const void*>(lbft_k_ct_run1));
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return e;
  if (sets && cls == K_SMALL) lbft_k_ct_ps_run0<<<grid, block, lds_bytes, stream>>>(*p, state, unfinished, sets, set_of, ctimes);
  else if (sets) lbft_k_ct_ps_run1<<<grid, block, lds_bytes, stream>>>(*p, state, unfinished, sets, set_of, ctimes);
  else if (cls == K_SMALL) lbft_k_ct_run0<<<grid, block, lds_bytes, stream>>>(*p, state, unfinished, ctimes);
  else lbft_k_ct_run1<<<grid, block, lds_bytes, stream>>>(*p, state, unfinished, ctimes);
  return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t lbft_ct_launch_histogram(const Params* p, const u32* state, const i32* ctimes, const u32* grp_inst,
                                                                          const u32* grp_off, u32 n_groups, u32 max_group, u32 bin_width, u32 bins,
                                                                          unsigned long long* hist, unsigned long long* stats, hipStream_t stream) {
  if (bin_width == 0 || bins == 0 || n_groups == 0 || max_group == 0) return hipErrorInvalidValue;
  const u32 gx = (u32)(((u64)max_group * p->n + LBFT_HIST_BLOCK - 1) / LBFT_HIST_BLOCK);
  lbft_k_ct_latency_hist<<<dim3(gx, n_groups), LBFT_HIST_BLOCK, 0, stream>>>(*p, state, ctimes, grp_inst, grp_off, bin_width, bins, hist, stats);
  return hipGetLastError();
}

}  // extern "C"
