// lbft_commit_times.hip -- HIP kernels (gfx950) of batches that record commit times (lbft_batch_record_commit_times).
//
// The run kernels are the commit-time twins of the lane-private run kernels: lbft_core.h's step instantiated for K_SMALL / K_MID (and
// their K_PARAM_SETS forms) with K_COMMIT_TIMES added, where commit_block also stores the clock of every commit into the batch's
// commit-time buffer ([instance][node][lcap] i32, the log's index).  Their run body (lbft_run_body.h) and LDS layout (lbft_launch.h) are
// those of lbft_k_run0 / lbft_k_run<1> and the parameter-set kernels, so the host side of liblbft_hip.so sizes them as those.
// The histogram kernel turns a finished run's logs and commit times into commit-latency histograms per group (parameter set); the
// timeline kernel turns the commit times alone into commits over time and the statistics of the commit-free intervals.
// Built as a library of its own (build.py): the code object of liblbft_hip.so, whose kernels are pinned byte for byte by the codegen
// manifest, does not change.
#include <hip/hip_runtime.h>

#include "../../include/lbft.h"
#include "lbft_core.h"
#include "lbft_commit_times.h"
#include "lbft_commit_timeline.h"

using namespace lbft;

#include "lbft_launch.h"
#include "lbft_run_body.h"  // run_body

// Small class (lbft_k_run0's geometry: two wavefronts per SIMD) and mid class (lbft_k_run<1>'s: one wavefront per SIMD, the whole register
// file), each plain and with parameter sets.
__global__ LBFT_TWO_WAVE_BOUNDS void lbft_k_ct_run0(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, i32* __restrict__ ctimes) {
  run_body<K_SMALL_TIMED>(p, state, unfinished, nullptr, nullptr, ctimes);
}
__global__ __launch_bounds__(64 * LBFT_RUN_WAVES_FULL)
void lbft_k_ct_run1(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, i32* __restrict__ ctimes) {
  run_body<K_MID_TIMED>(p, state, unfinished, nullptr, nullptr, ctimes);
}
__global__ LBFT_TWO_WAVE_BOUNDS void lbft_k_ct_ps_run0(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of,
                       i32* __restrict__ ctimes) {
  run_body<K_SMALL_SETS_TIMED>(p, state, unfinished, sets, set_of, ctimes);
}
__global__ __launch_bounds__(64 * LBFT_RUN_WAVES_FULL)
void lbft_k_ct_ps_run1(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of,
                       i32* __restrict__ ctimes) {
  run_body<K_MID_SETS_TIMED>(p, state, unfinished, sets, set_of, ctimes);
}

// Commit-latency histogram: grid = (lanes of the largest group / LBFT_HIST_BLOCK, groups); one lane per (instance, node) of the
// workgroup's group walks the node's log -- block id -> author (B_LINK) and proposer time (B_TIME), the author's startup time, the commit
// time -- and accumulates latency = commit time - (startup[author] + block time) by the scheme of lbft_group_stats.h: the workgroup's LDS
// histogram in passes of LBFT_HIST_LDS_BINS bins, samples / sum / min / max in registers, then wavefront, LDS and one global atomic each
// per workgroup.  Instances with a non-zero fault word are skipped.
#define LBFT_HIST_BLOCK 256
#define LBFT_HIST_LDS_BINS 8192  // 32 KiB of u32 counts (a workgroup counts at most 256 lanes x lcap <= 65 534 samples: no overflow)
__global__ __launch_bounds__(LBFT_HIST_BLOCK) void lbft_k_ct_latency_hist(Params p, const u32* __restrict__ state, const i32* __restrict__ ctimes,
                                                                          const u32* __restrict__ grp_inst, const u32* __restrict__ grp_off,
                                                                          u32 bin_width, u32 bins, unsigned long long* __restrict__ hist,
                                                                          unsigned long long* __restrict__ stats) {
  __shared__ u32 h[LBFT_HIST_LDS_BINS];
  __shared__ unsigned long long s_stat[4];
  const u32 g = blockIdx.y;
  const uint2 grp = gs_group(grp_inst, grp_off, g, p.m);
  const u32 first = grp.x, cnt = grp.y;
  const u32 lanes = cnt * p.n;  // (< 2^31: lbft_batch_create bounds instances x nodes)
  if (blockIdx.x * LBFT_HIST_BLOCK >= lanes) return;  // (the whole workgroup: its group has fewer lanes)
  const u32 t = blockIdx.x * LBFT_HIST_BLOCK + threadIdx.x;
  u32 node = 0, i = gs_instance(grp_inst, first, 0), nc = 0;
  if (t < lanes) {
    node = t / cnt;  // consecutive lanes -> consecutive instances of one node
    i = gs_instance(grp_inst, first, t % cnt);
  }
  Sim s(p, const_cast<u32*>(state), i);
  if (t < lanes && s.ld(I_FAULT) == 0) nc = s.nfm(node, NF_NCOMMITS);
  if (nc > p.lcap) nc = p.lcap;
  const i32* ct = ctimes + ((size_t)i * p.n + node) * p.lcap;
  gs_stats_clear<4>(s_stat);
  GsStat st = {};
  for (u32 base = 0; base < bins; base += LBFT_HIST_LDS_BINS) {
    const u32 span = bins - base < LBFT_HIST_LDS_BINS ? bins - base : LBFT_HIST_LDS_BINS;
    gs_lds_clear<LBFT_HIST_BLOCK>(h, span);
    __syncthreads();
    for (u32 k = 0; k < nc; k++) {
      const i32 c = ct[k];
      if (c < 0) continue;  // (not recorded)
      const u32 b = s.ld(p.off_log + node * p.lcap + k);
      const u32 a = s.blk_author(b);
      const i64 lat = (i64)c - ((i64)(i32)s.nfm(a, NF_STARTUP) + (i64)(i32)s.bf(b, B_TIME));  // in [0, max_clock]
      const u32 l = (u32)lat;  // (max_clock < 2^31: nothing is cut off)
      gs_lds_count(h, l, bin_width, bins, base, span);
      if (base == 0) gs_stat_add(st, l);
    }
    if (base == 0) gs_reduce_to_lds<1>(&st, s_stat, threadIdx.x % 64 == 0);
    __syncthreads();
    gs_lds_flush<LBFT_HIST_BLOCK>(h, hist, g, bins, base, span);
    if (base == 0) gs_stats_out<4>(s_stat, stats, g);
    __syncthreads();  // (before the next pass clears h)
  }
}

// Commit timelines (lbft_batch_commit_series / lbft_batch_commit_stalls): the commit-time rows alone -- no log, no block pool.  A row
// (one node of one instance, lcap i32) is read by a segment of LBFT_TL_SEG consecutive lanes, entry k by lane k % LBFT_TL_SEG, so a
// load instruction of a wavefront reads two runs of 128 contiguous bytes, not 64 lines (lbft_k_ct_latency_hist's lane per row), and
// only the nc recorded entries of a row are read.  A lane takes its predecessor's entry by __shfl_up -- lane 0 of the segment the last
// entry of the row's previous chunk -- and lbft_commit_timeline.h turns (entry, predecessor) into samples; the per-row quantities
// (longest interval, last instant, first instant at or after `since`) are segment reductions by __shfl_xor.
// grid = (workgroups per group, groups); a workgroup strides over the rows of its group, LBFT_TL_ROWS at a time, and accumulates by
// the scheme of lbft_group_stats.h, in passes of LBFT_HIST_LDS_BINS bins.
// stalls == 0: the series (one sample per entry: its commit time; no statistics).  stalls != 0: the gap histogram and
// stats[group * 16 + family * 4 + {samples, sum, ~min, max}].  Instances with a non-zero fault word are skipped.
#define LBFT_TL_BLOCK 256
#define LBFT_TL_SEG 32
#define LBFT_TL_ROWS (LBFT_TL_BLOCK / LBFT_TL_SEG)
#ifndef LBFT_TL_WORKGROUPS  // (a tuning build may set it: EXPERIMENTS.md "Commit timelines")
#define LBFT_TL_WORKGROUPS 1024u
#endif
__global__ __launch_bounds__(LBFT_TL_BLOCK) void lbft_k_ct_timeline(Params p, const u32* __restrict__ state, const i32* __restrict__ ctimes,
                                                                    const u32* __restrict__ grp_inst, const u32* __restrict__ grp_off, int stalls,
                                                                    const i32* __restrict__ since_of, u32 bin_width, u32 bins,
                                                                    unsigned long long* __restrict__ hist, unsigned long long* __restrict__ stats) {
  __shared__ u32 h[LBFT_HIST_LDS_BINS];
  __shared__ unsigned long long s_stat[LBFT_STALL_STATS];
  const u32 g = blockIdx.y;
  const uint2 grp = gs_group(grp_inst, grp_off, g, p.m);
  const u32 first = grp.x, cnt = grp.y;
  const u32 rows = cnt * p.n;  // (< 2^31: lbft_batch_create bounds instances x nodes)
  if (blockIdx.x * LBFT_TL_ROWS >= rows) return;  // (the whole workgroup: its group has fewer rows)
  const u32 seg = threadIdx.x / LBFT_TL_SEG, k0 = threadIdx.x % LBFT_TL_SEG;
  const i32 since = since_of ? since_of[g] : 0;
  gs_stats_clear<LBFT_STALL_STATS>(s_stat);
  GsStat st[CTL_FAMILIES] = {};
  for (u32 base = 0; base < bins; base += LBFT_HIST_LDS_BINS) {
    const u32 span = bins - base < LBFT_HIST_LDS_BINS ? bins - base : LBFT_HIST_LDS_BINS;
    gs_lds_clear<LBFT_TL_BLOCK>(h, span);
    __syncthreads();
    // What a row starts from -- its first chunk, the instance's fault word, the node's commit count -- is loaded one row ahead, all
    // three together (none waits for another), and most rows are one chunk: the loads of the next row are in flight while this one is
    // turned into samples.
    const u32 stride = gridDim.x * LBFT_TL_ROWS;
    const i32* ct_next = nullptr;
    i32 head_next = -1;
    u32 fault_next = 1, nc_next = 0;
    auto fetch = [&](u32 r) {
      const u32 node = r % p.n, i = gs_instance(grp_inst, first, r / p.n);
      ct_next = ctimes + ((size_t)i * p.n + node) * p.lcap;
      head_next = k0 < p.lcap ? ct_next[k0] : -1;
      Sim s(p, const_cast<u32*>(state), i);
      fault_next = s.ld(I_FAULT);
      nc_next = s.nfm(node, NF_NCOMMITS);
    };
    u32 r = blockIdx.x * LBFT_TL_ROWS + seg;  // (one row per segment: uniform in it)
    if (r < rows) fetch(r);
    for (; r < rows; r += stride) {
      const i32* ct = ct_next;
      const i32 head = head_next;
      const u32 fault = fault_next;
      const u32 nc = nc_next < p.lcap ? nc_next : p.lcap;
      if (r + stride < rows) fetch(r + stride);
      if (fault != 0) continue;
      CtlRow row = ctl_empty();
      i32 carry = -1;  // the last entry of the row's previous chunk
      for (u32 c0 = 0; c0 < nc; c0 += LBFT_TL_SEG) {
        const i32 c = c0 + k0 >= nc ? -1 : c0 ? ct[c0 + k0] : head;
        i32 prev = __shfl_up(c, 1, LBFT_TL_SEG);
        if (k0 == 0) prev = carry;
        carry = __shfl(c, LBFT_TL_SEG - 1, LBFT_TL_SEG);
        u32 sample = 0;
        bool have = false;
        if (stalls) { sample = ctl_entry(row, c, prev, since); have = sample != 0; }
        else { sample = (u32)c; have = c >= 0; }
        if (have) {
          gs_lds_count(h, sample, bin_width, bins, base, span);
          if (stalls && base == 0) gs_stat_add(st[CTL_GAPS], sample);
        }
      }
      if (stalls && base == 0) {
        for (u32 d = LBFT_TL_SEG / 2; d; d >>= 1) {
          CtlRow o;
          o.longest = (u32)__shfl_xor((int)row.longest, (int)d, LBFT_TL_SEG);
          o.last = __shfl_xor(row.last, (int)d, LBFT_TL_SEG);
          o.first = (u32)__shfl_xor((int)row.first, (int)d, LBFT_TL_SEG);
          row = ctl_merge(row, o);
        }
        if (k0 == 0) {  // one sample per node
          if (row.first != LBFT_CTL_NONE) gs_stat_add(st[CTL_FIRST], row.first);
          gs_stat_add(st[CTL_TAIL], ctl_tail(row, p.max_clock));
          gs_stat_add(st[CTL_LONGEST], ctl_longest(row, p.max_clock));
        }
      }
    }
    if (stalls && base == 0) gs_reduce_to_lds<CTL_FAMILIES>(st, s_stat, threadIdx.x % 64 == 0);
    __syncthreads();
    gs_lds_flush<LBFT_TL_BLOCK>(h, hist, g, bins, base, span);
    if (stalls && base == 0) gs_stats_out<LBFT_STALL_STATS>(s_stat, stats, g);
    __syncthreads();  // (before the next pass clears h)
  }
}

extern "C" {

__attribute__((visibility("default"))) hipError_t lbft_ct_launch_run(int cls, const Params* p, u32* state, u32* unfinished, const ParamSetDev* sets,
                                                                    const u8* set_of, i32* ctimes, u32 grid, u32 block, size_t lds_bytes,
                                                                    hipStream_t stream) {
  if (cls != K_SMALL && cls != K_MID) return hipErrorInvalidValue;
  if (sets)
    return launch_run_kernel(cls == K_SMALL ? lbft_k_ct_ps_run0 : lbft_k_ct_ps_run1, grid, block, lds_bytes, stream, *p, state, unfinished, sets, set_of,
                             ctimes);
  return launch_run_kernel(cls == K_SMALL ? lbft_k_ct_run0 : lbft_k_ct_run1, grid, block, lds_bytes, stream, *p, state, unfinished, ctimes);
}

__attribute__((visibility("default"))) hipError_t lbft_ct_launch_histogram(const Params* p, const u32* state, const i32* ctimes, const u32* grp_inst,
                                                                          const u32* grp_off, u32 n_groups, u32 max_group, u32 bin_width, u32 bins,
                                                                          unsigned long long* hist, unsigned long long* stats, hipStream_t stream) {
  if (bin_width == 0 || bins == 0 || n_groups == 0 || max_group == 0) return hipErrorInvalidValue;
  const u32 gx = (u32)(((u64)max_group * p->n + LBFT_HIST_BLOCK - 1) / LBFT_HIST_BLOCK);
  lbft_k_ct_latency_hist<<<dim3(gx, n_groups), LBFT_HIST_BLOCK, 0, stream>>>(*p, state, ctimes, grp_inst, grp_off, bin_width, bins, hist, stats);
  return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t lbft_ct_launch_timeline(const Params* p, const u32* state, const i32* ctimes, const u32* grp_inst,
                                                                         const u32* grp_off, u32 n_groups, u32 max_group, int stalls,
                                                                         const i32* since_of, u32 bin_width, u32 bins, unsigned long long* hist,
                                                                         unsigned long long* stats, hipStream_t stream) {
  if (bin_width == 0 || bins == 0 || n_groups == 0 || max_group == 0 || (stalls && !stats)) return hipErrorInvalidValue;
  const u64 rows = (u64)max_group * p->n;  // of the largest group; a row gives at most lcap samples
  const u64 gx = gs_workgroups(LBFT_TL_WORKGROUPS, n_groups, (rows + LBFT_TL_ROWS - 1) / LBFT_TL_ROWS, rows * p->lcap);
  lbft_k_ct_timeline<<<dim3((u32)gx, n_groups), LBFT_TL_BLOCK, 0, stream>>>(*p, state, ctimes, grp_inst, grp_off, stalls, since_of, bin_width, bins, hist,
                                                                          stats);
  return hipGetLastError();
}

}  // extern "C"
