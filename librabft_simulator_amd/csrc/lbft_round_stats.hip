// lbft_round_stats.hip -- the HIP kernel (gfx950) of lbft_batch_round_stats: per group (parameter set), the statistics of the round-switch
// trace (lbft_batch_enable_round_trace) -- how long nodes stay in a round, how many rounds they jump, how far apart the nodes of a network
// enter a round and how many of them enter it at all -- computed from the trace rows where they lie.
// Built as a library of its own (build.py), opened by liblbft_hip.so on first use: the code object of liblbft_hip.so, whose kernels are
// pinned byte for byte by the codegen manifest, does not change, and a traced batch loads no commit-time twins.
#include <hip/hip_runtime.h>

#include "../../include/lbft.h"
#include "lbft_core.h"
#include "lbft_round_stats.h"
#include "lbft_round_timeline.h"

using namespace lbft;

// One wavefront per instance, lane = round.  The kernel reads, through the generic Sim accessors (every layout: tile widths 1, lanes
// per wavefront, 64), the instance's fault word, max_round[n] and the cells first_time[n][rcap] below rows = min(max max_round, rcap).
//   node-major pass (stay, skipped): for each node, 64 rounds of its row at a time; a lane's nearest non-empty predecessor is the highest
//     set bit below it in the ballot of the non-empty lanes, its time comes by one shuffle, and the last non-empty cell of a chunk is
//     carried (wavefront-uniform) into the next one.
//   round-major pass (skew, reach): 64 rounds at a time, each lane walks the nodes of its round keeping earliest / latest / count in
//     registers; nothing is carried.  It reads the cells a second time, from L2.
// With tile width 1 a load instruction reads 256 contiguous bytes; with wider tiles consecutive rounds lie 4 * tw bytes apart and the
// neighbouring instances' wavefronts read the lines' other words.
// grid = (workgroups per group, groups); a workgroup's LBFT_RS_WAVES wavefronts stride over the instances of its group and accumulate
// by the scheme of lbft_group_stats.h: two LDS histograms, in passes of LBFT_RS_LDS_BINS bins.  Instances with a non-zero fault word are
// skipped.
#define LBFT_RS_BLOCK 256
#define LBFT_RS_WAVES (LBFT_RS_BLOCK / 64)
#define LBFT_RS_LDS_BINS 4096  // per histogram: 2 x 16 KiB of u32 counts
#define LBFT_RS_WORKGROUPS 1024u

__global__ __launch_bounds__(LBFT_RS_BLOCK) void lbft_k_rs_rounds(Params p, const u32* __restrict__ state, const u32* __restrict__ grp_inst,
                                                                  const u32* __restrict__ grp_off, u32 bin_width, u32 bins,
                                                                  unsigned long long* __restrict__ stay_hist,
                                                                  unsigned long long* __restrict__ skew_hist,
                                                                  unsigned long long* __restrict__ stats) {
  __shared__ u32 h_stay[LBFT_RS_LDS_BINS], h_skew[LBFT_RS_LDS_BINS];
  __shared__ unsigned long long s_stat[LBFT_ROUND_STATS];
  const u32 g = blockIdx.y;
  const uint2 grp = gs_group(grp_inst, grp_off, g, p.m);
  const u32 first = grp.x, cnt = grp.y;
  if (blockIdx.x * LBFT_RS_WAVES >= cnt) return;  // (the whole workgroup: its group has fewer instances)
  const u32 wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const u32 n = p.n, rcap = p.rcap, tr = p.off_trace;
  gs_stats_clear<LBFT_ROUND_STATS>(s_stat);
  GsStat st[RTL_FAMILIES] = {};
  for (u32 base = 0; base < bins; base += LBFT_RS_LDS_BINS) {
    const u32 span = bins - base < LBFT_RS_LDS_BINS ? bins - base : LBFT_RS_LDS_BINS;
    const bool stat_pass = base == 0;
    gs_lds_clear<LBFT_RS_BLOCK>(h_stay, span);
    gs_lds_clear<LBFT_RS_BLOCK>(h_skew, span);
    __syncthreads();
    for (u32 k = blockIdx.x * LBFT_RS_WAVES + wave; k < cnt; k += gridDim.x * LBFT_RS_WAVES) {  // (one instance per wavefront: uniform in it)
      const u32 i = gs_instance(grp_inst, first, k);
      Sim s(p, const_cast<u32*>(state), i);
      if (s.ld(I_FAULT) != 0) continue;
      u32 highest = 0;
      for (u32 j = lane; j < n; j += 64) {
        const u32 v = s.ld(tr + n * rcap + j);
        highest = v > highest ? v : highest;
      }
      for (int d = 32; d; d >>= 1) {
        const u32 o = (u32)__shfl_xor((int)highest, d, 64);
        highest = o > highest ? o : highest;
      }
      const u32 rows = rtl_rows(highest, rcap);
      for (u32 j = 0; j < n; j++) {  // node-major: stay, skipped
        u32 carry_r = LBFT_RTL_NO_ROUND, carry_t = 0;  // the last non-empty cell of the row's previous chunks
        for (u32 c0 = 0; c0 < rows; c0 += 64) {
          const u32 r = c0 + lane;
          const u32 t = rtl_cell(r < rows ? s.ld(tr + j * rcap + r) : LBFT_RTL_EMPTY, r, rows);
          const unsigned long long mask = __ballot(!rtl_empty(t));
          const unsigned long long below = mask & ((1ull << lane) - 1ull);
          const u32 pl = below ? 63u - (u32)__clzll((long long)below) : 0u;
          const u32 pt_chunk = (u32)__shfl((int)t, (int)pl, 64);
          const u32 pr = below ? c0 + pl : carry_r, pt = below ? pt_chunk : carry_t;
          u32 stay, skipped;
          if (rtl_pair(t, r, pt, pr, stay, skipped)) {
            gs_lds_count(h_stay, stay, bin_width, bins, base, span);
            if (stat_pass) { gs_stat_add(st[RTL_STAY], stay); gs_stat_add(st[RTL_SKIPPED], skipped); }
          }
          if (mask) {
            const u32 hl = 63u - (u32)__clzll((long long)mask);
            carry_r = c0 + hl;
            carry_t = (u32)__shfl((int)t, (int)hl, 64);
          }
        }
      }
      for (u32 c0 = 0; c0 < rows; c0 += 64) {  // round-major: skew, reach
        const u32 r = c0 + lane;
        RtlRound q = rtl_round_empty();
        if (r < rows)
          for (u32 j = 0; j < n; j++) rtl_round_add(q, s.ld(tr + j * rcap + r));
        u32 v;
        if (rtl_skew(q, r, rows, v)) {
          gs_lds_count(h_skew, v, bin_width, bins, base, span);
          if (stat_pass) gs_stat_add(st[RTL_SKEW], v);
        }
        if (stat_pass && rtl_reach(q, r, rows, v)) gs_stat_add(st[RTL_REACH], v);
      }
    }
    if (stat_pass) gs_reduce_to_lds<RTL_FAMILIES>(st, s_stat, lane == 0);
    __syncthreads();
    gs_lds_flush<LBFT_RS_BLOCK>(h_stay, stay_hist, g, bins, base, span);
    gs_lds_flush<LBFT_RS_BLOCK>(h_skew, skew_hist, g, bins, base, span);
    if (stat_pass) gs_stats_out<LBFT_ROUND_STATS>(s_stat, stats, g);
    __syncthreads();  // (before the next pass clears the histograms)
  }
}

extern "C" {

__attribute__((visibility("default"))) hipError_t lbft_rs_launch_rounds(const Params* p, const u32* state, const u32* grp_inst, const u32* grp_off,
                                                                       u32 n_groups, u32 max_group, u32 bin_width, u32 bins,
                                                                       unsigned long long* stay_hist, unsigned long long* skew_hist,
                                                                       unsigned long long* stats, hipStream_t stream) {
  if (bin_width == 0 || bins == 0 || n_groups == 0 || max_group == 0 || p->rcap == 0 || !stay_hist || !skew_hist || !stats) return hipErrorInvalidValue;
  // (an instance of the largest group gives at most n x rcap cells)
  const u64 gx = gs_workgroups(LBFT_RS_WORKGROUPS, n_groups, ((u64)max_group + LBFT_RS_WAVES - 1) / LBFT_RS_WAVES, (u64)max_group * p->n * p->rcap);
  lbft_k_rs_rounds<<<dim3((u32)gx, n_groups), LBFT_RS_BLOCK, 0, stream>>>(*p, state, grp_inst, grp_off, bin_width, bins, stay_hist, skew_hist, stats);
  return hipGetLastError();
}

}  // extern "C"
