// lbft_chain_stats.hip -- the HIP kernel (gfx950) of lbft_batch_chain_stats: per group (parameter set), the statistics of the
// committed chain -- the intervals between its blocks' proposals, its length, how far the nodes lag behind it, how long a leader keeps
// authoring it, whose blocks it holds, and the audit that every node's log is a prefix of it and that it is ordered in time --
// computed from what every run leaves in HBM: the commit logs, the block pool, the startup times and the fault words.  It asks nothing
// of the run: no commit-time twins, no round trace.
// Built as a library of its own (build.py), opened by liblbft_hip.so on first use: the code object of liblbft_hip.so, whose kernels are
// pinned byte for byte by the codegen manifest, does not change.
#include <hip/hip_runtime.h>

#include "../../include/lbft.h"
#include "lbft_core.h"
#include "lbft_chain_rules.h"
#include "lbft_chain_stats.h"

using namespace lbft;

#include "lbft_chain_walk.h"  // the workgroup prologue, the node pass, the proposal time, the predecessor by shuffle

// One wavefront per instance, walked with lbft_chain_walk.h.  The kernel reads, through the generic Sim accessors (every layout: tile
// widths 1, lanes per wavefront, 64), the instance's fault word, NF_NCOMMITS and NF_STARTUP of its nodes, the log rows log[n][lcap] and of
// the block records B_LINK and B_TIME.
//   node pass: each lane adds its nodes' lag samples L - nc_j.
//   chain pass (lane = entry, 64 at a time): b = log[ref][k], then the dependent gathers B_LINK, B_TIME and startup[author]; time and
//     author of the predecessor (cw_prev).  A lane that begins a run of its author finds the previous run start as the highest set bit
//     below it in the ballot of the run starts, or carried.
//   audit (inside the chain pass, the chunk's block ids in registers): the same 64 entries of every other node's row, compared below
//     that node's nc_j (<= L: the chain is the longest log).  The rows are read whether or not they are compared (k < L <= lcap: inside
//     the row), so the loads do not wait for the counts.
// With tile width 1 a load instruction of a row reads 256 contiguous bytes; with wider tiles consecutive entries lie 4 * tw bytes apart
// and the neighbouring instances' wavefronts read the lines' other words.  The block-record gathers are scattered in either layout:
// one chain's records are as many lines.
// grid = (workgroups per group, groups); a workgroup's LBFT_CS_WAVES wavefronts stride over the instances of its group and accumulate
// by the scheme of lbft_group_stats.h: two LDS histograms (the intervals in passes of LBFT_CS_LDS_BINS bins; the authors, at most
// LBFT_MAX_NODES of them, in the first pass), the statistics in registers in the first pass.  Instances with a non-zero fault word are
// skipped.
#define LBFT_CS_BLOCK 256
#define LBFT_CS_WAVES (LBFT_CS_BLOCK / 64)
#define LBFT_CS_LDS_BINS 4096  // the interval histogram: 16 KiB of u32 counts
#define LBFT_CS_WORKGROUPS 1024u
#define LBFT_CS_NODE_ROUNDS ((LBFT_MAX_NODES + 63) / 64)
static_assert(LBFT_CHAIN_STATS == CHN_FAMILIES * 4, "six families of (samples, sum, min, max)");

__global__ __launch_bounds__(LBFT_CS_BLOCK) void lbft_k_cs_chain(Params p, const u32* __restrict__ state, const u32* __restrict__ grp_inst,
                                                                 const u32* __restrict__ grp_off, u32 bin_width, u32 bins,
                                                                 unsigned long long* __restrict__ interval_hist,
                                                                 unsigned long long* __restrict__ author_blocks,
                                                                 unsigned long long* __restrict__ stats) {
  __shared__ u32 h_int[LBFT_CS_LDS_BINS], h_auth[LBFT_MAX_NODES];
  __shared__ unsigned long long s_stat[LBFT_CHAIN_STATS];
  CwGroup w;
  if (!cw_group_begin<LBFT_CS_WAVES>(w, p, grp_inst, grp_off)) return;
  const u32 g = w.g, first = w.first, cnt = w.cnt, wave = w.wave, lane = w.lane;
  const u32 n = p.n, lcap = p.lcap, lg = p.off_log;
  gs_stats_clear<LBFT_CHAIN_STATS>(s_stat);
  GsStat st[CHN_FAMILIES] = {};
  for (u32 base = 0; base < bins; base += LBFT_CS_LDS_BINS) {
    const u32 span = bins - base < LBFT_CS_LDS_BINS ? bins - base : LBFT_CS_LDS_BINS;
    const bool stat_pass = base == 0;
    gs_lds_clear<LBFT_CS_BLOCK>(h_int, span);
    if (stat_pass) gs_lds_clear<LBFT_CS_BLOCK>(h_auth, n);
    __syncthreads();
    for (u32 q = blockIdx.x * LBFT_CS_WAVES + wave; q < cnt; q += gridDim.x * LBFT_CS_WAVES) {  // (one instance per wavefront: uniform in it)
      const u32 i = gs_instance(grp_inst, first, q);
      Sim s(p, const_cast<u32*>(state), i);
      if (s.ld(I_FAULT) != 0) continue;
      // node pass
      u32 nc[LBFT_CS_NODE_ROUNDS];
      const CwChain ch = cw_chain_of(s, lane, n, lcap, 64u, nc);
      const u32 L = ch.L, ref = ch.ref;
      if (stat_pass) {
#pragma unroll
        for (u32 r = 0; r < LBFT_CS_NODE_ROUNDS; r++)
          if (r * 64 + lane < n) gs_stat_add(st[CHN_LAG], L - nc[r]);
      }
      // chain pass
      i32 carry_g = 0;
      u32 carry_a = 0, carry_start = 0;  // the last entry of the previous chunk; the index at which the run open at its end began
      u32 differing = 0, inversions = 0;
      for (u32 c0 = 0; c0 < L; c0 += 64) {
        const u32 k = c0 + lane;
        const bool have = k < L;
        u32 b = 0, a = 0;
        i32 gt = 0;
        if (have) {
          b = s.ld(lg + ref * lcap + k);
          a = s.blk_author(b);
          gt = cw_proposal(s, b, a);
        }
        const i32 pg = cw_prev(gt, carry_g, lane);
        const u32 pa = cw_prev(a, carry_a, lane);
        if (have && k > 0) {
          const u32 v = chn_interval(pg, gt);
          gs_lds_count(h_int, v, bin_width, bins, base, span);
          if (stat_pass) { gs_stat_add(st[CHN_INTERVAL], v); inversions += chn_inverted(pg, gt) ? 1u : 0u; }
        }
        if (!stat_pass) continue;
        const bool start = have && chn_run_start(k, a, pa);
        const unsigned long long starts = __ballot(start);
        if (start && k > 0) gs_stat_add(st[CHN_TENURE], chn_tenure(k, starts & ((1ull << lane) - 1ull), c0, carry_start));
        carry_start = chn_carry_start(starts, c0, carry_start);
        if (have) gs_lds_count(h_auth, a, 1u, n, 0u, n);
        for (u32 j = 0; j < n; j++) {  // audit
          if (j == ref) continue;
          const u32 ncj = chn_commits(s.nfm(j, NF_NCOMMITS), lcap);
          const u32 w = have ? s.ld(lg + j * lcap + k) : b;
          differing += (k < ncj && w != b) ? 1u : 0u;
        }
      }
      if (stat_pass) {
        for (int d = 32; d; d >>= 1) {
          differing += (u32)__shfl_xor((int)differing, d, 64);
          inversions += (u32)__shfl_xor((int)inversions, d, 64);
        }
        if (lane == 0) {  // one sample per instance; the run still open at the chain's end
          gs_stat_add(st[CHN_LENGTH], L);
          gs_stat_add(st[CHN_DIFFERING], differing);
          gs_stat_add(st[CHN_INVERSIONS], inversions);
          if (L) gs_stat_add(st[CHN_TENURE], L - carry_start);
        }
      }
    }
    if (stat_pass) gs_reduce_to_lds<CHN_FAMILIES>(st, s_stat, lane == 0);
    __syncthreads();
    gs_lds_flush<LBFT_CS_BLOCK>(h_int, interval_hist, g, bins, base, span);
    if (stat_pass) {
      gs_lds_flush<LBFT_CS_BLOCK>(h_auth, author_blocks, g, n, 0u, n);
      gs_stats_out<LBFT_CHAIN_STATS>(s_stat, stats, g);
    }
    __syncthreads();  // (before the next pass clears the histogram)
  }
}

extern "C" {

__attribute__((visibility("default"))) hipError_t lbft_cs_launch_chain(const Params* p, const u32* state, const u32* grp_inst, const u32* grp_off,
                                                                      u32 n_groups, u32 max_group, u32 bin_width, u32 bins,
                                                                      unsigned long long* interval_hist, unsigned long long* author_blocks,
                                                                      unsigned long long* stats, hipStream_t stream) {
  if (bin_width == 0 || bins == 0 || n_groups == 0 || max_group == 0 || p->n > LBFT_MAX_NODES || !interval_hist || !author_blocks || !stats)
    return hipErrorInvalidValue;
  // (an instance of the largest group gives at most lcap samples to a bin of the interval or author histogram, and n lag samples)
  const u64 per_instance = p->lcap > p->n ? p->lcap : p->n;
  const u64 gx = gs_workgroups(LBFT_CS_WORKGROUPS, n_groups, ((u64)max_group + LBFT_CS_WAVES - 1) / LBFT_CS_WAVES, (u64)max_group * per_instance);
  lbft_k_cs_chain<<<dim3((u32)gx, n_groups), LBFT_CS_BLOCK, 0, stream>>>(*p, state, grp_inst, grp_off, bin_width, bins, interval_hist, author_blocks, stats);
  return hipGetLastError();
}

}  // extern "C"
