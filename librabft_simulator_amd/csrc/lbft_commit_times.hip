// lbft_commit_times.hip -- HIP kernels (gfx950) of batches that record commit times (lbft_batch_record_commit_times).
//
// The run kernels are the commit-time twins of the lane-private run kernels: lbft_core.h's step instantiated for K_SMALL / K_MID (and
// their K_PARAM_SETS forms) with K_COMMIT_TIMES added, where commit_block also stores the clock of every commit into the batch's
// commit-time buffer ([instance][node][lcap] i32, the log's index).  Their run body (lbft_run_body.h) and LDS layout (lbft_launch.h) are
// those of lbft_k_run0 / lbft_k_run<1> and the parameter-set kernels, so the host side of liblbft_hip.so sizes them as those.
// The histogram kernel turns a finished run's logs and commit times into commit-latency histograms per group (parameter set); the
// timeline kernel turns the commit times alone into commits over time and the statistics of the commit-free intervals; the finality
// kernel looks across the nodes of every chain entry: when the first node, a quorum of the voting rights and every node committed it;
// the instance kernel takes the samples of all three and keeps them per instance (lbft_batch_instance_stats); the phase kernel splits
// the latency and the finality by the phase of an entry's proposal time (lbft_batch_commit_phases).
// Built as a library of its own (build.py): the code object of liblbft_hip.so, whose kernels are pinned byte for byte by the codegen
// manifest, does not change.
#include <hip/hip_runtime.h>

#include "../../include/lbft.h"
#include "lbft_core.h"
#include "lbft_commit_times.h"
#include "lbft_commit_timeline.h"
#include "lbft_chain_rules.h"
#include "lbft_commit_finality.h"
#include "lbft_instance_stats.h"
#include "lbft_commit_phases.h"

using namespace lbft;

#include "lbft_launch.h"
#include "lbft_run_body.h"  // run_body
#include "lbft_chain_walk.h"

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
      const u32 l = fin_after(c, cw_proposal(s, b));  // in [0, max_clock]
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
        for (int d = LBFT_TL_SEG / 2; d; d >>= 1) row = ctl_merge_step<LBFT_TL_SEG>(row, d);
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

// Commit finality (lbft_batch_commit_finality): per entry of an instance's chain, the commit times of all its nodes -- an order
// statistic under the voting rights (lbft_commit_finality.h).  The walk -- node pass, chunks of 64 entries, the [n][64] tile, the rights
// table in LDS -- is lbft_chain_walk.h's; the kernel adds what becomes of a column (fin_samples, the two histograms, the first committer,
// the open entries).
// grid = (workgroups per group, groups); a workgroup's LBFT_FN_WAVES wavefronts stride over the instances of its group and accumulate by
// the scheme of lbft_group_stats.h: two LDS histograms (quorum finality and spread) in passes of LBFT_FN_LDS_BINS bins, the first
// committers (n bins) in the first pass, the statistics in registers in the first pass.  Instances with a non-zero fault word are
// skipped.  LDS: tile 4 x 32 x 64 x 4 B = 32 KiB, histograms 2 x 16 KiB, 128 B first committers, 128 B rights, 192 B statistics:
// 65 984 B, two workgroups per CU.
#define LBFT_FN_BLOCK 256
#define LBFT_FN_WAVES (LBFT_FN_BLOCK / 64)
#define LBFT_FN_MAX_NODES CW_MAX_NODES
#define LBFT_FN_LDS_BINS 4096  // each of the two histograms: 16 KiB of u32 counts
#define LBFT_FN_WORKGROUPS 1024u
static_assert(LBFT_FINALITY_STATS == FIN_FAMILIES * 4, "six families of (samples, sum, min, max)");

__global__ __launch_bounds__(LBFT_FN_BLOCK) void lbft_k_ct_finality(Params p, const u32* __restrict__ state, const i32* __restrict__ ctimes,
                                                                    const u32* __restrict__ grp_inst, const u32* __restrict__ grp_off,
                                                                    u32 bin_width, u32 bins, unsigned long long* __restrict__ finality_hist,
                                                                    unsigned long long* __restrict__ spread_hist,
                                                                    unsigned long long* __restrict__ first_committer,
                                                                    unsigned long long* __restrict__ stats) {
  __shared__ i32 tile[LBFT_FN_WAVES][LBFT_FN_MAX_NODES][64];
  __shared__ u32 h_fin[LBFT_FN_LDS_BINS], h_spr[LBFT_FN_LDS_BINS], h_fc[LBFT_FN_MAX_NODES], s_rights[LBFT_FN_MAX_NODES];
  __shared__ unsigned long long s_stat[LBFT_FINALITY_STATS];
  CwWalk w;
  if (!cw_begin(w, p, grp_inst, grp_off, tile, s_rights)) return;  // (the rights: read after the pass loop's first barrier)
  const u32 n = w.n, lane = w.lane;
  gs_stats_clear<LBFT_FINALITY_STATS>(s_stat);
  GsStat st[FIN_FAMILIES] = {};
  for (u32 base = 0; base < bins; base += LBFT_FN_LDS_BINS) {
    const u32 span = bins - base < LBFT_FN_LDS_BINS ? bins - base : LBFT_FN_LDS_BINS;
    const bool stat_pass = base == 0;
    gs_lds_clear<LBFT_FN_BLOCK>(h_fin, span);
    gs_lds_clear<LBFT_FN_BLOCK>(h_spr, span);
    if (stat_pass) gs_lds_clear<LBFT_FN_BLOCK>(h_fc, n);
    __syncthreads();
    for (u32 q = blockIdx.x * LBFT_FN_WAVES + w.wave; q < w.cnt; q += gridDim.x * LBFT_FN_WAVES) {  // (one instance per wavefront: uniform in it)
      const u32 i = gs_instance(grp_inst, w.first, q);
      Sim s(p, const_cast<u32*>(state), i);
      if (s.ld(I_FAULT) != 0) continue;
      const u32 nc = cw_commits(s, lane, n, w.lcap);
      const CwChain ch = cw_node_pass<1>(&nc, lane, n, 64u);
      u32 open = 0;
      for (u32 c0 = 0; c0 < ch.L; c0 += 64) {
        const u32 k = c0 + lane;
        for (u32 j = 0; j < n; j++) cw_stage(w, ctimes, i, nc, j, k);
        if (k >= ch.L) continue;
        const i32 gt = cw_proposal(s, s.ld(w.lg + ch.ref * w.lcap + k));
        const FinEntry e = cw_column(w, k);
        const i32 all = fin_all(e, n);
        if (e.quorum >= 0) gs_lds_count(h_fin, fin_after(e.quorum, gt), bin_width, bins, base, span);
        if (all >= 0) gs_lds_count(h_spr, fin_after(all, e.first), bin_width, bins, base, span);
        if (!stat_pass) continue;
        fin_samples(e, n, gt, [&](u32 family, u32 v) { gs_stat_add(st[family], v); });
        if (e.committers) gs_lds_count(h_fc, e.first_node, 1u, n, 0u, n);
        open += fin_open(e) ? 1u : 0u;
      }
      if (stat_pass) {
        for (int d = 32; d; d >>= 1) open += (u32)__shfl_xor((int)open, d, 64);
        if (lane == 0) gs_stat_add(st[FIN_OPEN], open);  // one sample per instance
      }
    }
    if (stat_pass) gs_reduce_to_lds<FIN_FAMILIES>(st, s_stat, lane == 0);
    __syncthreads();
    gs_lds_flush<LBFT_FN_BLOCK>(h_fin, finality_hist, w.g, bins, base, span);
    gs_lds_flush<LBFT_FN_BLOCK>(h_spr, spread_hist, w.g, bins, base, span);
    if (stat_pass) {
      gs_lds_flush<LBFT_FN_BLOCK>(h_fc, first_committer, w.g, n, 0u, n);
      gs_stats_out<LBFT_FINALITY_STATS>(s_stat, stats, w.g);
    }
    __syncthreads();  // (before the next pass clears the histograms)
  }
}

// Per-instance statistics (lbft_batch_instance_stats): the samples of the three kernels above, with the instance as the unit -- no
// histogram, no atomic, one writer per row (lbft_instance_stats.h).  One wavefront per instance, IST_WAVES per workgroup, striding over
// the instances of the workgroup's group (a group matters for `since` alone), through the generic Sim accessors.
//   node pass and chain pass: lbft_chain_walk.h's.  While row j of a chunk is staged, its entries also give the timeline samples -- the
//     predecessor c_j(k - 1) is the lower lane's entry (__shfl_up; lane 0 reads the row's word before the chunk, so no carry is kept),
//     ctl_entry makes the gap sample, and the chunk's CtlRow is reduced by a butterfly and merged into lane j's (lane = node) -- and the
//     latency sample c_j(k) - its origin (cw_own_proposal).  Lane k then takes the six finality quantities from its column (ist_column).
//   closing pass (lane = node): the row's first / tail / longest samples.
// Every family is accumulated per lane (IstStat), reduced by butterflies once per instance, and the row's IST_WORDS words are stored by
// as many lanes: 352 contiguous bytes.  The row of an instance with a non-zero fault word is left as the caller zeroed it.
// LDS: the tile, 4 x 32 x 64 x 4 B = 32 KiB, and 128 B of rights.
#define LBFT_IS_BLOCK (64 * IST_WAVES)
static_assert(LBFT_INSTANCE_STATS == IST_WORDS && LBFT_INSTANCE_FAMILIES == IST_FAMILIES, "eleven families of (samples, sum, min, max)");
static_assert(LBFT_STALL_STATS == CTL_FAMILIES * 4, "the stall families");

__device__ __forceinline__ IstStat ist_wave_reduce(IstStat s) {
  for (int d = 32; d; d >>= 1) {
    IstStat o;
    o.cnt = (u32)__shfl_xor((int)s.cnt, d, 64);
    o.min = (u32)__shfl_xor((int)s.min, d, 64);
    o.max = (u32)__shfl_xor((int)s.max, d, 64);
    o.sum = (u64)__shfl_xor((unsigned long long)s.sum, d, 64);
    s = ist_merge(s, o);
  }
  return s;
}

__global__ __launch_bounds__(LBFT_IS_BLOCK) void lbft_k_ct_instances(Params p, const u32* __restrict__ state, const i32* __restrict__ ctimes,
                                                                     const u32* __restrict__ grp_inst, const u32* __restrict__ grp_off,
                                                                     const i32* __restrict__ since_of, unsigned long long* __restrict__ rows) {
  __shared__ i32 tile[IST_WAVES][LBFT_FN_MAX_NODES][64];
  __shared__ u32 s_rights[LBFT_FN_MAX_NODES];
  CwWalk w;
  if (!cw_begin(w, p, grp_inst, grp_off, tile, s_rights)) return;
  const u32 n = w.n, lane = w.lane;
  const i32 since = since_of ? since_of[w.g] : 0;
  __syncthreads();
  for (u32 q = blockIdx.x * IST_WAVES + w.wave; q < w.cnt; q += gridDim.x * IST_WAVES) {  // (one instance per wavefront: uniform in it)
    const u32 i = gs_instance(grp_inst, w.first, q);
    Sim s(p, const_cast<u32*>(state), i);
    if (s.ld(I_FAULT) != 0) continue;
    const u32 nc = cw_commits(s, lane, n, w.lcap);
    const CwChain ch = cw_node_pass<1>(&nc, lane, n, 64u);
    IstStat st[IST_FAMILIES];
    for (u32 f = 0; f < IST_FAMILIES; f++) st[f] = ist_empty();
    CtlRow row = ctl_empty();  // of node `lane`
    u32 open = 0;
    for (u32 c0 = 0; c0 < ch.L; c0 += 64) {
      const u32 k = c0 + lane;
      const bool have = k < ch.L;
      u32 b = 0;
      i32 gt = 0;
      if (have) {
        b = s.ld(w.lg + ch.ref * w.lcap + k);
        gt = cw_proposal(s, b);
      }
      for (u32 j = 0; j < n; j++) {
        const CwStaged e = cw_stage(w, ctimes, i, nc, j, k);
        const i32 c = e.c;
        // Lane 0: the last entry of the row's previous chunk.  The load stays in front of the shuffle: folded into the `if` below it the
        // kernel was 6 % slower on 32-node batches (where its code falls, EXPERIMENTS.md "One chain walk"), so time the call after moving it.
        const i32 before = lane == 0 && c0 && k < e.commits ? e.ct[k - 1] : -1;
        i32 prev = __shfl_up(c, 1, 64);
        if (lane == 0) prev = before;
        CtlRow r = ctl_empty();
        const u32 gap = ctl_entry(r, c, prev, since);
        if (gap) ist_add(st[IST_STALLS + CTL_GAPS], gap);
        for (int d = 32; d; d >>= 1) r = ctl_merge_step<64>(r, d);
        if (lane == j) row = ctl_merge(row, r);
        if (c >= 0) ist_add(st[IST_LATENCY], ist_latency(c, cw_own_proposal(s, w, j, k, b, gt)));
      }
      if (have) open += ist_column(st, cw_column(w, k), n, gt);
    }
    // closing pass (lane = node)
    if (lane < n) ist_node(st, row, p.max_clock);
    for (int d = 32; d; d >>= 1) open += (u32)__shfl_xor((int)open, d, 64);
    if (lane == 0) ist_add(st[IST_FINALITY + FIN_OPEN], open);  // one sample per instance
    // reduction and store
    unsigned long long word = 0;
#pragma unroll
    for (u32 f = 0; f < IST_FAMILIES; f++) {
      const IstStat t = ist_wave_reduce(st[f]);
      if (lane / 4 == f) word = ist_word(t, lane % 4);
    }
    if (lane < IST_WORDS) rows[(size_t)i * IST_WORDS + lane] = word;
  }
}

// Commit phases (lbft_batch_commit_phases): the latency histogram's samples and the finality's families first .. spread, split by the
// phase of the entry's proposal time (lbft_commit_phases.h) -- the second grouping axis.  The walk is lbft_chain_walk.h's, LBFT_PH_WAVES
// wavefronts per workgroup striding over the instances of the workgroup's group.  While row j of a chunk is staged, lane k also takes
// the latency sample c_j(k) - its origin (cw_own_proposal), in the origin's phase (on the device the origin is g_k and the phase the
// lane's; a node whose log differs has its own); lane k then takes its column's samples (fin_samples) in the phase of g_k.  The group's
// edges are copied into LDS once per workgroup.
// Histograms: latency and quorum finality, each one virtual histogram of phases x bins bins (phase p's slice at p * bins), in passes of
// LBFT_PH_LDS_BINS LDS bins by the scheme of lbft_group_stats.h; a group's slice of the global array is the virtual histogram itself.
// Statistics, first pass: GsStat accumulators per phase in registers would be an array indexed by a run-time phase, which lands in
// scratch; every sample goes, with four LDS integer atomics, into the workgroup's [phases][24] block of {samples, sum, max(~sample),
// max} words, which is flushed once per workgroup by gs_stats_out's rule with the phase offset.  (The other form -- the lanes of a
// chunk share one or two phases, so one butterfly per distinct phase and one lane's atomics -- is
// profiles/commit_phases/ballot_prereduction.patch, against the kernel's body as it was before lbft_chain_walk.h: faster with one
// phase, slower with three and eight, EXPERIMENTS.md "Commit phases".)  Instances with a non-zero fault word are skipped.
// LDS: tile 32 KiB, histograms 2 x 16 KiB, 128 B rights, 32 B edges, 1536 B statistics: 67 232 B, two workgroups per CU.
#define LBFT_PH_BLOCK 256
#define LBFT_PH_WAVES (LBFT_PH_BLOCK / 64)
#define LBFT_PH_LDS_BINS 4096  // each of the two histograms: 16 KiB of u32 counts
#define LBFT_PH_WORKGROUPS 1024u
static_assert(LBFT_MAX_PHASES == CPH_MAX_PHASES && LBFT_PHASE_FAMILIES == CPH_FAMILIES && LBFT_PHASE_STATS == CPH_STATS, "include/lbft.h");
static_assert(CPH_FINALITY + FIN_SPREAD + 1 == CPH_FAMILIES && CPH_MAX_PHASES * CPH_STATS <= LBFT_PH_BLOCK, "latency, first .. spread; a thread per word");

// One sample into the workgroup's statistics.
__device__ __forceinline__ void cph_sample_to_lds(unsigned long long* s_stat, u32 phase, u32 family, u32 v) {
  atomicAdd(&s_stat[cph_word(phase, family, 0)], 1ull); atomicAdd(&s_stat[cph_word(phase, family, 1)], (unsigned long long)v);
  atomicMax(&s_stat[cph_word(phase, family, 2)], ~(unsigned long long)v); atomicMax(&s_stat[cph_word(phase, family, 3)], (unsigned long long)v);
}

__global__ __launch_bounds__(LBFT_PH_BLOCK) void lbft_k_ct_phases(Params p, const u32* __restrict__ state, const i32* __restrict__ ctimes,
                                                                  const u32* __restrict__ grp_inst, const u32* __restrict__ grp_off,
                                                                  const i32* __restrict__ edges, u32 phases, u32 bin_width, u32 bins,
                                                                  unsigned long long* __restrict__ latency_hist,
                                                                  unsigned long long* __restrict__ finality_hist, unsigned long long* __restrict__ stats) {
  __shared__ i32 tile[LBFT_PH_WAVES][LBFT_FN_MAX_NODES][64];
  __shared__ u32 h_lat[LBFT_PH_LDS_BINS], h_fin[LBFT_PH_LDS_BINS], s_rights[LBFT_FN_MAX_NODES];
  __shared__ i32 s_edges[CPH_MAX_PHASES];
  __shared__ unsigned long long s_stat[CPH_MAX_PHASES * CPH_STATS];
  CwWalk w;
  if (!cw_begin(w, p, grp_inst, grp_off, tile, s_rights)) return;  // (the rights and the edges: read after the pass loop's first barrier)
  const u32 n = w.n, lane = w.lane, g = w.g;
  const u32 n_edges = phases - 1u, vbins = phases * bins, words = phases * CPH_STATS;  // (phases x bins < 2^32: the launcher)
  if (threadIdx.x < CPH_MAX_PHASES) s_edges[threadIdx.x] = threadIdx.x < n_edges ? edges[g * n_edges + threadIdx.x] : CPH_NO_EDGE;
  gs_stats_clear<CPH_MAX_PHASES * CPH_STATS>(s_stat);
  for (u32 base = 0; base < vbins; base += LBFT_PH_LDS_BINS) {
    const u32 span = vbins - base < LBFT_PH_LDS_BINS ? vbins - base : LBFT_PH_LDS_BINS;
    const bool stat_pass = base == 0;
    gs_lds_clear<LBFT_PH_BLOCK>(h_lat, span);
    gs_lds_clear<LBFT_PH_BLOCK>(h_fin, span);
    __syncthreads();
    for (u32 q = blockIdx.x * LBFT_PH_WAVES + w.wave; q < w.cnt; q += gridDim.x * LBFT_PH_WAVES) {  // (one instance per wavefront: uniform in it)
      const u32 i = gs_instance(grp_inst, w.first, q);
      Sim s(p, const_cast<u32*>(state), i);
      if (s.ld(I_FAULT) != 0) continue;
      const u32 nc = cw_commits(s, lane, n, w.lcap);
      const CwChain ch = cw_node_pass<1>(&nc, lane, n, 64u);
      for (u32 c0 = 0; c0 < ch.L; c0 += 64) {
        const u32 k = c0 + lane;
        const bool have = k < ch.L;
        u32 b = 0;
        i32 gt = 0;
        if (have) {
          b = s.ld(w.lg + ch.ref * w.lcap + k);
          gt = cw_proposal(s, b);
        }
        const u32 ph = cph_phase(s_edges, gt);
        for (u32 j = 0; j < n; j++) {
          const i32 c = cw_stage(w, ctimes, i, nc, j, k).c;
          if (c >= 0) {
            const i32 gj = cw_own_proposal(s, w, j, k, b, gt);
            const u32 pj = gj == gt ? ph : cph_phase(s_edges, gj);  // (another block, another time: it has its own phase)
            const u32 l = fin_after(c, gj);
            const u32 vb = cph_bin(pj, l, bin_width, bins);
            if (cph_in_pass(vb, base, span)) atomicAdd(&h_lat[vb - base], 1u);
            if (stat_pass) cph_sample_to_lds(s_stat, pj, CPH_LATENCY, l);
          }
        }
        if (have) {
          const FinEntry e = cw_column(w, k);
          if (e.quorum >= 0) {
            const u32 vb = cph_bin(ph, fin_after(e.quorum, gt), bin_width, bins);
            if (cph_in_pass(vb, base, span)) atomicAdd(&h_fin[vb - base], 1u);
          }
          if (stat_pass) fin_samples(e, n, gt, [&](u32 family, u32 v) { cph_sample_to_lds(s_stat, ph, CPH_FINALITY + family, v); });
        }
      }
    }
    __syncthreads();
    gs_lds_flush<LBFT_PH_BLOCK>(h_lat, latency_hist, g, vbins, base, span);
    gs_lds_flush<LBFT_PH_BLOCK>(h_fin, finality_hist, g, vbins, base, span);
    if (stat_pass && threadIdx.x < words && s_stat[threadIdx.x & ~3u]) {  // gs_stats_out's rule; a group's block is phases x CPH_STATS words
      if ((threadIdx.x & 3u) < 2u) atomicAdd(&stats[(size_t)g * words + threadIdx.x], s_stat[threadIdx.x]);
      else atomicMax(&stats[(size_t)g * words + threadIdx.x], s_stat[threadIdx.x]);
    }
    __syncthreads();  // (before the next pass clears the histograms)
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

__attribute__((visibility("default"))) hipError_t lbft_ct_launch_finality(const Params* p, const u32* state, const i32* ctimes, const u32* grp_inst,
                                                                         const u32* grp_off, u32 n_groups, u32 max_group, u32 bin_width, u32 bins,
                                                                         unsigned long long* finality_hist, unsigned long long* spread_hist,
                                                                         unsigned long long* first_committer, unsigned long long* stats,
                                                                         hipStream_t stream) {
  if (bin_width == 0 || bins == 0 || n_groups == 0 || max_group == 0 || p->n > LBFT_FN_MAX_NODES || !ctimes || !finality_hist || !spread_hist ||
      !first_committer || !stats)
    return hipErrorInvalidValue;
  // (an instance of the largest group gives at most lcap samples to a bin of a histogram)
  const u64 gx = gs_workgroups(LBFT_FN_WORKGROUPS, n_groups, ((u64)max_group + LBFT_FN_WAVES - 1) / LBFT_FN_WAVES, (u64)max_group * p->lcap);
  lbft_k_ct_finality<<<dim3((u32)gx, n_groups), LBFT_FN_BLOCK, 0, stream>>>(*p, state, ctimes, grp_inst, grp_off, bin_width, bins, finality_hist, spread_hist,
                                                                         first_committer, stats);
  return hipGetLastError();
}

// rows[instance * LBFT_INSTANCE_STATS ..], zeroed by the caller.  The kernel writes the minimum itself, not its complement: a row has
// one writer, so the caller's GroupedCall::finish() has nothing to undo (the output is no `stats` buffer).  Grid: ist_workgroups.
__attribute__((visibility("default"))) hipError_t lbft_ct_launch_instances(const Params* p, const u32* state, const i32* ctimes, const u32* grp_inst,
                                                                          const u32* grp_off, u32 n_groups, u32 max_group, const i32* since_of,
                                                                          unsigned long long* rows, hipStream_t stream) {
  if (n_groups == 0 || max_group == 0 || p->n > LBFT_FN_MAX_NODES || !ctimes || !rows) return hipErrorInvalidValue;
  const u64 gx = ist_workgroups(n_groups, max_group);
  lbft_k_ct_instances<<<dim3((u32)gx, n_groups), LBFT_IS_BLOCK, 0, stream>>>(*p, state, ctimes, grp_inst, grp_off, since_of, rows);
  return hipGetLastError();
}

// edges[group * (phases - 1) ..]: the group's edges, each in [0, p->max_clock + 1] and none below its predecessor (the caller checked);
// NULL with phases == 1.  Every output zeroed by the caller.  Grid: gs_workgroups, an instance giving a bin at most n x lcap samples.
__attribute__((visibility("default"))) hipError_t lbft_ct_launch_phases(const Params* p, const u32* state, const i32* ctimes, const u32* grp_inst,
                                                                       const u32* grp_off, u32 n_groups, u32 max_group, const i32* edges, u32 phases,
                                                                       u32 bin_width, u32 bins, unsigned long long* latency_hist,
                                                                       unsigned long long* finality_hist, unsigned long long* stats, hipStream_t stream) {
  if (bin_width == 0 || bins == 0 || n_groups == 0 || max_group == 0 || p->n > LBFT_FN_MAX_NODES || !ctimes || !latency_hist || !finality_hist ||
      !stats || phases == 0 || phases > CPH_MAX_PHASES || (phases > 1 && !edges) || (u64)phases * bins > 0xffffffffull)
    return hipErrorInvalidValue;
  const u64 gx = gs_workgroups(LBFT_PH_WORKGROUPS, n_groups, ((u64)max_group + LBFT_PH_WAVES - 1) / LBFT_PH_WAVES, (u64)max_group * p->n * p->lcap);
  lbft_k_ct_phases<<<dim3((u32)gx, n_groups), LBFT_PH_BLOCK, 0, stream>>>(*p, state, ctimes, grp_inst, grp_off, edges, phases, bin_width, bins, latency_hist,
                                                                        finality_hist, stats);
  return hipGetLastError();
}

}  // extern "C"
