// lbft_paramsets.hip -- HIP kernels (gfx950) of parameter-set batches (lbft_batch_create_param_sets): one batch in which every instance
// runs one of up to LBFT_MAX_PARAM_SETS sets of delay, pacemaker and loss parameters.
//
// The step is lbft_core.h's, instantiated for the classes K_SMALL_SETS / K_MID_SETS / K_GENERIC_SETS: the K_SMALL / K_MID / K_GENERIC
// step whose accessors of those parameters (SimT::MU, LAMBDA, DUR_TAB, DROP_PPM, ...) read the lane's own set, loaded once at kernel entry
// (SimT::load_set), instead of the batch-wide Params.  Everything else -- network size, voting rights, protocol mode, capacities, state
// layout, LDS layout (lbft_launch.h) -- is the batch's, so the host side of liblbft_hip.so sizes and reads back these batches as any other.
// Built as a library of its own (build.py): the code object of liblbft_hip.so, whose kernels are pinned byte for byte by the codegen
// manifest, does not change.
// The library also holds the four kernels behind every finished run of every kind of batch: lbft_k_ps_counters (the batch counters),
// lbft_k_ps_load (the run load per group and per instance), lbft_k_ps_votes (the vote statistics per group) and lbft_k_ps_epochs (the
// epoch statistics per group).  liblbft_hip.so looks up all six launchers or refuses the file: one built before lbft_ps_launch_load,
// lbft_ps_launch_votes or lbft_ps_launch_epochs existed is refused as a whole, and plain batches then reduce their counters with
// lbft_k_finalize, as they do when the file is missing.
#include <hip/hip_runtime.h>

#include "../../include/lbft.h"
#include "lbft_core.h"
#include "lbft_paramsets.h"

using namespace lbft;

#include "lbft_launch.h"
#include "lbft_run_body.h"  // run_body

// Simulator::new for every instance: init() draws the startup times with the set's delay parameters.
__global__ __launch_bounds__(LBFT_BLOCK) void lbft_k_ps_init(Params p, u32* __restrict__ state, const u64* __restrict__ seeds,
                                                              const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of) {
  u32 i = blockIdx.x * p.lpw + threadIdx.x;
  if (threadIdx.x >= p.lpw || i >= p.m) return;
  SimTSets<K_GENERIC_SETS> s(p, state, i);
  s.load_set(sets[set_of[i]]);
  s.init(seeds[i]);
}

// Small class (lbft_k_run0's geometry: two wavefronts per SIMD): n <= 16, honest, lossless, no trace, reference routing.
__global__ LBFT_TWO_WAVE_BOUNDS void lbft_k_ps_run0(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of) {
  run_body<K_SMALL_SETS>(p, state, unfinished, sets, set_of);
}
// Mid class (lbft_k_run<1>'s geometry: one wavefront per SIMD, the whole register file): n <= 32, every feature.
__global__ __launch_bounds__(64 * LBFT_RUN_WAVES_FULL)
void lbft_k_ps_run1(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of) {
  run_body<K_MID_SETS>(p, state, unfinished, sets, set_of);
}

// The batch counters of a finished run without the State hashes: the tail of lbft_k_finalize (liblbft_hip.so) as a kernel of its own, for
// batches of every kind -- it reads the instance's scalar rows and two words per node through the generic accessors, whatever kernel ran.
// One lane per instance; a workgroup of LBFT_COUNTER_WAVES wavefronts reduces its instances' words (shuffles within a wavefront, then
// LDS across the wavefronts) and adds them to the batch's with ONE atomic per counter: the atomics of a run all go to one 128-byte line.
#include "lbft_batch_counters.h"
#define LBFT_COUNTER_WAVES 16
__global__ __launch_bounds__(64 * LBFT_COUNTER_WAVES) void lbft_k_ps_counters(Params p, const u32* __restrict__ state, unsigned long long* __restrict__ counters) {
  __shared__ u64 part[LBFT_COUNTER_WAVES][C_WORDS];
  u64 c[C_WORDS];
  instance_counter_words(p, state, blockIdx.x * (64 * LBFT_COUNTER_WAVES) + threadIdx.x, c);
  for (int k = 0; k < C_WORDS; k++) {
    u64 r = k >= C_MAXQ ? wave_max(c[k]) : wave_sum(c[k]);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = r;
  }
  __syncthreads();
  if (threadIdx.x >= C_WORDS) return;
  const u32 k = threadIdx.x;
  const bool is_max = k >= C_MAXQ;
  u64 r = part[0][k];
  for (int w = 1; w < LBFT_COUNTER_WAVES; w++) r = is_max ? (part[w][k] > r ? part[w][k] : r) : r + part[w][k];
  if (is_max) atomicMax(&counters[k], (unsigned long long)r);
  else atomicAdd(&counters[k], (unsigned long long)r);
}

// The run load (lbft_batch_load_stats, lbft_batch_instance_load): sixteen u32 samples per instance -- the rule header's families -- from
// the words a finished run of any kind leaves on the device, read through the generic accessors (instance-major rows or 64-instance
// tiles alike).  One 16-lane segment per instance, four instances per wavefront, lane f of a segment = family f:
//   lanes 0-3 and 5-12 load their family's word; `messages` is a segment add of lanes 0-2; for the three families over the nodes the
//   segment's lanes stride over the nodes two words each (128 nodes: eight trips) and merge by a 16-lane butterfly;
//   rows != NULL: lane f stores rows[i * 16 + f] (consecutive instances: 256 contiguous bytes per wavefront);
//   stats != NULL: lane k (and k + 16) counts fault bit k into the census; of an instance without a fault every lane adds its sample to
//   its ONE GsStat, lane hist_family bins it.  The workgroup's stride over, the segments are combined (ld_reduce_to_lds).
// The stride is uniform in the wavefront (its four instances are predicated), so every shuffle has all 64 lanes.
// grid = (ld_workgroups per group, groups); the LDS histogram goes in passes of LD_LDS_BINS bins (lbft_group_stats.h), the rows, the
// census and the statistics in the first.
#include "lbft_load_stats.h"
__device__ __forceinline__ u32 ld_row_of(u32 w) {  // LoadWord -> the instance's row
  return w < LDW_STAMP ? I_EV0 + w : w == LDW_STAMP ? (u32)I_STAMP : w == LDW_DRAWS ? (u32)I_DRAWS : w == LDW_NFOLD ? (u32)I_NFOLD : w == LDW_NUPD ? (u32)I_NUPD
       : w == LDW_MAXQ ? (u32)I_MAXQ : w == LDW_CAL_BUMP ? (u32)I_CAL_BUMP : w == LDW_MAXSNAP ? (u32)I_MAXSNAP : (u32)I_NBLOCKS;
}
static_assert(I_EV1 == I_EV0 + 1 && I_EV2 == I_EV0 + 2 && I_EV3 == I_EV0 + 3 && LDW_STAMP == 4, "ld_row_of");
__global__ __launch_bounds__(LD_BLOCK) void lbft_k_ps_load(Params p, const u32* __restrict__ state, const u32* __restrict__ grp_inst,
                                                           const u32* __restrict__ grp_off, u32 hist_family, u32 bin_width, u32 bins,
                                                           unsigned long long* __restrict__ hist, unsigned long long* __restrict__ faults,
                                                           unsigned long long* __restrict__ stats, u32* __restrict__ rows) {
  __shared__ u32 h[LD_LDS_BINS];
  __shared__ unsigned long long s_stat[LD_WORDS];
  __shared__ u32 s_fault[LD_FAULT_BITS];
  const u32 per = LD_BLOCK / LD_SEGMENT;  // instances per workgroup and step
  const u32 g = blockIdx.y;
  const uint2 grp = gs_group(grp_inst, grp_off, g, p.m);
  const u32 first = grp.x, cnt = grp.y;
  if (blockIdx.x * per >= cnt) return;  // (the whole workgroup: its group has fewer instances)
  const u32 lane = threadIdx.x % 64, f = threadIdx.x % LD_SEGMENT, seg = threadIdx.x / LD_SEGMENT;
  const u32 n = p.n, word = ld_word_of(f);
  const bool calendar = p.qcal != 0, grouped = stats != nullptr;
  if (grouped) {
    gs_stats_clear<LD_WORDS>(s_stat);
    if (threadIdx.x < LD_FAULT_BITS) s_fault[threadIdx.x] = 0;
  }
  GsStat st = {};
  for (u32 base = 0; base < bins; base += LD_LDS_BINS) {
    const u32 span = bins - base < LD_LDS_BINS ? bins - base : LD_LDS_BINS;
    const bool first_pass = base == 0;
    if (grouped) gs_lds_clear<LD_BLOCK>(h, span);
    __syncthreads();
    for (u32 k0 = blockIdx.x * per; k0 < cnt; k0 += gridDim.x * per) {  // (uniform in the workgroup)
      const u32 k = k0 + seg;
      const bool valid = k < cnt;
      u32 i = 0, fault = 0, v = 0;
      LdNodes nodes = ld_nodes_empty();
      if (valid) {
        i = gs_instance(grp_inst, first, k);
        Sim s(p, const_cast<u32*>(state), i);
        fault = s.ld(I_FAULT);
        if (word != LDW_NONE) v = ld_word_sample(f, s.ld(ld_row_of(word)), calendar);
        for (u32 q = f; q < n; q += LD_SEGMENT) ld_nodes_add(nodes, s.nfm(q, NF_NCOMMITS), s.nfm(q, NF_PM_ROUND));
      }
      nodes = ld_segment_merge(nodes);
      v = ld_sample(f, v, ld_segment_sum(ld_message_share(f, v)), nodes);
      if (!valid) continue;
      if (first_pass && rows) rows[(size_t)i * LD_FAMILIES + f] = v;
      if (!grouped) continue;
      if (first_pass) {
        if (ld_fault_bit(fault, f)) atomicAdd(&s_fault[f], 1u);
        if (ld_fault_bit(fault, f + LD_SEGMENT)) atomicAdd(&s_fault[f + LD_SEGMENT], 1u);
      }
      if (!ld_clean(fault)) continue;
      if (first_pass) gs_stat_add(st, v);
      if (f == hist_family) gs_lds_count(h, v, bin_width, bins, base, span);
    }
    if (!grouped) return;  // (the rows alone: one pass, nothing in LDS)
    if (first_pass) ld_reduce_to_lds(st, s_stat, lane);
    __syncthreads();
    gs_lds_flush<LD_BLOCK>(h, hist, g, bins, base, span);
    if (first_pass) {
      gs_stats_out<LD_WORDS>(s_stat, stats, g);
      if (threadIdx.x < LD_FAULT_BITS && s_fault[threadIdx.x]) atomicAdd(&faults[(size_t)g * LD_FAULT_BITS + threadIdx.x], (unsigned long long)s_fault[threadIdx.x]);
    }
    __syncthreads();  // (before the next pass clears the histogram)
  }
}

// The vote statistics (lbft_batch_vote_stats): per group, the voter sets of the committed chain -- votes, weight and margin of every
// quorum certificate, who voted, the rounds the chain skipped -- and the block pool sorted into chain, orphaned and pending, by author.
// One wavefront per instance, walked with lbft_chain_walk.h (node pass, pool bound, chunk head, predecessor and tip, membership): the
// kernel reads, through the generic Sim accessors (every layout), the fault word, I_NBLOCKS, NF_NCOMMITS of the nodes, the reference
// node's log row and of the block records B_LINK, B_ROUND, B_EPOCH, B_DEPTH and the mw voter words.
//   chain pass (lane = entry, 64 at a time): popcounts of the voter words; the weight from the rights table in LDS at the epoch's
//     rotation (unit rights: the popcount); every voter bit counts into the LDS node table.  Round and epoch of the predecessor and of
//     the tip.
//   pool pass (lane = block id, 64 at a time over 1 .. nb; first pass only): proposed and orphaned count into the LDS node table by
//     author, the per-instance counts are ballots.
// grid = (workgroups per group, groups); a workgroup's VT_WAVES wavefronts stride over the instances of its group and accumulate by the
// scheme of lbft_group_stats.h: the margin histogram in passes of VT_LDS_BINS bins; the vote-count histogram, the node table and the
// statistics in the first pass.  Instances with a non-zero fault word are skipped.
#include "lbft_record_hash_rules.h"  // rh_voter_field, rh_author_bits
#include "lbft_vote_rules.h"
#include "lbft_chain_walk.h"  // (after the vote rules: cw_pool_member)
#define VT_BLOCK 256
#define VT_WAVES (VT_BLOCK / 64)
#define VT_LDS_BINS 4096  // the margin histogram: 16 KiB of u32 counts
#define VT_WORKGROUPS 1024u
#define VT_NODE_ROUNDS ((LBFT_MAX_NODES + 63) / 64)
#define VT_MASK_WORDS ((LBFT_MAX_NODES + 31) / 32)
static_assert(LBFT_VOTE_STATS == VT_FAMILIES * 4 && LBFT_VOTE_FAMILIES == VT_FAMILIES && LBFT_VOTE_NODE_COLUMNS == VT_NODE_COLUMNS, "lbft.h");
static_assert(LBFT_MAX_NODES <= VT_BLOCK, "the rights table is copied by one lane per node");
__global__ __launch_bounds__(VT_BLOCK) void lbft_k_ps_votes(Params p, const u32* __restrict__ state, const u32* __restrict__ grp_inst,
                                                            const u32* __restrict__ grp_off, u32 bin_width, u32 bins,
                                                            unsigned long long* __restrict__ margin_hist, unsigned long long* __restrict__ votes_hist,
                                                            unsigned long long* __restrict__ node_table, unsigned long long* __restrict__ stats) {
  __shared__ u32 h_margin[VT_LDS_BINS], h_votes[LBFT_MAX_NODES + 1], h_node[LBFT_MAX_NODES * VT_NODE_COLUMNS], s_rights[LBFT_MAX_NODES];
  __shared__ unsigned long long s_stat[LBFT_VOTE_STATS];
  // cw_group_begin, written out: through the helper this kernel takes 128 vector registers for 127 (EXPERIMENTS.md "One pool walk")
  const u32 g = blockIdx.y;
  const uint2 grp = gs_group(grp_inst, grp_off, g, p.m);
  const u32 first = grp.x, cnt = grp.y;
  if (blockIdx.x * VT_WAVES >= cnt) return;
  const u32 wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const u32 n = p.n, lcap = p.lcap, lg = p.off_log, mw = p.mw, quorum = p.quorum, rot = p.rot;
  const bool unit = p.unit_weights != 0;
  gs_stats_clear<LBFT_VOTE_STATS>(s_stat);
  if (!unit && threadIdx.x < n) s_rights[threadIdx.x] = p.weights[threadIdx.x];  // (read after the pass loop's first barrier)
  GsStat st[VT_FAMILIES] = {};
  for (u32 base = 0; base < bins; base += VT_LDS_BINS) {
    const u32 span = bins - base < VT_LDS_BINS ? bins - base : VT_LDS_BINS;
    const bool stat_pass = base == 0;
    gs_lds_clear<VT_BLOCK>(h_margin, span);
    if (stat_pass) {
      gs_lds_clear<VT_BLOCK>(h_votes, n + 1);
      gs_lds_clear<VT_BLOCK>(h_node, n * VT_NODE_COLUMNS);
    }
    __syncthreads();
    for (u32 q = blockIdx.x * VT_WAVES + wave; q < cnt; q += gridDim.x * VT_WAVES) {  // (one instance per wavefront: uniform in it)
      const u32 i = gs_instance(grp_inst, first, q);
      Sim s(p, const_cast<u32*>(state), i);
      if (s.ld(I_FAULT) != 0) continue;
      // node pass
      u32 nc[VT_NODE_ROUNDS];
      const CwChain ch = cw_chain_of(s, lane, n, lcap, 64u, nc);
      const u32 row = lg + ch.ref * lcap, nb = cw_pool_blocks(s, p);
      // chain pass
      u32 L = ch.L;  // the chain's entries: up to the first id outside the pool
      u32 carry_r = 0, carry_e = 0, tip_r = 0, tip_e = 0;
      for (u32 c0 = 0; c0 < L; c0 += 64) {
        const u32 k = c0 + lane;
        const CwChunk ck = cw_chunk(s, row, c0, L, nb, lane, 64u, 0u);
        const u32 y = ck.y, nv = ck.nv;
        const bool live = lane < nv;
        u32 round = 0, epoch = 0, votes = 0, weight = 0;
        if (live) {
          round = s.bf(y, B_ROUND); epoch = s.bf(y, B_EPOCH);
          const u32 shift = vt_rights_shift(epoch, rot, n);
#pragma unroll
          for (u32 w = 0; w < VT_MASK_WORDS; w++) {
            if (w >= mw) continue;
            const u32 v = s.bf(y, rh_voter_field(w, mw)) & rh_author_bits(w, n);
            votes += (u32)__popc(v);
            if (unit && !stat_pass) continue;
            for (u32 m = v; m; m &= m - 1u) {
              const u32 a = 32 * w + (u32)ctz32(m);  // (a < n: rh_author_bits)
              if (!unit) weight += s_rights[vt_right_index(a, shift, n)];
              if (stat_pass) atomicAdd(&h_node[vt_node_cell(a, VT_COL_VOTED)], 1u);
            }
          }
          if (unit) weight = votes;
        }
        const u32 pr = cw_prev(round, carry_r, lane), pe = cw_prev(epoch, carry_e, lane);
        if (nv) { tip_r = cw_tip(round, nv); tip_e = cw_tip(epoch, nv); }
        if (live && votes) {
          const u32 margin = vt_margin(weight, quorum);
          gs_lds_count(h_margin, margin, bin_width, bins, base, span);
          if (stat_pass) {
            gs_stat_add(st[VT_VOTES], votes); gs_stat_add(st[VT_WEIGHT], weight); gs_stat_add(st[VT_MARGIN], margin);
            atomicAdd(&h_votes[votes], 1u);  // (votes <= n: the bits of authors below n)
          }
        }
        if (stat_pass && live && k > 0 && vt_same_epoch(pe, epoch)) gs_stat_add(st[VT_SKIPPED], vt_skipped(pr, round));
        if (cw_ends(ck)) L = c0 + nv;  // (ends the loop)
      }
      if (!stat_pass) continue;
      // pool pass
      u32 orphaned = 0, pending = 0, certified_off = 0;
      for (u32 b0 = 1; b0 <= nb; b0 += 64) {
        const u32 b = b0 + lane;
        const bool have = b <= nb;
        u32 cls = VT_ON_CHAIN, author = 0;
        bool certified = false;
        if (have) {
          author = s.bf(b, B_LINK) >> 16;
          const u32 round = s.bf(b, B_ROUND), epoch = s.bf(b, B_EPOCH), depth = s.bf(b, B_DEPTH);
#pragma unroll
          for (u32 w = 0; w < VT_MASK_WORDS; w++)
            if (w < mw) certified |= (s.bf(b, rh_voter_field(w, mw)) & rh_author_bits(w, n)) != 0;
          cls = vt_classify(cw_pool_member(s, row, depth, L, b), L != 0, epoch, round, tip_e, tip_r);
          if (author < n) {
            atomicAdd(&h_node[vt_node_cell(author, VT_COL_PROPOSED)], 1u);
            if (cls == VT_ORPHAN) atomicAdd(&h_node[vt_node_cell(author, VT_COL_ORPHANED)], 1u);
          }
        }
        orphaned += cw_ballot_count(have && cls == VT_ORPHAN);
        pending += cw_ballot_count(have && cls == VT_PENDING_BLOCK);
        certified_off += cw_ballot_count(have && cls != VT_ON_CHAIN && certified);
      }
      if (lane == 0) {  // one sample per instance
        gs_stat_add(st[VT_BLOCKS], nb); gs_stat_add(st[VT_ORPHANED], orphaned);
        gs_stat_add(st[VT_PENDING], pending); gs_stat_add(st[VT_CERTIFIED_OFF], certified_off);
      }
    }
    if (stat_pass) gs_reduce_to_lds<VT_FAMILIES>(st, s_stat, lane == 0);
    __syncthreads();
    gs_lds_flush<VT_BLOCK>(h_margin, margin_hist, g, bins, base, span);
    if (stat_pass) {
      gs_lds_flush<VT_BLOCK>(h_votes, votes_hist, g, n + 1, 0u, n + 1);
      gs_lds_flush<VT_BLOCK>(h_node, node_table, g, n * VT_NODE_COLUMNS, 0u, n * VT_NODE_COLUMNS);
      gs_stats_out<LBFT_VOTE_STATS>(s_stat, stats, g);
    }
    __syncthreads();  // (before the next pass clears the histogram)
  }
}

// The epoch statistics (lbft_batch_epoch_stats): per group, the committed chain cut into segments of one epoch -- their length, duration
// and rounds, the handover between two of them --, the epochs the nodes ended in and the pool blocks stranded in an epoch the chain has
// left; the same per epoch in the epoch table.  One wavefront per instance, walked with lbft_chain_walk.h as lbft_k_ps_votes is, the
// generic Sim accessors (every layout).  The kernel reads the fault word, I_NBLOCKS, NF_NCOMMITS, NF_EPOCH and NF_STARTUP of the nodes, the
// reference node's log row and of the block records B_LINK, B_ROUND, B_EPOCH, B_TIME and B_DEPTH.
//   node pass: the same lanes read NF_EPOCH, and wavefront max, min and sum of it give families node_epoch and behind whole.
//   chain pass (lane = entry, 64 at a time): e, r and g of the predecessor (cw_prev).
//     The segment starts of a chunk are a ballot; a start at k > 0 is a boundary and closes the segment before it, whose first entry is
//     the highest start below the lane or the carried one (ep_segment_first; its g by one more shuffle): length, duration, last_round
//     and the row of the EARLIER epoch (complete, duration), handover and the row of the LATER one.  Every start gives first_round and
//     counts a segment, every entry counts into its epoch's row: the open segment at the chain's end has thereby given all it gives.
//   pool pass (lane = block id, 64 at a time over 1 .. nb; first pass only): a block counts into its epoch's row; stranded
//     (ep_stranded) by ballot for the instance and per block for the row.
// LDS: the handover histogram in passes of EP_LDS_BINS bins (16 KiB); the table's five counting columns as u32 cells for all 512 rows
// (10 KiB) and its two time columns as 64-bit cells for the first EP_LDS_SUM_ROWS rows (4 KiB) -- a sum of times is never held in less
// than 64 bits; rows above that, which only a chain of more than 256 epochs reaches, add to the global table directly --; the
// statistics.  Table and statistics are taken in the first pass.  Instances with a non-zero fault word are skipped.
#include "lbft_epoch_rules.h"
#define EP_BLOCK 256
#define EP_WAVES (EP_BLOCK / 64)
#define EP_LDS_BINS 4096  // the handover histogram: 16 KiB of u32 counts
#define EP_WORKGROUPS 1024u
#define EP_NODE_ROUNDS ((LBFT_MAX_NODES + 63) / 64)
#define EP_COUNT_COLUMNS 5u  // segments, complete, entries, stranded, blocks
#define EP_SUM_COLUMNS 2u    // duration, handover
#define EP_LDS_SUM_ROWS 256u
static_assert(LBFT_EPOCH_STATS == EP_FAMILIES * 4 && LBFT_EPOCH_FAMILIES == EP_FAMILIES && LBFT_EPOCH_COLUMNS == EP_COLUMNS && LBFT_EPOCH_MAX_BINS == EP_MAX_BINS, "lbft.h");
static_assert(EP_COUNT_COLUMNS + EP_SUM_COLUMNS == EP_COLUMNS && EP_COL_DURATION == 3 && EP_COL_HANDOVER == 4, "ep_count_slot / ep_count_column");
__device__ __forceinline__ u32 ep_count_slot(u32 column) { return column < EP_COL_DURATION ? column : column - EP_SUM_COLUMNS; }  // column -> its LDS cell of a row
__device__ __forceinline__ u32 ep_count_column(u32 slot) { return slot < EP_COL_DURATION ? slot : slot + EP_SUM_COLUMNS; }
__device__ __forceinline__ void ep_count(u32* t_cnt, u32 row, u32 column) { atomicAdd(&t_cnt[row * EP_COUNT_COLUMNS + ep_count_slot(column)], 1u); }
// A time into column `column` of row `row`: the 64-bit LDS cell, or above EP_LDS_SUM_ROWS the group's global row (table_g).
__device__ __forceinline__ void ep_time(unsigned long long* t_sum, unsigned long long* table_g, u32 row, u32 column, u32 v) {
  if (row < EP_LDS_SUM_ROWS) atomicAdd(&t_sum[row * EP_SUM_COLUMNS + (column - EP_COL_DURATION)], (unsigned long long)v);
  else atomicAdd(&table_g[ep_cell(row, column)], (unsigned long long)v);
}
// `cnt` samples of family f, summing to `sum` and lying in [lo, hi], straight into the workgroup's statistics (GsStat's words: the
// minimum as max(~v)).  For the families with one sample per instance or per node, by one lane per instance: held in registers like the
// others, each would take eight in every lane.
__device__ __forceinline__ void ep_stat_lds(unsigned long long* s_stat, u32 f, u64 cnt, u64 sum, u32 lo, u32 hi) {
  atomicAdd(&s_stat[4 * f], (unsigned long long)cnt); atomicAdd(&s_stat[4 * f + 1], (unsigned long long)sum);
  atomicMax(&s_stat[4 * f + 2], ~(unsigned long long)lo); atomicMax(&s_stat[4 * f + 3], (unsigned long long)hi);
}
#define EP_LANE_FIRST EP_LENGTH  // families EP_LENGTH .. EP_HANDOVER have a sample per segment or boundary: registers of the lanes
#define EP_LANE_FAMILIES (EP_HANDOVER - EP_LENGTH + 1)
__global__ __launch_bounds__(EP_BLOCK) void lbft_k_ps_epochs(Params p, const u32* __restrict__ state, const u32* __restrict__ grp_inst,
                                                             const u32* __restrict__ grp_off, u32 bin_width, u32 bins, u32 epoch_bins,
                                                             unsigned long long* __restrict__ handover_hist, unsigned long long* __restrict__ epoch_table,
                                                             unsigned long long* __restrict__ stats) {
  __shared__ u32 h_hand[EP_LDS_BINS], t_cnt[EP_MAX_BINS * EP_COUNT_COLUMNS];
  __shared__ unsigned long long t_sum[EP_LDS_SUM_ROWS * EP_SUM_COLUMNS], s_stat[LBFT_EPOCH_STATS];
  CwGroup wg;
  if (!cw_group_begin<EP_WAVES>(wg, p, grp_inst, grp_off)) return;
  const u32 g = wg.g, first = wg.first, cnt = wg.cnt, wave = wg.wave, lane = wg.lane;
  const u32 n = p.n, lcap = p.lcap, lg = p.off_log;
  const u32 sum_rows = epoch_bins < EP_LDS_SUM_ROWS ? epoch_bins : EP_LDS_SUM_ROWS;
  unsigned long long* const table_g = epoch_table + (size_t)g * epoch_bins * EP_COLUMNS;
  gs_stats_clear<LBFT_EPOCH_STATS>(s_stat);
  GsStat st[EP_LANE_FAMILIES] = {};  // family f at st[f - EP_LANE_FIRST]
  for (u32 base = 0; base < bins; base += EP_LDS_BINS) {
    const u32 span = bins - base < EP_LDS_BINS ? bins - base : EP_LDS_BINS;
    const bool stat_pass = base == 0;
    gs_lds_clear<EP_BLOCK>(h_hand, span);
    if (stat_pass) {
      gs_lds_clear<EP_BLOCK>(t_cnt, epoch_bins * EP_COUNT_COLUMNS);
      for (u32 k = threadIdx.x; k < sum_rows * EP_SUM_COLUMNS; k += EP_BLOCK) t_sum[k] = 0;
    }
    __syncthreads();
    for (u32 q = blockIdx.x * EP_WAVES + wave; q < cnt; q += gridDim.x * EP_WAVES) {  // (one instance per wavefront: uniform in it)
      const u32 i = gs_instance(grp_inst, first, q);
      Sim s(p, const_cast<u32*>(state), i);
      if (s.ld(I_FAULT) != 0) continue;
      // node pass
      u32 nc[EP_NODE_ROUNDS], e_max = 0, e_min = ~0u;
      unsigned long long e_sum = 0;
      const CwChain ch = cw_chain_of(s, lane, n, lcap, 64u, nc);
#pragma unroll
      for (u32 r = 0; r < EP_NODE_ROUNDS; r++)
        if (r * 64 + lane < n) {
          const u32 e = s.nfm(r * 64 + lane, NF_EPOCH);
          e_max = e > e_max ? e : e_max; e_min = e < e_min ? e : e_min; e_sum += e;
        }
      if (stat_pass) {  // E_max, E_min and the sum of the E_j: behind's samples E_max - E_j lie in [0, E_max - E_min] and sum to n E_max - sum
        for (int d = 32; d; d >>= 1) {
          const u32 hi = (u32)__shfl_xor((int)e_max, d, 64), lo = (u32)__shfl_xor((int)e_min, d, 64);
          e_max = hi > e_max ? hi : e_max; e_min = lo < e_min ? lo : e_min; e_sum += __shfl_xor(e_sum, d, 64);
        }
        if (lane == 0) {
          ep_stat_lds(s_stat, EP_NODE_EPOCH, n, e_sum, e_min, e_max);
          ep_stat_lds(s_stat, EP_BEHIND, n, (u64)n * e_max - e_sum, 0u, e_max - e_min);
        }
      }
      const u32 row = lg + ch.ref * lcap, nb = cw_pool_blocks(s, p);
      // chain pass
      u32 L = ch.L;  // the chain's entries: up to the first id outside the pool
      u32 carry_e = 0, carry_r = 0, carry_start = 0, tip_e = 0, segments = 0;
      i32 carry_g = 0, carry_first_g = 0;  // g of the previous chunk's last entry; g of the entry at carry_start
      for (u32 c0 = 0; c0 < L; c0 += 64) {
        const u32 k = c0 + lane;
        const CwChunk ck = cw_chunk(s, row, c0, L, nb, lane, 64u, 0u);
        const u32 y = ck.y, nv = ck.nv;
        const bool live = lane < nv;
        u32 epoch = 0, round = 0;
        i32 gt = 0;
        if (live) {
          epoch = s.bf(y, B_EPOCH); round = s.bf(y, B_ROUND);
          gt = cw_proposal(s, y, s.blk_author(y));
        }
        const u32 pe = cw_prev(epoch, carry_e, lane), pr = cw_prev(round, carry_r, lane);
        const i32 pg = cw_prev(gt, carry_g, lane);
        if (nv) tip_e = cw_tip(epoch, nv);
        const bool start = live && ep_segment_start(k, epoch, pe);
        const unsigned long long starts = __ballot(start), below = starts & ((1ull << lane) - 1ull);
        const i32 lane_first_g = __shfl(gt, (int)ep_start_lane(below), 64);
        const i32 first_g = below ? lane_first_g : carry_first_g;  // g of the first entry of the segment that ends before this lane
        if (start && k > 0) {  // a boundary
          const u32 handover = ep_clamped(gt, pg);
          gs_lds_count(h_hand, handover, bin_width, bins, base, span);
          if (stat_pass) {
            const u32 duration = ep_clamped(pg, first_g), x_prev = ep_bin(pe, epoch_bins);
            gs_stat_add(st[EP_LENGTH - EP_LANE_FIRST], k - ep_segment_first(below, c0, carry_start));
            gs_stat_add(st[EP_DURATION - EP_LANE_FIRST], duration); gs_stat_add(st[EP_LAST_ROUND - EP_LANE_FIRST], pr); gs_stat_add(st[EP_HANDOVER - EP_LANE_FIRST], handover);
            ep_count(t_cnt, x_prev, EP_COL_COMPLETE);
            ep_time(t_sum, table_g, x_prev, EP_COL_DURATION, duration);
            ep_time(t_sum, table_g, ep_bin(epoch, epoch_bins), EP_COL_HANDOVER, handover);
          }
        }
        if (stat_pass && live) {
          const u32 x = ep_bin(epoch, epoch_bins);
          ep_count(t_cnt, x, EP_COL_ENTRIES);
          if (start) { gs_stat_add(st[EP_FIRST_ROUND - EP_LANE_FIRST], round); ep_count(t_cnt, x, EP_COL_SEGMENTS); }
        }
        if (starts) carry_first_g = __shfl(gt, (int)ep_highest(starts), 64);
        carry_start = ep_carry_start(starts, c0, carry_start);
        segments += (u32)__popcll(starts);
        if (cw_ends(ck)) L = c0 + nv;  // (ends the loop)
      }
      if (!stat_pass) continue;
      // pool pass
      u32 stranded = 0;
      for (u32 b0 = 1; b0 <= nb; b0 += 64) {
        const u32 b = b0 + lane;
        const bool have = b <= nb;
        bool off = false;
        if (have) {
          const u32 epoch = s.bf(b, B_EPOCH), x = ep_bin(epoch, epoch_bins);
          off = ep_stranded(cw_pool_member(s, row, s.bf(b, B_DEPTH), L, b), L != 0, epoch, tip_e);
          ep_count(t_cnt, x, EP_COL_BLOCKS);
          if (off) ep_count(t_cnt, x, EP_COL_STRANDED);
        }
        stranded += cw_ballot_count(off);
      }
      if (lane == 0) {  // one sample per instance
        ep_stat_lds(s_stat, EP_SEGMENTS, 1, segments, segments, segments); ep_stat_lds(s_stat, EP_STRANDED, 1, stranded, stranded, stranded);
        ep_stat_lds(s_stat, EP_BLOCKS, 1, nb, nb, nb);
      }
    }
    if (stat_pass) gs_reduce_to_lds<EP_LANE_FAMILIES>(st, s_stat + 4 * EP_LANE_FIRST, lane == 0);
    __syncthreads();
    gs_lds_flush<EP_BLOCK>(h_hand, handover_hist, g, bins, base, span);
    if (stat_pass) {
      for (u32 k = threadIdx.x; k < epoch_bins * EP_COUNT_COLUMNS; k += EP_BLOCK)
        if (t_cnt[k]) atomicAdd(&table_g[ep_cell(k / EP_COUNT_COLUMNS, ep_count_column(k % EP_COUNT_COLUMNS))], (unsigned long long)t_cnt[k]);
      for (u32 k = threadIdx.x; k < sum_rows * EP_SUM_COLUMNS; k += EP_BLOCK)
        if (t_sum[k]) atomicAdd(&table_g[ep_cell(k / EP_SUM_COLUMNS, EP_COL_DURATION + k % EP_SUM_COLUMNS)], t_sum[k]);
      gs_stats_out<LBFT_EPOCH_STATS>(s_stat, stats, g);
    }
    __syncthreads();  // (before the next pass clears the histogram)
  }
}

extern "C" {

// The caller zeroed all three outputs.
__attribute__((visibility("default"))) hipError_t lbft_ps_launch_epochs(const Params* p, const u32* state, const u32* grp_inst, const u32* grp_off, u32 n_groups,
                                                                       u32 max_group, u32 bin_width, u32 bins, u32 epoch_bins,
                                                                       unsigned long long* handover_hist, unsigned long long* epoch_table,
                                                                       unsigned long long* stats, hipStream_t stream) {
  if (bin_width == 0 || bins == 0 || epoch_bins == 0 || epoch_bins > EP_MAX_BINS || n_groups == 0 || max_group == 0 || p->n == 0 || p->n > LBFT_MAX_NODES ||
      !handover_hist || !epoch_table || !stats)
    return hipErrorInvalidValue;
  // (an instance of the largest group gives at most bcap >= lcap samples to a bin of the histogram or a counting cell of the table)
  const u64 gx = gs_workgroups(EP_WORKGROUPS, n_groups, ((u64)max_group + EP_WAVES - 1) / EP_WAVES, (u64)max_group * p->bcap);
  lbft_k_ps_epochs<<<dim3((u32)gx, n_groups), EP_BLOCK, 0, stream>>>(*p, state, grp_inst, grp_off, bin_width, bins, epoch_bins, handover_hist, epoch_table, stats);
  return hipGetLastError();
}

// The caller zeroed all four outputs.
__attribute__((visibility("default"))) hipError_t lbft_ps_launch_votes(const Params* p, const u32* state, const u32* grp_inst, const u32* grp_off, u32 n_groups,
                                                                      u32 max_group, u32 bin_width, u32 bins, unsigned long long* margin_hist,
                                                                      unsigned long long* votes_hist, unsigned long long* node_table,
                                                                      unsigned long long* stats, hipStream_t stream) {
  if (bin_width == 0 || bins == 0 || n_groups == 0 || max_group == 0 || p->n == 0 || p->n > LBFT_MAX_NODES || !margin_hist || !votes_hist || !node_table || !stats)
    return hipErrorInvalidValue;
  // (an instance of the largest group gives at most bcap >= lcap samples to a bin of a histogram or a cell of the node table)
  const u64 gx = gs_workgroups(VT_WORKGROUPS, n_groups, ((u64)max_group + VT_WAVES - 1) / VT_WAVES, (u64)max_group * p->bcap);
  lbft_k_ps_votes<<<dim3((u32)gx, n_groups), VT_BLOCK, 0, stream>>>(*p, state, grp_inst, grp_off, bin_width, bins, margin_hist, votes_hist, node_table, stats);
  return hipGetLastError();
}

// stats == NULL: the rows alone (lbft_batch_instance_load); else the grouped outputs, all three (rows may be NULL).
__attribute__((visibility("default"))) hipError_t lbft_ps_launch_load(const Params* p, const u32* state, const u32* grp_inst, const u32* grp_off, u32 n_groups,
                                                                     u32 max_group, u32 hist_family, u32 bin_width, u32 bins, unsigned long long* hist,
                                                                     unsigned long long* faults, unsigned long long* stats, u32* rows, hipStream_t stream) {
  if (n_groups == 0 || max_group == 0 || hist_family >= LD_FAMILIES || bin_width == 0 || bins == 0) return hipErrorInvalidValue;
  if (stats ? !hist || !faults : !rows || hist || faults || bins != 1) return hipErrorInvalidValue;
  lbft_k_ps_load<<<dim3((u32)ld_workgroups(n_groups, max_group), n_groups), LD_BLOCK, 0, stream>>>(*p, state, grp_inst, grp_off, hist_family, bin_width, bins, hist,
                                                                                                    faults, stats, rows);
  return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t lbft_ps_launch_counters(const Params* p, const u32* state, unsigned long long* counters, hipStream_t stream) {
  const u32 per_group = 64 * LBFT_COUNTER_WAVES;
  lbft_k_ps_counters<<<(p->m + per_group - 1) / per_group, per_group, 0, stream>>>(*p, state, counters);
  return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t lbft_ps_launch_init(const Params* p, u32* state, const u64* seeds, const ParamSetDev* sets, const u8* set_of,
                                                                     u32 grid, hipStream_t stream) {
  lbft_k_ps_init<<<grid, LBFT_BLOCK, 0, stream>>>(*p, state, seeds, sets, set_of);
  return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t lbft_ps_launch_run(int cls, const Params* p, u32* state, u32* unfinished, const ParamSetDev* sets,
                                                                    const u8* set_of, u32 grid, u32 block, size_t lds_bytes, hipStream_t stream) {
  if (cls != K_SMALL && cls != K_MID) return hipErrorInvalidValue;
  return launch_run_kernel(cls == K_SMALL ? lbft_k_ps_run0 : lbft_k_ps_run1, grid, block, lds_bytes, stream, *p, state, unfinished, sets, set_of);
}

}  // extern "C"
