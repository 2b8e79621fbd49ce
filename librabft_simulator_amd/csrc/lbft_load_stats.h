// lbft_load_stats.h -- the run load of a finished batch (lbft_batch_load_stats, lbft_batch_instance_load; include/lbft.h): how much
// work every instance did and how close it came to each of its capacities, as sixteen u32 samples per instance, one per family.  Here
// are the family table, how a sample comes from the words an instance leaves on the device, the fault census, and -- for the device --
// the reductions over the 16-lane segment that owns an instance.  The first part needs nothing but <stdint.h>: the kernel
// (lbft_k_ps_load, lbft_paramsets.hip) and a plain C++ host shim (tests/load_stats_host.cpp) compile the same arithmetic.
#ifndef LBFT_LOAD_STATS_H
#define LBFT_LOAD_STATS_H

#include <stdint.h>

#include "lbft_group_stats.h"  // LBFT_HD; GsStat, gs_workgroups

// The families, rows[i * LD_FAMILIES + family] and stats[g * LD_WORDS + 4 * family + {samples, sum, min, max}].
enum LoadFamily {
  LD_NOTIFICATIONS = 0, LD_REQUESTS, LD_RESPONSES, LD_TIMERS,  // events by kind
  LD_MESSAGES,                                                 // the first three added (a u32 add)
  LD_SCHEDULED, LD_DRAWS, LD_FOLDED, LD_UPDATES,               // creation stamps, RNG draws, folded timers, update_node calls
  LD_QUEUE, LD_CHUNKS, LD_SNAPSHOTS, LD_BLOCKS,                // high-water marks: event queue, calendar chunk pool, snapshot pool; blocks
  LD_LOG, LD_COMMITS, LD_ROUNDS,                               // over the nodes: largest and smallest commit count, smallest active round
  LD_FAMILIES, LD_WORDS = LD_FAMILIES * 4
};
#define LD_SEGMENT 16u     // lanes per instance: lane f of a segment owns family f
#define LD_FAULT_BITS 32u  // the census counts every bit of the fault word

// The words of an instance that a family's lane reads as they are (LDW_NONE: the family is computed -- messages, and the three
// over the nodes).  The kernel maps them to the instance's rows; the shim is handed them in this order.
enum LoadWord {
  LDW_EV0 = 0, LDW_EV1, LDW_EV2, LDW_EV3, LDW_STAMP, LDW_DRAWS, LDW_NFOLD, LDW_NUPD, LDW_MAXQ, LDW_CAL_BUMP, LDW_MAXSNAP, LDW_NBLOCKS,
  LDW_WORDS, LDW_NONE = LDW_WORDS
};
LBFT_HD uint32_t ld_word_of(uint32_t family) {
  return family < LD_MESSAGES ? LDW_EV0 + family : family == LD_MESSAGES || family >= LD_LOG ? (uint32_t)LDW_NONE : LDW_STAMP + (family - LD_SCHEDULED);
}
// The sample of a family that reads a word: the word itself; the chunk pool's bump pointer only where the batch runs the calendar
// queue (any other queue leaves that word as it found it).
LBFT_HD uint32_t ld_word_sample(uint32_t family, uint32_t word, bool calendar) { return family == LD_CHUNKS && !calendar ? 0u : word; }
// The lane's share of family `messages`: lanes 0 to 2 give their word, the segment adds them.
LBFT_HD uint32_t ld_message_share(uint32_t family, uint32_t sample) { return family < LD_MESSAGES - 1u ? sample : 0u; }

// The three families over the nodes of an instance: a lane takes nodes f, f + 16, ...; the lanes' parts are merged.
struct LdNodes {
  uint32_t log, commits, rounds;  // max commit count (unclamped: past the log capacity after an overflow), min commit count, min active round
};
LBFT_HD LdNodes ld_nodes_empty() {
  LdNodes a;
  a.log = 0; a.commits = 0xffffffffu; a.rounds = 0xffffffffu;
  return a;
}
LBFT_HD void ld_nodes_add(LdNodes& a, uint32_t commits, uint32_t round) {
  a.log = commits > a.log ? commits : a.log;
  a.commits = commits < a.commits ? commits : a.commits;
  a.rounds = round < a.rounds ? round : a.rounds;
}
LBFT_HD LdNodes ld_nodes_merge(const LdNodes& a, const LdNodes& b) {
  LdNodes r;
  r.log = a.log > b.log ? a.log : b.log;
  r.commits = a.commits < b.commits ? a.commits : b.commits;
  r.rounds = a.rounds < b.rounds ? a.rounds : b.rounds;
  return r;
}
LBFT_HD uint32_t ld_nodes_sample(uint32_t family, const LdNodes& a) { return family == LD_LOG ? a.log : family == LD_COMMITS ? a.commits : a.rounds; }

// What lane `family` holds once its segment has merged: its word's sample, the segment's message sum, or its family over the nodes.
LBFT_HD uint32_t ld_sample(uint32_t family, uint32_t word_sample, uint32_t messages, const LdNodes& nodes) {
  return family == LD_MESSAGES ? messages : family >= LD_LOG ? ld_nodes_sample(family, nodes) : word_sample;
}

// The census counts every instance with bit k in its fault word; the statistics and the histogram take the instances without any.
LBFT_HD bool ld_fault_bit(uint32_t fault, uint32_t k) { return (fault >> k) & 1u; }
LBFT_HD bool ld_clean(uint32_t fault) { return fault == 0; }

// The launcher's grid rule: workgroups per group (gridDim.x) of LD_BLOCK threads = LD_BLOCK / LD_SEGMENT instances at a time.  A
// group's histogram gets one sample per instance.
#define LD_BLOCK 256u
#define LD_WORKGROUPS 1024u
#define LD_LDS_BINS 8192u  // 32 KiB of u32 counts per pass
LBFT_HD uint64_t ld_workgroups(uint64_t n_groups, uint64_t max_group) {
  const uint64_t per = LD_BLOCK / LD_SEGMENT;
  return gs_workgroups(LD_WORKGROUPS, n_groups, (max_group + per - 1) / per, max_group);
}

#if defined(__HIPCC__)
// ---- the segment: 16 consecutive lanes of a wavefront (xor distances below 16 stay inside it).  Every lane of the wavefront calls. ----
__device__ __forceinline__ uint32_t ld_segment_sum(uint32_t v) {
  for (int d = LD_SEGMENT / 2; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}
__device__ __forceinline__ LdNodes ld_segment_merge(LdNodes a) {
  for (int d = LD_SEGMENT / 2; d; d >>= 1) {
    LdNodes o;
    o.log = (uint32_t)__shfl_xor((int)a.log, d, 64);
    o.commits = (uint32_t)__shfl_xor((int)a.commits, d, 64);
    o.rounds = (uint32_t)__shfl_xor((int)a.rounds, d, 64);
    a = ld_nodes_merge(a, o);
  }
  return a;
}
// The statistics: every lane carries ONE GsStat, its family's over the workgroup's whole stride.  The wavefront's four segments are
// combined over the distances 32 and 16; lanes 0 to 15 then add their family to the workgroup's s_stat[LD_WORDS] (gs_stats_clear
// before, a barrier and gs_stats_out<LD_WORDS> after: lbft_group_stats.h's scheme).
__device__ __forceinline__ void ld_reduce_to_lds(const GsStat& st, unsigned long long* s_stat, uint32_t lane) {
  unsigned long long cnt = st.cnt, sum = st.sum, nmin = st.nmin, max = st.max;
  for (int d = 32; d >= (int)LD_SEGMENT; d >>= 1) {
    cnt += __shfl_xor(cnt, d, 64);
    sum += __shfl_xor(sum, d, 64);
    const unsigned long long on = __shfl_xor(nmin, d, 64), om = __shfl_xor(max, d, 64);
    nmin = on > nmin ? on : nmin;
    max = om > max ? om : max;
  }
  if (lane < LD_SEGMENT && cnt) {
    atomicAdd(&s_stat[lane * 4 + 0], cnt); atomicAdd(&s_stat[lane * 4 + 1], sum);
    atomicMax(&s_stat[lane * 4 + 2], nmin); atomicMax(&s_stat[lane * 4 + 3], max);
  }
}
#endif  // __HIPCC__

#endif  // LBFT_LOAD_STATS_H
