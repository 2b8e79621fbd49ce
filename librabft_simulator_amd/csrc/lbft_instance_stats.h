// lbft_instance_stats.h -- the arithmetic of the per-instance statistics (lbft_batch_instance_stats, include/lbft.h): the samples of the
// latency histogram, the commit stalls and the commit finality, kept per instance instead of per group -- what those calls would report
// if every instance were a group of its own.  The samples themselves are made by the rule headers (lbft_commit_timeline.h,
// lbft_commit_finality.h, lbft_chain_rules.h); here is what becomes of them: the eleven families of a row, the accumulator of one
// family, how an entry's column and a node's closed row add to it, and the launcher's grid rule.  Compiled by the device kernel
// (lbft_k_ct_instances, lbft_commit_times.hip) and by a plain C++ host shim (tests/instance_stats_host.cpp), so the CPU tests check the
// same code the GPU runs.  Needs nothing of the device.
#ifndef LBFT_INSTANCE_STATS_H
#define LBFT_INSTANCE_STATS_H

#include <stdint.h>

#include "lbft_chain_rules.h"
#include "lbft_commit_finality.h"
#include "lbft_commit_timeline.h"
#include "lbft_group_stats.h"  // LBFT_HD; gs_workgroups

// The families of a row, rows[i * IST_WORDS + 4 * family + {samples, sum, min, max}]: the latency, then lbft_batch_commit_stalls' four
// (IST_STALLS + CTL_*), then lbft_batch_commit_finality's six (IST_FINALITY + FIN_*).
enum { IST_LATENCY = 0, IST_STALLS = 1, IST_FINALITY = IST_STALLS + CTL_FAMILIES, IST_FAMILIES = IST_FINALITY + FIN_FAMILIES, IST_WORDS = IST_FAMILIES * 4 };

// One family of one instance as it is accumulated.  An instance gives a family at most nodes x log capacity < 2^32 samples, each
// below 2^31: the count and the extremes are 32-bit.  The minimum is kept as itself (0xffffffff without samples), not as GsStat's
// complement: a row has one writer and is never combined by atomics.
struct IstStat {
  uint32_t cnt, min, max;
  uint64_t sum;
};
LBFT_HD IstStat ist_empty() {
  IstStat s;
  s.cnt = 0; s.min = 0xffffffffu; s.max = 0; s.sum = 0;
  return s;
}
LBFT_HD void ist_add(IstStat& s, uint32_t v) {
  s.cnt++; s.sum += v;
  s.min = v < s.min ? v : s.min;
  s.max = v > s.max ? v : s.max;
}
LBFT_HD IstStat ist_merge(const IstStat& a, const IstStat& b) {
  IstStat r;
  r.cnt = a.cnt + b.cnt; r.sum = a.sum + b.sum;
  r.min = a.min < b.min ? a.min : b.min;
  r.max = a.max > b.max ? a.max : b.max;
  return r;
}
// Word w of the family as the row holds it: samples, sum, min, max; min = max = 0 without samples.
LBFT_HD uint64_t ist_word(const IstStat& s, uint32_t w) { return w == 0 ? s.cnt : w == 1 ? s.sum : w == 2 ? (s.cnt ? s.min : 0u) : s.max; }

// The latency of an entry a node committed at c: after the global proposal time g of the block in the node's own log.
LBFT_HD uint32_t ist_latency(int32_t c, int32_t g) { return (uint32_t)c - (uint32_t)g; }

// What the column of entry k gives the finality families (st = the row's IST_FAMILIES accumulators, g = the entry's proposal time);
// returns 1 if the entry is open.
LBFT_HD uint32_t ist_column(IstStat* st, const FinEntry& e, uint32_t n, int32_t g) {
  fin_samples(e, n, g, [&](uint32_t family, uint32_t v) { ist_add(st[IST_FINALITY + family], v); });
  return fin_open(e) ? 1u : 0u;
}
// What a node's whole row gives the stall families: first (if any), tail, longest -- one sample each.
LBFT_HD void ist_node(IstStat* st, const CtlRow& row, int32_t max_clock) {
  if (row.first != LBFT_CTL_NONE) ist_add(st[IST_STALLS + CTL_FIRST], row.first);
  ist_add(st[IST_STALLS + CTL_TAIL], ctl_tail(row, max_clock));
  ist_add(st[IST_STALLS + CTL_LONGEST], ctl_longest(row, max_clock));
}

// The launcher's grid rule: workgroups per group (gridDim.x) of IST_WAVES wavefronts, one instance per wavefront at a time.  About
// IST_WORKGROUPS workgroups in all, never more than a group's stride has steps: above IST_WORKGROUPS / groups * IST_WAVES instances in
// the largest group a wavefront takes a second instance.  (No LDS histogram: no floor from a sample count.)
#define IST_WAVES 4u
#define IST_WORKGROUPS 1024u
LBFT_HD uint64_t ist_workgroups(uint64_t n_groups, uint64_t max_group) {
  return gs_workgroups(IST_WORKGROUPS, n_groups, (max_group + IST_WAVES - 1) / IST_WAVES, 0);
}

#endif  // LBFT_INSTANCE_STATS_H
