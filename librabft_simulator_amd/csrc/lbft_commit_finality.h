// lbft_commit_finality.h -- the arithmetic of commit finality (lbft_batch_commit_finality, include/lbft.h): how the commit times that
// the nodes of one instance recorded for ONE entry of the chain turn into the times at which the entry is final -- committed by the
// first node, by nodes holding `valid` and `quorum` voting rights, by every node.  Compiled by the device kernel (lbft_k_ct_finality,
// lbft_commit_times.hip) and by a plain C++ host shim (tests/commit_finality_host.cpp), so the CPU tests check the same code the GPU
// runs.  Needs nothing but <stdint.h> and lbft_group_stats.h, which says what becomes of a sample.
//
// An entry's column is the n commit times c_j(k), one per node, read as col[j * stride]: the kernel's column of its [n][64] LDS tile
// (stride 64), the shim's chunk buffer (stride = chunk).  A node that is no committer of the entry holds FIN_NONE in the column: whoever
// fills it applies fin_committer.  The thresholds are found by rank counting, without a sort: for every committer j, the voting rights
// of the committers with a time <= c_j(k) -- nodes with equal times count together --, and the threshold's time is the smallest c_j(k)
// whose rank weight reaches it.  n^2 reads of the column.
#ifndef LBFT_COMMIT_FINALITY_H
#define LBFT_COMMIT_FINALITY_H

#include <stdint.h>

#include "lbft_group_stats.h"  // LBFT_HD; GsStat / gs_bin: what becomes of a sample

#define FIN_NONE (-1)  // no time: a node that is no committer, a threshold the committers do not reach

// The sample families.  LBFT_FINALITY_STATS = these 6 x GsStat's 4 words.
enum { FIN_FIRST = 0, FIN_VALID = 1, FIN_QUORUM = 2, FIN_ALL = 3, FIN_SPREAD = 4, FIN_OPEN = 5, FIN_FAMILIES = 6 };

// commands_per_epoch as the 32-bit divisor of an entry index (k < 2^32 - 1: every larger value gives epoch 0 as well).
LBFT_HD uint32_t fin_cpe32(uint64_t commands_per_epoch) { return commands_per_epoch > 0xffffffffull ? 0xffffffffu : (uint32_t)commands_per_epoch; }
// The shift of the voting rights at entry k, ((k / cpe) * rot) % n, and node j's place in the rights table, (j + e_k * rot) % n with
// e_k = k / cpe (rights_rotation, include/lbft.h).  32-bit arithmetic: k is below the log capacity (< 2^16), so e_k < 2^16; rot < n and
// j < n <= 2^7: e_k * rot < 2^23, and j + shift < 2n needs one subtraction, no second division.
LBFT_HD uint32_t fin_rights_shift(uint32_t k, uint32_t cpe, uint32_t rot, uint32_t n) { return rot ? ((k / cpe) * rot) % n : 0u; }
LBFT_HD uint32_t fin_rights_index(uint32_t j, uint32_t shift, uint32_t n) { return j + shift >= n ? j + shift - n : j + shift; }

// Node j is a committer of entry k: the entry lies below its (clamped) commit count and its commit time was recorded.
LBFT_HD bool fin_committer(uint32_t k, uint32_t commits, int32_t commit_time) { return k < commits && commit_time >= 0; }

// What one column gives.  first / last: the smallest / largest time of a committer; first_node: the lowest-numbered committer with the
// smallest time (n without a committer); committers: how many; valid / quorum: the smallest t such that the committers with a time
// <= t hold at least t_valid / t_quorum voting rights, FIN_NONE when all committers together hold less.
struct FinEntry {
  int32_t first, last, valid, quorum;
  uint32_t first_node, committers;
};
// rights: the table of n voting rights, node j holding rights[fin_rights_index(j, shift, n)]; NULL = every right is 1.
LBFT_HD FinEntry fin_entry(const int32_t* col, uint32_t stride, uint32_t n, const uint32_t* rights, uint32_t shift, uint32_t t_valid, uint32_t t_quorum) {
  FinEntry e = {FIN_NONE, FIN_NONE, FIN_NONE, FIN_NONE, n, 0u};
  for (uint32_t j = 0; j < n; j++) {
    const int32_t cj = col[j * stride];
    if (cj < 0) continue;
    e.committers++;
    if (e.first < 0 || cj < e.first) { e.first = cj; e.first_node = j; }  // (strictly smaller: a tie stays with the lower number)
    if (cj > e.last) e.last = cj;
    uint32_t weight = 0;  // of the committers that committed no later than j: at most total_votes < 2^32
    for (uint32_t i = 0; i < n; i++) {
      const int32_t ci = col[i * stride];
      if (ci >= 0 && ci <= cj) weight += rights ? rights[fin_rights_index(i, shift, n)] : 1u;
    }
    if (weight >= t_valid && (e.valid < 0 || cj < e.valid)) e.valid = cj;
    if (weight >= t_quorum && (e.quorum < 0 || cj < e.quorum)) e.quorum = cj;
  }
  return e;
}
// The `all` time: defined when every node is a committer, and then the latest commit.
LBFT_HD int32_t fin_all(const FinEntry& e, uint32_t n) { return e.committers == n ? e.last : FIN_NONE; }
// The thresholds of `valid` (so many rights that at least one honest node is among their holders) and of the entry counted as open.
LBFT_HD uint32_t fin_valid_threshold(uint32_t total_votes, uint32_t quorum) { return total_votes - quorum + 1u; }
LBFT_HD bool fin_open(const FinEntry& e) { return e.committers != 0 && e.quorum < 0; }
// A sample: a time of the entry after its proposal time g_k, or after its first commit.  Nothing is clamped: a time before its origin
// would show as a sample above max_clock (the tests' reference asserts that there is none).
LBFT_HD uint32_t fin_after(int32_t t, int32_t origin) { return (uint32_t)t - (uint32_t)origin; }
// The samples an entry gives the families first .. spread, each with its guard: f(family, sample), in the families' order.  g = the
// entry's proposal time.  (The sixth family, FIN_OPEN, is one sample per instance: the count of its fin_open entries.)
template <class F>
LBFT_HD void fin_samples(const FinEntry& e, uint32_t n, int32_t g, F&& f) {
  const int32_t all = fin_all(e, n);
  if (e.committers) f(FIN_FIRST, fin_after(e.first, g));
  if (e.valid >= 0) f(FIN_VALID, fin_after(e.valid, g));
  if (e.quorum >= 0) f(FIN_QUORUM, fin_after(e.quorum, g));
  if (all >= 0) { f(FIN_ALL, fin_after(all, g)); f(FIN_SPREAD, fin_after(all, e.first)); }
}

#endif  // LBFT_COMMIT_FINALITY_H
