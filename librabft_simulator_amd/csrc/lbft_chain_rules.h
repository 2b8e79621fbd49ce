// lbft_chain_rules.h -- the arithmetic of the chain statistics (lbft_batch_chain_stats, include/lbft.h): how the commit logs of one
// instance turn into samples.  Compiled by the device kernel (lbft_k_cs_chain, lbft_chain_stats.hip) and by a plain C++ host shim
// (tests/chain_stats_host.cpp), so the CPU tests check the same code the GPU runs.  Needs nothing but <stdint.h> and
// lbft_group_stats.h, which says what becomes of a sample.
//
// The chain of an instance is the log of its reference node: the lowest-numbered node with the largest (clamped) commit count.  Entry
// k of the chain has an author a_k and a global proposal time g_k.  The entries are looked at in pairs of neighbours (interval,
// inversion), in maximal runs of one author (tenure) and one by one (authors; against the other nodes' logs: differing).  Entries are
// taken `chunk` at a time (the kernel: the 64 lanes of a wavefront); what a chunk needs of its predecessors -- the last entry's time
// and author, the index at which the current run began -- is carried.
#ifndef LBFT_CHAIN_RULES_H
#define LBFT_CHAIN_RULES_H

#include <stdint.h>

#include "lbft_group_stats.h"  // LBFT_HD; GsStat / gs_bin: what becomes of a sample

// The reference-node order: nodes are compared by (commit count, ~index) and the largest wins, so that a tie goes to the lowest
// index.  A lane without a node holds 0, which every node beats (~index is never 0 for an index below 2^32 - 1).
LBFT_HD uint64_t chn_ref_key(uint32_t commits, uint32_t node) { return ((uint64_t)commits << 32) | (uint32_t)~node; }
LBFT_HD uint64_t chn_ref_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
LBFT_HD uint32_t chn_ref_len(uint64_t key) { return (uint32_t)(key >> 32); }
LBFT_HD uint32_t chn_ref_node(uint64_t key) { return ~(uint32_t)key; }
// nc_j: a log holds at most its capacity.
LBFT_HD uint32_t chn_commits(uint32_t commit_count, uint32_t log_capacity) { return commit_count < log_capacity ? commit_count : log_capacity; }

// Entry k >= 1 and its predecessor (global proposal times g and g_prev, each a GlobalTime in [0, max_clock]): the interval between
// them, clamped at 0 where the successor was proposed earlier -- that pair is an inversion.
LBFT_HD uint32_t chn_interval(int32_t g_prev, int32_t g) { return g < g_prev ? 0u : (uint32_t)g - (uint32_t)g_prev; }
LBFT_HD bool chn_inverted(int32_t g_prev, int32_t g) { return g < g_prev; }

// Entry k begins a run of its author: the first entry, or another author than its predecessor's.
LBFT_HD bool chn_run_start(uint32_t k, uint32_t author, uint32_t author_prev) { return k == 0 || author != author_prev; }
// A run start at k > 0 ends the run before it, whose length is k - the previous start: the highest start among the chunk's lanes
// below this one (starts_below = the ballot of the chunk's run starts, masked to the lanes below; chunk_first = the index of lane 0),
// or else the start carried in from the earlier chunks.
LBFT_HD uint32_t chn_highest(uint64_t mask) { return 63u - (uint32_t)__builtin_clzll(mask); }  // (mask != 0)
LBFT_HD uint32_t chn_tenure(uint32_t k, uint64_t starts_below, uint32_t chunk_first, uint32_t carried_start) {
  return k - (starts_below ? chunk_first + chn_highest(starts_below) : carried_start);
}
// The start carried out of a chunk; after the last chunk the run still open has L - that start entries (L >= 1).
LBFT_HD uint32_t chn_carry_start(uint64_t starts, uint32_t chunk_first, uint32_t carried_start) {
  return starts ? chunk_first + chn_highest(starts) : carried_start;
}

// The sample families.  LBFT_CHAIN_STATS = these 6 x GsStat's 4 words.
enum { CHN_INTERVAL = 0, CHN_LENGTH = 1, CHN_LAG = 2, CHN_TENURE = 3, CHN_DIFFERING = 4, CHN_INVERSIONS = 5, CHN_FAMILIES = 6 };

#endif  // LBFT_CHAIN_RULES_H
