// lbft_epoch_rules.h -- the arithmetic of the epoch statistics (lbft_batch_epoch_stats, include/lbft.h): how the epochs of the committed
// chain, of the block pool and of the nodes of one instance turn into samples and into rows of the epoch table.  Compiled by the device
// kernel (lbft_k_ps_epochs, lbft_paramsets.hip) and by a plain C++ host shim (tests/epoch_stats_host_model.cpp), so the CPU tests check
// the same code the GPU runs.  Needs nothing but <stdint.h> and lbft_group_stats.h, which says what becomes of a sample.
//
// The chain of an instance is that of the vote statistics: b_k = log[ref][k] up to the first entry that is no pool index.  Entry k has
// the epoch e_k, the round r_k and the global proposal time g_k of its block.  A segment is a maximal run of entries with equal e_k; the
// last one is open, the others are complete; a boundary is a pair (k - 1, k) with e_{k-1} != e_k.  Nothing here assumes that epochs
// rise, or rise by one.  Entries are taken `chunk` at a time (the kernel: the 64 lanes of a wavefront); what a chunk needs of its
// predecessors -- the last entry's e, r and g, and the index and g of the entry that began the segment open at its end -- is carried.
#ifndef LBFT_EPOCH_RULES_H
#define LBFT_EPOCH_RULES_H

#include <stdint.h>

#include "lbft_group_stats.h"  // LBFT_HD; GsStat / gs_bin: what becomes of a sample

// The sample families.  LBFT_EPOCH_STATS = these 10 x GsStat's 4 words.
enum { EP_SEGMENTS = 0, EP_NODE_EPOCH = 1, EP_BEHIND = 2, EP_LENGTH = 3, EP_DURATION = 4, EP_LAST_ROUND = 5, EP_FIRST_ROUND = 6, EP_HANDOVER = 7,
       EP_STRANDED = 8, EP_BLOCKS = 9, EP_FAMILIES = 10 };
// The columns of the epoch table.  Five count, two (EP_COL_DURATION, EP_COL_HANDOVER) sum times: those need 64-bit accumulators.
enum { EP_COL_SEGMENTS = 0, EP_COL_COMPLETE = 1, EP_COL_ENTRIES = 2, EP_COL_DURATION = 3, EP_COL_HANDOVER = 4, EP_COL_STRANDED = 5, EP_COL_BLOCKS = 6,
       EP_COLUMNS = 7 };
#define EP_MAX_BINS 512u  // LBFT_EPOCH_MAX_BINS

// The table's row of an epoch: the last row also takes every epoch above it.  1 <= epoch_bins.
LBFT_HD uint32_t ep_bin(uint32_t epoch, uint32_t epoch_bins) { return epoch < epoch_bins - 1u ? epoch : epoch_bins - 1u; }
LBFT_HD uint32_t ep_cell(uint32_t row, uint32_t column) { return row * EP_COLUMNS + column; }

// Entry k begins a segment: the first entry, or another epoch than its predecessor's.  A start at k > 0 is a boundary: it ends the
// segment before it.
LBFT_HD bool ep_segment_start(uint32_t k, uint32_t epoch, uint32_t epoch_prev) { return k == 0 || epoch != epoch_prev; }
// Where the segment that a boundary at lane `lane` of a chunk ends began: the highest start among the chunk's lanes below it
// (starts_below = the ballot of the chunk's segment starts, masked to the lanes below), else the start carried in.  ep_start_lane: the
// lane whose g is that segment's first (valid when starts_below != 0).
LBFT_HD uint32_t ep_highest(uint64_t mask) { return 63u - (uint32_t)__builtin_clzll(mask); }  // (mask != 0)
LBFT_HD uint32_t ep_start_lane(uint64_t starts_below) { return starts_below ? ep_highest(starts_below) : 0u; }
LBFT_HD uint32_t ep_segment_first(uint64_t starts_below, uint32_t chunk_first, uint32_t carried_start) {
  return starts_below ? chunk_first + ep_highest(starts_below) : carried_start;
}
// The start carried out of a chunk (`starts`: the whole ballot) and the g that goes with it.
LBFT_HD uint32_t ep_carry_start(uint64_t starts, uint32_t chunk_first, uint32_t carried_start) { return ep_segment_first(starts, chunk_first, carried_start); }

// later - earlier, clamped at 0: a segment's duration (g_last - g_first) and a boundary's handover (g_k - g_{k-1}).  The difference of
// two 32-bit times is taken in 64 bits and is below 2^32.
LBFT_HD uint32_t ep_clamped(int32_t later, int32_t earlier) { return later > earlier ? (uint32_t)((int64_t)later - (int64_t)earlier) : 0u; }

// A pool block is stranded when it is no chain entry and its epoch lies below the tip's: the chain has left its epoch.  Without a tip
// (L == 0) nothing is stranded.
LBFT_HD bool ep_stranded(bool member, bool has_tip, uint32_t epoch, uint32_t tip_epoch) { return !member && has_tip && epoch < tip_epoch; }

#endif  // LBFT_EPOCH_RULES_H
