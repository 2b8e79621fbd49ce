// lbft_vote_rules.h -- the arithmetic of the vote statistics (lbft_batch_vote_stats, include/lbft.h): how the voter sets of the
// committed chain and the block pool of one instance turn into samples.  Compiled by the device kernel (lbft_k_ps_votes,
// lbft_paramsets.hip) and by a plain C++ host shim (tests/vote_stats_host_model.cpp), so the CPU tests check the same code the GPU
// runs.  Needs nothing but <stdint.h> and lbft_group_stats.h, which says what becomes of a sample.
//
// The chain of an instance is that of the chain statistics (lbft_chain_rules.h): the log of the reference node, b_k = log[ref][k].
// Every block record carries its round, its epoch, its author, its ledger depth and the voter set V of its quorum certificate (empty:
// the block has none).  The chain's entries are looked at one by one (votes, weight, margin, who voted) and in pairs of neighbours
// (skipped rounds), the pool's blocks one by one (on the chain, orphaned or pending; certified or not).  Entries and blocks are taken
// `chunk` at a time (the kernel: the 64 lanes of a wavefront); what a chunk needs of its predecessor -- the last entry's round and
// epoch -- is carried.
#ifndef LBFT_VOTE_RULES_H
#define LBFT_VOTE_RULES_H

#include <stdint.h>

#include "lbft_group_stats.h"  // LBFT_HD; GsStat / gs_bin: what becomes of a sample

// The sample families.  LBFT_VOTE_STATS = these 8 x GsStat's 4 words.
enum { VT_VOTES = 0, VT_WEIGHT = 1, VT_MARGIN = 2, VT_SKIPPED = 3, VT_BLOCKS = 4, VT_ORPHANED = 5, VT_PENDING = 6, VT_CERTIFIED_OFF = 7, VT_FAMILIES = 8 };
// The columns of the node table, and the cell of (author, column) in a group's part of it.
enum { VT_COL_PROPOSED = 0, VT_COL_ORPHANED = 1, VT_COL_VOTED = 2, VT_NODE_COLUMNS = 3 };
LBFT_HD uint32_t vt_node_cell(uint32_t author, uint32_t column) { return author * VT_NODE_COLUMNS + column; }

// The voting rights of epoch e: author a holds rights[vt_right_index(a, vt_rights_shift(e, rot, n), n)] (fin_rights_shift's rule with
// the block's own epoch for k / commands_per_epoch; rot == 0: the reference, no rotation).  a < n and shift < n.
LBFT_HD uint32_t vt_rights_shift(uint32_t epoch, uint32_t rot, uint32_t n) { return rot ? (uint32_t)(((uint64_t)epoch * rot) % n) : 0u; }
LBFT_HD uint32_t vt_right_index(uint32_t author, uint32_t shift, uint32_t n) { const uint32_t x = author + shift; return x >= n ? x - n : x; }

// What the voters' rights leave above the quorum (a certificate holds at least the quorum: 0 is the least).
LBFT_HD uint32_t vt_margin(uint32_t weight, uint32_t quorum) { return weight > quorum ? weight - quorum : 0u; }

// A chain entry and its predecessor of the same epoch: the rounds between them that put nothing on the chain (rounds rise strictly
// within an epoch; a pair of two epochs gives no sample: rounds start again).
LBFT_HD bool vt_same_epoch(uint32_t epoch_prev, uint32_t epoch) { return epoch_prev == epoch; }
LBFT_HD uint32_t vt_skipped(uint32_t round_prev, uint32_t round) { return round > round_prev ? round - round_prev - 1u : 0u; }

// Chain membership of pool block b by one dependent gather: a block of ledger depth d can only be entry d - 1 of the chain, so b is
// on the chain of length L iff 1 <= d <= L and log[ref][d - 1] == b.  vt_chain_slot: the entry to gather, or L (none: nothing is read).
LBFT_HD uint32_t vt_chain_slot(uint32_t depth, uint32_t L) { return depth - 1u < L ? depth - 1u : L; }
LBFT_HD bool vt_member(uint32_t slot, uint32_t L, uint32_t entry_at_slot, uint32_t b) { return slot < L && entry_at_slot == b; }

// A pool block that is no chain entry: orphaned when its (epoch, round) is not above the tip's -- the chain has passed it, it can
// never commit -- and pending otherwise.  Without a tip (L == 0) every block is pending.
enum { VT_ON_CHAIN = 0, VT_ORPHAN = 1, VT_PENDING_BLOCK = 2 };
LBFT_HD bool vt_not_above(uint32_t epoch, uint32_t round, uint32_t tip_epoch, uint32_t tip_round) {
  return epoch < tip_epoch || (epoch == tip_epoch && round <= tip_round);
}
LBFT_HD uint32_t vt_classify(bool member, bool has_tip, uint32_t epoch, uint32_t round, uint32_t tip_epoch, uint32_t tip_round) {
  return member ? (uint32_t)VT_ON_CHAIN : (has_tip && vt_not_above(epoch, round, tip_epoch, tip_round)) ? (uint32_t)VT_ORPHAN : (uint32_t)VT_PENDING_BLOCK;
}

#endif  // LBFT_VOTE_RULES_H
