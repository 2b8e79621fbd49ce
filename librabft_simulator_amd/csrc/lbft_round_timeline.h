// lbft_round_timeline.h -- the arithmetic of the round statistics (lbft_batch_round_stats, include/lbft.h): how the cells of one
// instance's round-switch table turn into samples.  Compiled by the device kernel (lbft_k_rs_rounds, lbft_round_stats.hip) and by a
// plain C++ host shim (tests/round_stats_host.cpp), so the CPU tests check the same code the GPU runs.  Needs nothing but <stdint.h> and
// lbft_group_stats.h, which says what becomes of a sample.
//
// The table of an instance is T[r][j], r in [0, rows), rows = min(max_j max_round[j], trace capacity): the row of the highest round
// reached is not part of it (data_writer.rs:74-75), although the device stores that cell too.  A cell is the GlobalTime at which node j
// was first seen in round r, or empty.  A node's non-empty cells are looked at in pairs of neighbours -- a cell and its nearest
// non-empty predecessor in the node's row (rtl_pair): stay and skipped --, a round's cells together (RtlRound): skew and reach.  Each
// sample needs nothing else, so any assignment of cells to lanes gives the same sums.
#ifndef LBFT_ROUND_TIMELINE_H
#define LBFT_ROUND_TIMELINE_H

#include <stdint.h>

#include "lbft_group_stats.h"  // LBFT_HD; GsStat / gs_bin: what becomes of a sample

#define LBFT_RTL_EMPTY 0xffffffffu  // an empty cell as the device stores it (a GlobalTime is a non-negative i32)
#define LBFT_RTL_NO_ROUND 0xffffffffu  // "no predecessor" (a round index is below the trace capacity)

// Rows of the table: the rounds below the highest round any node reached, as far as the trace holds them.
LBFT_HD uint32_t rtl_rows(uint32_t highest_round, uint32_t capacity) { return highest_round < capacity ? highest_round : capacity; }
// The cell of row r as the statistics see it: what lies at or past `rows` (the stored cell of the highest round) reads as empty.
LBFT_HD uint32_t rtl_cell(uint32_t stored, uint32_t r, uint32_t rows) { return r < rows ? stored : LBFT_RTL_EMPTY; }
LBFT_HD bool rtl_empty(uint32_t cell) { return cell == LBFT_RTL_EMPTY; }

// A non-empty cell (round r, time t) of a node's row and its nearest non-empty predecessor (round pr < r, time pt; pr ==
// LBFT_RTL_NO_ROUND: the node's first recorded round, no sample): stay = the time between the two, skipped = the rounds jumped over.
LBFT_HD bool rtl_pair(uint32_t t, uint32_t r, uint32_t pt, uint32_t pr, uint32_t& stay, uint32_t& skipped) {
  if (rtl_empty(t) || pr == LBFT_RTL_NO_ROUND) return false;
  stay = t - pt;  // (the event clock never goes back: >= 0, and 0 does occur)
  skipped = r - pr - 1u;
  return true;
}

// The non-empty cells of one round: earliest, latest, how many.
struct RtlRound {
  uint32_t first, last, cells;
};
LBFT_HD RtlRound rtl_round_empty() {
  RtlRound q;
  q.first = LBFT_RTL_EMPTY; q.last = 0; q.cells = 0;
  return q;
}
LBFT_HD void rtl_round_add(RtlRound& q, uint32_t cell) {
  if (rtl_empty(cell)) return;
  q.first = cell < q.first ? cell : q.first;
  q.last = cell > q.last ? cell : q.last;
  q.cells++;
}
// skew: a sample for a row of the table with at least two cells.  reach: a sample for every row but row 0 (always empty: nodes start in
// round 1), also when it holds no cell.
LBFT_HD bool rtl_skew(const RtlRound& q, uint32_t r, uint32_t rows, uint32_t& skew) {
  if (r >= rows || q.cells < 2u) return false;
  skew = q.last - q.first;
  return true;
}
LBFT_HD bool rtl_reach(const RtlRound& q, uint32_t r, uint32_t rows, uint32_t& reach) {
  if (r == 0 || r >= rows) return false;
  reach = q.cells;
  return true;
}

// The sample families.  LBFT_ROUND_STATS = these 4 x GsStat's 4 words.
enum { RTL_STAY = 0, RTL_SKIPPED = 1, RTL_SKEW = 2, RTL_REACH = 3, RTL_FAMILIES = 4 };

#endif  // LBFT_ROUND_TIMELINE_H
