// lbft_commit_timeline.h -- the arithmetic of the commit timelines (lbft_batch_commit_series / lbft_batch_commit_stalls, include/lbft.h):
// how one node's row of recorded commit times turns into samples.  Compiled by the device kernel (lbft_k_ct_timeline,
// lbft_commit_times.hip) and by a plain C++ host shim (tests/commit_timeline_host.cpp), so the CPU tests check the same code the GPU runs.
// Needs nothing but <stdint.h> and lbft_group_stats.h, which says what becomes of a sample.
//
// A row c[0 .. nc) is non-negative and non-decreasing.  Its commit instants t_1 < ... < t_r are its distinct values; they cut
// [0, max_clock] into r + 1 intervals: the leading one [0, t_1], the gaps t_{s+1} - t_s, and the tail max_clock - t_r.  Each entry is
// looked at with its predecessor alone (ctl_entry), and what a row needs beyond its gap samples -- the longest interval, the last
// instant, the first instant at or after `since` -- is a maximum or a minimum over its entries, so partial results of pieces of a row
// combine in any order (ctl_merge): the kernel spreads a row over the lanes of a wavefront segment, the host shim walks it in order.
#ifndef LBFT_COMMIT_TIMELINE_H
#define LBFT_COMMIT_TIMELINE_H

#include <stdint.h>

#include "lbft_group_stats.h"  // LBFT_HD; GsStat / gs_bin: what becomes of a sample

#define LBFT_CTL_NONE 0xffffffffu  // "no instant at or after since" (every real distance is <= max_clock < 2^31)

// What a piece of a row has seen so far.
struct CtlRow {
  uint32_t longest;  // the longest interval that ends at one of the piece's instants (the leading interval and the gaps)
  int32_t last;      // its last instant, -1 = none
  uint32_t first;    // the smallest (instant - since) over its instants >= since, LBFT_CTL_NONE = none
};
LBFT_HD CtlRow ctl_empty() {
  CtlRow r;
  r.longest = 0; r.last = -1; r.first = LBFT_CTL_NONE;
  return r;
}
// Entry c of a row whose previous entry is prev (-1 for the row's first entry; an entry that was never recorded reads as -1 and is no
// instant).  Returns the gap sample this entry closes, 0 = none (a repeated time, or the row's first instant: gaps are >= 1).
LBFT_HD uint32_t ctl_entry(CtlRow& r, int32_t c, int32_t prev, int32_t since) {
  if (c < 0 || c == prev) return 0u;
  const uint32_t interval = (uint32_t)c - (prev < 0 ? 0u : (uint32_t)prev);  // from the previous instant, or from clock 0
  r.longest = interval > r.longest ? interval : r.longest;
  r.last = c > r.last ? c : r.last;
  if (c >= since) {
    const uint32_t d = (uint32_t)c - (uint32_t)since;
    r.first = d < r.first ? d : r.first;
  }
  return prev < 0 ? 0u : interval;
}
LBFT_HD CtlRow ctl_merge(const CtlRow& a, const CtlRow& b) {
  CtlRow r;
  r.longest = a.longest > b.longest ? a.longest : b.longest;
  r.last = a.last > b.last ? a.last : b.last;
  r.first = a.first < b.first ? a.first : b.first;
  return r;
}
// The whole row's samples: tail = max_clock - t_r, longest = the longest of its r + 1 intervals (both max_clock for a row without
// commits); first is r.first (a sample unless LBFT_CTL_NONE).
LBFT_HD uint32_t ctl_tail(const CtlRow& r, int32_t max_clock) { return (uint32_t)max_clock - (r.last < 0 ? 0u : (uint32_t)r.last); }
LBFT_HD uint32_t ctl_longest(const CtlRow& r, int32_t max_clock) {
  const uint32_t tail = ctl_tail(r, max_clock);
  return r.longest > tail ? r.longest : tail;
}

// The sample families (every sample is a clock difference within [0, max_clock] < 2^31).  LBFT_STALL_STATS = these 4 x GsStat's 4 words.
enum { CTL_GAPS = 0, CTL_FIRST = 1, CTL_TAIL = 2, CTL_LONGEST = 3, CTL_FAMILIES = 4 };

#endif  // LBFT_COMMIT_TIMELINE_H
