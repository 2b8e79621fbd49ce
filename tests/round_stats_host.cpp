// TEST INFRASTRUCTURE: host shim over lbft_round_timeline.h, the arithmetic lbft_k_rs_rounds turns an instance's round-switch trace into
// samples with.  It takes the trace as the device holds it -- first_time[instance][node][rcap] u32 with 0xffffffff = empty, and
// max_round[instance][node] -- and walks it the way the kernel does: node-major, `chunk` rounds of a node's row side by side, each
// lane finding its nearest non-empty predecessor among the lanes below it and otherwise taking the one carried from the previous
// chunks; then round-major, each round's cells over the nodes.  Plain loops in place of the wavefront; chunk = 1 is a plain walk.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../librabft_simulator_amd/csrc/lbft_round_timeline.h"

extern "C" int rtl_host(const uint32_t* first_time, const uint32_t* max_round, const uint32_t* faults, const uint32_t* group_of, uint32_t m,
                        uint32_t n, uint32_t rcap, uint32_t groups, uint32_t width, uint32_t bins, uint32_t chunk, uint64_t* stay_hist,
                        uint64_t* skew_hist, uint64_t* stats) {
  if (!width || !bins || !chunk || !groups || !rcap) return -1;
  std::vector<GsStat> st((size_t)groups * RTL_FAMILIES, GsStat{0, 0, 0, 0});
  std::vector<uint32_t> t(chunk);
  for (uint32_t i = 0; i < m; i++) {
    if (faults[i]) continue;
    const uint32_t g = group_of ? group_of[i] : 0;
    if (g >= groups) return -1;
    uint32_t highest = 0;
    for (uint32_t j = 0; j < n; j++) highest = max_round[(size_t)i * n + j] > highest ? max_round[(size_t)i * n + j] : highest;
    const uint32_t rows = rtl_rows(highest, rcap);
    const uint32_t* table = first_time + (size_t)i * n * rcap;
    for (uint32_t j = 0; j < n; j++) {
      uint32_t carry_r = LBFT_RTL_NO_ROUND, carry_t = 0;
      for (uint32_t c0 = 0; c0 < rows; c0 += chunk) {
        for (uint32_t l = 0; l < chunk; l++) t[l] = rtl_cell(c0 + l < rcap ? table[(size_t)j * rcap + c0 + l] : LBFT_RTL_EMPTY, c0 + l, rows);
        for (uint32_t l = 0; l < chunk; l++) {
          uint32_t pr = carry_r, pt = carry_t;
          for (uint32_t b = l; b-- > 0;)
            if (!rtl_empty(t[b])) { pr = c0 + b; pt = t[b]; break; }
          uint32_t stay, skipped;
          if (rtl_pair(t[l], c0 + l, pt, pr, stay, skipped)) {
            stay_hist[(size_t)g * bins + gs_bin(stay, width, bins)]++;
            gs_stat_add(st[g * RTL_FAMILIES + RTL_STAY], stay);
            gs_stat_add(st[g * RTL_FAMILIES + RTL_SKIPPED], skipped);
          }
        }
        for (uint32_t l = chunk; l-- > 0;)
          if (!rtl_empty(t[l])) { carry_r = c0 + l; carry_t = t[l]; break; }
      }
    }
    // (round-major over every stored row, also those at and past `rows`: the cut is the header's)
    for (uint32_t r = 0; r < rcap; r++) {
      RtlRound q = rtl_round_empty();
      for (uint32_t j = 0; j < n; j++) rtl_round_add(q, table[(size_t)j * rcap + r]);
      uint32_t v;
      if (rtl_skew(q, r, rows, v)) {
        skew_hist[(size_t)g * bins + gs_bin(v, width, bins)]++;
        gs_stat_add(st[g * RTL_FAMILIES + RTL_SKEW], v);
      }
      if (rtl_reach(q, r, rows, v)) gs_stat_add(st[g * RTL_FAMILIES + RTL_REACH], v);
    }
  }
  for (size_t q = 0; q < st.size(); q++) {
    stats[q * 4 + 0] = st[q].cnt; stats[q * 4 + 1] = st[q].sum;
    stats[q * 4 + 2] = st[q].cnt ? ~st[q].nmin : 0; stats[q * 4 + 3] = st[q].max;
  }
  return 0;
}

// The grid rule of the statistic kernels' launchers (lbft_group_stats.h), as it is.
extern "C" uint64_t gs_workgroups_host(uint64_t target, uint64_t groups, uint64_t steps, uint64_t samples) { return gs_workgroups(target, groups, steps, samples); }
