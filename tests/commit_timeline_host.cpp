// TEST INFRASTRUCTURE: host shim over lbft_commit_timeline.h, the arithmetic lbft_k_ct_timeline turns a row of commit times into samples
// with.  It walks every row the way the kernel does -- `seg` lanes side by side, entry k in lane k % seg, each lane seeing its
// predecessor's entry (lane 0 the last entry of the previous chunk), the lanes' partial rows merged at the end -- with plain loops in
// place of the wavefront, and accumulates series / gap histogram / statistics as the C ABI returns them.  seg = 1 is a plain walk.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../librabft_simulator_amd/csrc/lbft_commit_timeline.h"

extern "C" int ctl_host(const int64_t* ct, const uint32_t* counts, const uint32_t* faults, const uint32_t* group_of, uint32_t m, uint32_t n,
                        uint32_t cap, uint32_t groups, const int64_t* since, int64_t max_clock, uint32_t width, uint32_t bins, uint32_t seg,
                        uint64_t* series, uint64_t* hist, uint64_t* stats) {
  if (!width || !bins || !seg || !groups) return -1;
  std::vector<GsStat> st((size_t)groups * CTL_FAMILIES, GsStat{0, 0, 0, 0});
  std::vector<CtlRow> lane(seg);
  std::vector<int32_t> c(seg);
  for (uint32_t i = 0; i < m; i++) {
    if (faults[i]) continue;
    const uint32_t g = group_of ? group_of[i] : 0;
    if (g >= groups) return -1;
    const int32_t s = since ? (int32_t)since[g] : 0;
    for (uint32_t j = 0; j < n; j++) {
      const int64_t* row = ct + ((size_t)i * n + j) * cap;
      const uint32_t nc = counts[i * n + j] < cap ? counts[i * n + j] : cap;
      for (uint32_t l = 0; l < seg; l++) lane[l] = ctl_empty();
      int32_t carry = -1;
      for (uint32_t c0 = 0; c0 < nc; c0 += seg) {
        for (uint32_t l = 0; l < seg; l++) c[l] = c0 + l < nc ? (int32_t)row[c0 + l] : -1;
        for (uint32_t l = 0; l < seg; l++) {
          if (c[l] >= 0) series[(size_t)g * bins + gs_bin((uint32_t)c[l], width, bins)]++;
          const uint32_t gap = ctl_entry(lane[l], c[l], l ? c[l - 1] : carry, s);
          if (gap) {
            hist[(size_t)g * bins + gs_bin(gap, width, bins)]++;
            gs_stat_add(st[g * CTL_FAMILIES + CTL_GAPS], gap);
          }
        }
        carry = c[seg - 1];
      }
      CtlRow r = lane[seg - 1];  // (merged in another order than the walk: the order must not matter)
      for (uint32_t l = 0; l + 1 < seg; l++) r = ctl_merge(lane[l], r);
      if (r.first != LBFT_CTL_NONE) gs_stat_add(st[g * CTL_FAMILIES + CTL_FIRST], r.first);
      gs_stat_add(st[g * CTL_FAMILIES + CTL_TAIL], ctl_tail(r, (int32_t)max_clock));
      gs_stat_add(st[g * CTL_FAMILIES + CTL_LONGEST], ctl_longest(r, (int32_t)max_clock));
    }
  }
  for (size_t q = 0; q < st.size(); q++) {
    stats[q * 4 + 0] = st[q].cnt; stats[q * 4 + 1] = st[q].sum;
    stats[q * 4 + 2] = st[q].cnt ? ~st[q].nmin : 0; stats[q * 4 + 3] = st[q].max;
  }
  return 0;
}
