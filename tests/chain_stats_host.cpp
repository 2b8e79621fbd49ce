// TEST INFRASTRUCTURE: host shim over lbft_chain_rules.h, the arithmetic lbft_k_cs_chain turns an instance's commit logs into samples
// with.  It takes the state as the device holds it -- logs[instance][node][lcap] of block ids (1-based), commits[instance][node] (not
// yet clamped), the block pool as blk_author / blk_time[instance][blocks + 1] (index = block id), startup[instance][node] and the fault
// words -- and walks it the way the kernel does: the reference node by the key order, the chain `chunk` entries side by side, each
// lane taking its predecessor from the lane below or from what the previous chunk carried, the run starts as a ballot over the chunk,
// and inside every chunk the other nodes' rows against the chunk's block ids.  Plain loops in place of the wavefront; chunk = 1 is a
// plain walk.  chunk <= 64: the ballot is one 64-bit word.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../librabft_simulator_amd/csrc/lbft_chain_rules.h"

extern "C" int chn_host(const uint32_t* logs, const uint32_t* commits, const uint32_t* blk_author, const int32_t* blk_time, const int32_t* startup,
                        const uint32_t* faults, const uint32_t* group_of, uint32_t m, uint32_t n, uint32_t lcap, uint32_t blocks, uint32_t groups,
                        uint32_t width, uint32_t bins, uint32_t chunk, uint64_t* interval_hist, uint64_t* author_blocks, uint64_t* stats) {
  if (!width || !bins || !chunk || chunk > 64 || !groups || !n) return -1;
  std::vector<GsStat> st((size_t)groups * CHN_FAMILIES, GsStat{0, 0, 0, 0});
  std::vector<uint32_t> b(chunk), a(chunk);
  std::vector<int32_t> gt(chunk);
  for (uint32_t i = 0; i < m; i++) {
    if (faults[i]) continue;
    const uint32_t g = group_of ? group_of[i] : 0;
    if (g >= groups) return -1;
    GsStat* s = &st[(size_t)g * CHN_FAMILIES];
    const uint32_t* log = logs + (size_t)i * n * lcap;
    const uint32_t* author = blk_author + (size_t)i * (blocks + 1);
    const int32_t* time = blk_time + (size_t)i * (blocks + 1);
    uint64_t best = 0;
    for (uint32_t j = 0; j < n; j++) best = chn_ref_max(best, chn_ref_key(chn_commits(commits[(size_t)i * n + j], lcap), j));
    const uint32_t L = chn_ref_len(best), ref = chn_ref_node(best);
    for (uint32_t j = 0; j < n; j++) gs_stat_add(s[CHN_LAG], L - chn_commits(commits[(size_t)i * n + j], lcap));
    int32_t carry_g = 0;
    uint32_t carry_a = 0, carry_start = 0, differing = 0, inversions = 0;
    for (uint32_t c0 = 0; c0 < L; c0 += chunk) {
      const uint32_t have = L - c0 < chunk ? L - c0 : chunk;  // lanes with an entry
      for (uint32_t l = 0; l < have; l++) {
        b[l] = log[(size_t)ref * lcap + c0 + l];
        if (b[l] == 0 || b[l] > blocks) return -2;
        a[l] = author[b[l]];
        if (a[l] >= n) return -2;
        gt[l] = startup[(size_t)i * n + a[l]] + time[b[l]];
      }
      uint64_t starts = 0;
      for (uint32_t l = 0; l < have; l++) {
        const uint32_t k = c0 + l;
        const int32_t pg = l ? gt[l - 1] : carry_g;
        const uint32_t pa = l ? a[l - 1] : carry_a;
        if (k > 0) {
          const uint32_t v = chn_interval(pg, gt[l]);
          interval_hist[(size_t)g * bins + gs_bin(v, width, bins)]++;
          gs_stat_add(s[CHN_INTERVAL], v);
          inversions += chn_inverted(pg, gt[l]) ? 1u : 0u;
        }
        if (chn_run_start(k, a[l], pa)) starts |= 1ull << l;
      }
      for (uint32_t l = 0; l < have; l++) {
        if (((starts >> l) & 1) && c0 + l > 0) gs_stat_add(s[CHN_TENURE], chn_tenure(c0 + l, starts & ((1ull << l) - 1ull), c0, carry_start));
        author_blocks[(size_t)g * n + a[l]]++;
      }
      carry_start = chn_carry_start(starts, c0, carry_start);
      carry_g = gt[have - 1];
      carry_a = a[have - 1];
      for (uint32_t j = 0; j < n; j++) {
        if (j == ref) continue;
        const uint32_t ncj = chn_commits(commits[(size_t)i * n + j], lcap);
        for (uint32_t l = 0; l < have; l++)
          differing += (c0 + l < ncj && log[(size_t)j * lcap + c0 + l] != b[l]) ? 1u : 0u;
      }
    }
    gs_stat_add(s[CHN_LENGTH], L);
    gs_stat_add(s[CHN_DIFFERING], differing);
    gs_stat_add(s[CHN_INVERSIONS], inversions);
    if (L) gs_stat_add(s[CHN_TENURE], L - carry_start);
  }
  for (size_t q = 0; q < st.size(); q++) {
    stats[q * 4 + 0] = st[q].cnt; stats[q * 4 + 1] = st[q].sum;
    stats[q * 4 + 2] = st[q].cnt ? ~st[q].nmin : 0; stats[q * 4 + 3] = st[q].max;
  }
  return 0;
}

// The grid rule of the launcher (lbft_group_stats.h), as lbft_cs_launch_chain calls it.
extern "C" uint64_t chn_workgroups_host(uint64_t target, uint64_t groups, uint64_t max_group, uint64_t waves, uint64_t lcap, uint64_t n) {
  return gs_workgroups(target, groups, (max_group + waves - 1) / waves, max_group * (lcap > n ? lcap : n));
}
