// TEST INFRASTRUCTURE: host shim over lbft_chain_rules.h, the arithmetic lbft_k_cs_chain turns an instance's commit logs into samples
// with.  The state as the device holds it (without commit times) and the first half of the walk -- the reference node, the chunks, the
// proposal time -- are tests/chain_walk_host.h's; the shim adds the fault words and what the kernel does with a chunk: each lane takes
// its predecessor from the lane below or from what the previous chunk carried, the run starts are a ballot over the chunk, and inside
// every chunk the other nodes' rows are compared against the chunk's block ids.  chunk <= 64: the ballot is one 64-bit word.
#include "chain_walk_host.h"

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
    const CwInstance v = cw_instance(nullptr, logs, commits, blk_author, blk_time, startup, i, n, lcap, blocks);
    const uint32_t* log = v.logs;
    const CwChain ch = cw_node_pass(v);
    const uint32_t L = ch.L, ref = ch.ref;
    for (uint32_t j = 0; j < n; j++) gs_stat_add(s[CHN_LAG], L - cw_commits(v, j));
    int32_t carry_g = 0;
    uint32_t carry_a = 0, carry_start = 0, differing = 0, inversions = 0;
    for (uint32_t c0 = 0; c0 < L; c0 += chunk) {
      const uint32_t have = cw_have(ch, c0, chunk);
      for (uint32_t l = 0; l < have; l++) {
        b[l] = log[(size_t)ref * lcap + c0 + l];
        if (!cw_proposal(v, b[l], gt[l])) return -2;
        a[l] = v.author[b[l]];
      }
      uint64_t starts = 0;
      for (uint32_t l = 0; l < have; l++) {
        const uint32_t k = c0 + l;
        const int32_t pg = l ? gt[l - 1] : carry_g;
        const uint32_t pa = l ? a[l - 1] : carry_a;
        if (k > 0) {
          const uint32_t d = chn_interval(pg, gt[l]);
          interval_hist[(size_t)g * bins + gs_bin(d, width, bins)]++;
          gs_stat_add(s[CHN_INTERVAL], d);
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
        const uint32_t ncj = cw_commits(v, j);
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
