// TEST INFRASTRUCTURE: host shim over lbft_commit_finality.h, the arithmetic lbft_k_ct_finality turns the commit times of an instance's
// nodes into finality samples with.  The state as the device holds it and the walk are tests/chain_walk_host.h's; the shim adds the
// fault words, the groups, the rights table (NULL = unit rights) with its rotation and commands_per_epoch, and what the kernel does
// with a column: the families' statistics, the two histograms, the first committers, the count of open entries.
#include "chain_walk_host.h"

extern "C" int fin_host(const int32_t* ctimes, const uint32_t* logs, const uint32_t* commits, const uint32_t* blk_author, const int32_t* blk_time,
                        const int32_t* startup, const uint32_t* faults, const uint32_t* group_of, const uint32_t* rights, uint32_t rot,
                        uint64_t commands_per_epoch, uint32_t total_votes, uint32_t quorum, uint32_t m, uint32_t n, uint32_t lcap, uint32_t blocks,
                        uint32_t groups, uint32_t width, uint32_t bins, uint32_t chunk, uint64_t* finality_hist, uint64_t* spread_hist,
                        uint64_t* first_committer, uint64_t* stats) {
  if (!width || !bins || !chunk || chunk > 64 || !groups || !n || !commands_per_epoch || rot >= n) return -1;
  std::vector<GsStat> st((size_t)groups * FIN_FAMILIES, GsStat{0, 0, 0, 0});
  std::vector<int32_t> tile((size_t)n * chunk);
  const uint32_t cpe = fin_cpe32(commands_per_epoch), t_valid = fin_valid_threshold(total_votes, quorum);
  for (uint32_t i = 0; i < m; i++) {
    if (faults[i]) continue;
    const uint32_t g = group_of ? group_of[i] : 0;
    if (g >= groups) return -1;
    GsStat* s = &st[(size_t)g * FIN_FAMILIES];
    const CwInstance v = cw_instance(ctimes, logs, commits, blk_author, blk_time, startup, i, n, lcap, blocks);
    const CwChain ch = cw_node_pass(v);
    uint32_t open = 0;
    for (uint32_t c0 = 0; c0 < ch.L; c0 += chunk) {
      const uint32_t have = cw_have(ch, c0, chunk);
      for (uint32_t j = 0; j < n; j++) cw_stage(v, j, c0, chunk, have, tile.data());
      for (uint32_t l = 0; l < have; l++) {
        const uint32_t k = c0 + l;
        int32_t gt;
        if (!cw_proposal(v, v.logs[(size_t)ch.ref * lcap + k], gt)) return -2;
        const FinEntry e = fin_entry(&tile[l], chunk, n, rights, fin_rights_shift(k, cpe, rot, n), t_valid, quorum);
        if (e.committers && e.first < gt) return -3;  // a commit before the proposal: a finding, not a sample
        fin_samples(e, n, gt, [&](uint32_t family, uint32_t sample) {
          gs_stat_add(s[family], sample);
          if (family == FIN_QUORUM) finality_hist[(size_t)g * bins + gs_bin(sample, width, bins)]++;
          if (family == FIN_SPREAD) spread_hist[(size_t)g * bins + gs_bin(sample, width, bins)]++;
        });
        if (e.committers) first_committer[(size_t)g * n + e.first_node]++;
        open += fin_open(e) ? 1u : 0u;
      }
    }
    gs_stat_add(s[FIN_OPEN], open);
  }
  for (size_t q = 0; q < st.size(); q++) {
    stats[q * 4 + 0] = st[q].cnt; stats[q * 4 + 1] = st[q].sum;
    stats[q * 4 + 2] = st[q].cnt ? ~st[q].nmin : 0; stats[q * 4 + 3] = st[q].max;
  }
  return 0;
}

// The right of node j at entry k, as the header computes it.
extern "C" uint32_t fin_rights_index_host(uint32_t j, uint32_t k, uint64_t commands_per_epoch, uint32_t rot, uint32_t n) {
  return fin_rights_index(j, fin_rights_shift(k, fin_cpe32(commands_per_epoch), rot, n), n);
}

// The grid rule of the launcher (lbft_group_stats.h), as lbft_ct_launch_finality calls it.
extern "C" uint64_t fin_workgroups_host(uint64_t target, uint64_t groups, uint64_t max_group, uint64_t waves, uint64_t lcap) {
  return gs_workgroups(target, groups, (max_group + waves - 1) / waves, max_group * lcap);
}
