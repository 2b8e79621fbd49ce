// TEST INFRASTRUCTURE: host shim over lbft_commit_finality.h, the arithmetic lbft_k_ct_finality turns the commit times of an instance's
// nodes into finality samples with.  It takes the state as the device holds it -- ctimes[instance][node][lcap] (-1 = not recorded),
// logs[instance][node][lcap] of block ids (1-based), commits[instance][node] (not yet clamped), the block pool as blk_author /
// blk_time[instance][blocks + 1] (index = block id), startup[instance][node], the fault words, the rights table (NULL = unit rights) with
// its rotation and commands_per_epoch -- and walks it the way the kernel does: the reference node by the key order, the chain `chunk`
// entries side by side, the n rows of a chunk staged as an [n][chunk] tile with FIN_NONE where the node is no committer, each lane
// then taking its column (stride = chunk).  Plain loops in place of the wavefront; chunk = 1 is a plain walk.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../librabft_simulator_amd/csrc/lbft_chain_rules.h"
#include "../librabft_simulator_amd/csrc/lbft_commit_finality.h"

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
    const uint32_t* author = blk_author + (size_t)i * (blocks + 1);
    const int32_t* time = blk_time + (size_t)i * (blocks + 1);
    uint64_t best = 0;
    for (uint32_t j = 0; j < n; j++) best = chn_ref_max(best, chn_ref_key(chn_commits(commits[(size_t)i * n + j], lcap), j));
    const uint32_t L = chn_ref_len(best), ref = chn_ref_node(best);
    uint32_t open = 0;
    for (uint32_t c0 = 0; c0 < L; c0 += chunk) {
      const uint32_t have = L - c0 < chunk ? L - c0 : chunk;  // lanes with an entry
      for (uint32_t j = 0; j < n; j++) {
        const uint32_t ncj = chn_commits(commits[(size_t)i * n + j], lcap);
        for (uint32_t l = 0; l < chunk; l++) {
          const uint32_t k = c0 + l;
          const int32_t c = k < ncj ? ctimes[((size_t)i * n + j) * lcap + k] : FIN_NONE;
          tile[(size_t)j * chunk + l] = fin_committer(k, ncj, c) ? c : FIN_NONE;
        }
      }
      for (uint32_t l = 0; l < have; l++) {
        const uint32_t k = c0 + l;
        const uint32_t b = logs[((size_t)i * n + ref) * lcap + k];
        if (b == 0 || b > blocks) return -2;
        const uint32_t a = author[b];
        if (a >= n) return -2;
        const int32_t gt = startup[(size_t)i * n + a] + time[b];
        const FinEntry e = fin_entry(&tile[l], chunk, n, rights, fin_rights_shift(k, cpe, rot, n), t_valid, quorum);
        const int32_t all = fin_all(e, n);
        if (e.committers) {
          if (e.first < gt) return -3;  // a commit before the proposal: a finding, not a sample
          gs_stat_add(s[FIN_FIRST], fin_after(e.first, gt));
          first_committer[(size_t)g * n + e.first_node]++;
        }
        if (e.valid >= 0) gs_stat_add(s[FIN_VALID], fin_after(e.valid, gt));
        if (e.quorum >= 0) {
          gs_stat_add(s[FIN_QUORUM], fin_after(e.quorum, gt));
          finality_hist[(size_t)g * bins + gs_bin(fin_after(e.quorum, gt), width, bins)]++;
        }
        if (all >= 0) {
          gs_stat_add(s[FIN_ALL], fin_after(all, gt));
          gs_stat_add(s[FIN_SPREAD], fin_after(all, e.first));
          spread_hist[(size_t)g * bins + gs_bin(fin_after(all, e.first), width, bins)]++;
        }
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
