// TEST INFRASTRUCTURE: host shim over lbft_instance_stats.h and the rule headers it includes, the arithmetic lbft_k_ct_instances turns a
// finished run into per-instance statistics with.  The state as the device holds it and the walk are tests/chain_walk_host.h's; the
// shim adds the fault words, the rights table (NULL = unit rights) with its rotation and commands_per_epoch, since[group] (NULL = 0),
// and what the kernel does beside the walk: while row j of a chunk is staged its entries give the timeline samples (the predecessor is
// the lower lane's entry, lane 0 reads the row's word before the chunk; the chunk's CtlRow is merged into node j's) and the latency
// samples, each lane then takes its column, the closing pass goes over the nodes, and the lanes' accumulators are merged.
#include "chain_walk_host.h"

#include "../librabft_simulator_amd/csrc/lbft_instance_stats.h"

extern "C" int ist_host(const int32_t* ctimes, const uint32_t* logs, const uint32_t* commits, const uint32_t* blk_author, const int32_t* blk_time,
                        const int32_t* startup, const uint32_t* faults, const uint32_t* group_of, const uint32_t* rights, uint32_t rot,
                        uint64_t commands_per_epoch, uint32_t total_votes, uint32_t quorum, uint32_t m, uint32_t n, uint32_t lcap, uint32_t blocks,
                        uint32_t groups, const int32_t* since_of, int32_t max_clock, uint32_t chunk, uint64_t* rows) {
  if (!chunk || chunk > 64 || !groups || !n || !commands_per_epoch || rot >= n || max_clock < 0) return -1;
  const uint32_t cpe = fin_cpe32(commands_per_epoch), t_valid = fin_valid_threshold(total_votes, quorum);
  std::vector<int32_t> tile((size_t)n * chunk), gt(chunk);
  std::vector<uint32_t> b_of(chunk);
  std::vector<IstStat> st((size_t)chunk * IST_FAMILIES);  // [lane][family]
  std::vector<CtlRow> row(n);                              // (the kernel: lane j's registers)
  for (uint32_t i = 0; i < m; i++) {
    if (faults[i]) continue;  // (the row stays as the caller zeroed it)
    const uint32_t g = group_of ? group_of[i] : 0;
    if (g >= groups) return -1;
    const int32_t since = since_of ? since_of[g] : 0;
    if (since < 0 || since > max_clock) return -1;
    const CwInstance v = cw_instance(ctimes, logs, commits, blk_author, blk_time, startup, i, n, lcap, blocks);
    const CwChain ch = cw_node_pass(v);
    for (IstStat& s : st) s = ist_empty();
    for (CtlRow& r : row) r = ctl_empty();
    uint32_t open = 0;
    for (uint32_t c0 = 0; c0 < ch.L; c0 += chunk) {
      const uint32_t have = cw_have(ch, c0, chunk);
      for (uint32_t l = 0; l < have; l++) {
        b_of[l] = v.logs[(size_t)ch.ref * lcap + c0 + l];
        if (!cw_proposal(v, b_of[l], gt[l])) return -2;
      }
      for (uint32_t j = 0; j < n; j++) {
        if (!cw_stage(v, j, c0, chunk, have, tile.data())) return -4;
        const int32_t* c_of = &tile[(size_t)j * chunk];
        CtlRow piece = ctl_empty();
        for (uint32_t l = 0; l < chunk; l++) {
          const uint32_t k = c0 + l;
          const int32_t prev = l ? c_of[l - 1] : (c0 && k < cw_commits(v, j) ? v.ctimes[(size_t)j * lcap + k - 1] : -1);
          CtlRow r = ctl_empty();
          const uint32_t gap = ctl_entry(r, c_of[l], prev, since);
          if (gap) ist_add(st[(size_t)l * IST_FAMILIES + IST_STALLS + CTL_GAPS], gap);
          piece = ctl_merge(piece, r);
          if (c_of[l] >= 0) {
            int32_t gj;
            if (!cw_own_proposal(v, j, k, b_of[l], gt[l], gj)) return -2;
            if (c_of[l] < gj) return -3;  // a commit before the proposal: a finding, not a sample
            ist_add(st[(size_t)l * IST_FAMILIES + IST_LATENCY], ist_latency(c_of[l], gj));
          }
        }
        row[j] = ctl_merge(row[j], piece);
      }
      for (uint32_t l = 0; l < have; l++) {
        const FinEntry e = fin_entry(&tile[l], chunk, n, rights, fin_rights_shift(c0 + l, cpe, rot, n), t_valid, quorum);
        if (e.committers && e.first < gt[l]) return -3;
        open += ist_column(&st[(size_t)l * IST_FAMILIES], e, n, gt[l]);
      }
    }
    // closing pass: lane j = node j (the shim: lane j % chunk), lane 0 the instance's `open`
    for (uint32_t j = 0; j < n; j++) ist_node(&st[(size_t)(j % chunk) * IST_FAMILIES], row[j], max_clock);
    ist_add(st[IST_FINALITY + FIN_OPEN], open);
    for (uint32_t f = 0; f < IST_FAMILIES; f++) {
      IstStat t = ist_empty();
      for (uint32_t l = 0; l < chunk; l++) t = ist_merge(t, st[(size_t)l * IST_FAMILIES + f]);
      for (uint32_t w = 0; w < 4; w++) rows[(size_t)i * IST_WORDS + f * 4 + w] = ist_word(t, w);
    }
  }
  return 0;
}

// The grid rule of the launcher, as lbft_ct_launch_instances calls it, and the row's geometry.
extern "C" uint64_t ist_workgroups_host(uint64_t groups, uint64_t max_group) { return ist_workgroups(groups, max_group); }
extern "C" uint32_t ist_words_host() { return IST_WORDS; }
extern "C" uint32_t ist_waves_host() { return IST_WAVES; }

#ifdef IST_HOST_MAIN
// A stand-alone caller for a sanitizer build: the cases are read from stdin as plain numbers (tests/test_instance_stats_host.py writes
// them), the rows are printed.  Format: m n lcap blocks groups rot cpe total quorum max_clock chunk has_rights has_since, then the
// arrays in ist_host's order.
int main() {
  unsigned cases = 0;
  if (scanf("%u", &cases) != 1) return 2;
  for (unsigned q = 0; q < cases; q++) {
    unsigned m, n, lcap, blocks, groups, rot, total, quorum, chunk, has_rights, has_since;
    unsigned long long cpe;
    int max_clock;
    if (scanf("%u %u %u %u %u %u %llu %u %u %d %u %u %u", &m, &n, &lcap, &blocks, &groups, &rot, &cpe, &total, &quorum, &max_clock, &chunk, &has_rights,
              &has_since) != 13)
      return 2;
    CwArrays a;
    std::vector<int32_t> since;
    if (!cw_read_arrays(a, m, n, lcap, blocks, has_rights) || !cw_read_into(since, has_since ? groups : 0)) return 2;
    std::vector<uint64_t> rows((size_t)m * IST_WORDS, 0);
    const int rc = ist_host(a.ctimes.data(), a.logs.data(), a.commits.data(), a.blk_author.data(), a.blk_time.data(), a.startup.data(), a.faults.data(),
                            a.group_of.data(), has_rights ? a.rights.data() : nullptr, rot, cpe, total, quorum, m, n, lcap, blocks, groups,
                            has_since ? since.data() : nullptr, max_clock, chunk, rows.data());
    printf("%d", rc);
    for (uint64_t v : rows) printf(" %llu", (unsigned long long)v);
    printf("\n");
  }
  return 0;
}
#endif
