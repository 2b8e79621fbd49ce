// TEST INFRASTRUCTURE: host shim over lbft_commit_phases.h and the rule headers of the two calls it splits (lbft_commit_finality.h,
// lbft_chain_rules.h), the arithmetic lbft_k_ct_phases turns a finished run into per-phase statistics with.  The state as the device
// holds it and the walk are tests/chain_walk_host.h's; the shim adds the fault words, the rights table (NULL = unit rights) with its
// rotation and commands_per_epoch, the edges [group][phases - 1] as the launcher takes them, and what the kernel does with a sample:
// per pass of `lds_bins` bins of the virtual histograms, the latency samples while row j of a chunk is staged (in the phase of the
// block that gives the sample its origin), each lane then its column; every sample is added to the four words of its (phase, family).
// The words are kept as the kernel keeps them (samples, sum, max(~sample), max: GsStat's) and turned into the minimum at the end, as the
// library's caller does.
#include "chain_walk_host.h"

#include "../librabft_simulator_amd/csrc/lbft_commit_phases.h"

// (the kernel: four LDS atomics, add, add, max, max)
static void sample(uint64_t* words, uint32_t phase, uint32_t family, uint32_t v) {
  GsStat s = {words[cph_word(phase, family, 0)], words[cph_word(phase, family, 1)], words[cph_word(phase, family, 2)], words[cph_word(phase, family, 3)]};
  gs_stat_add(s, v);
  words[cph_word(phase, family, 0)] = s.cnt; words[cph_word(phase, family, 1)] = s.sum;
  words[cph_word(phase, family, 2)] = s.nmin; words[cph_word(phase, family, 3)] = s.max;
}

extern "C" int cph_host(const int32_t* ctimes, const uint32_t* logs, const uint32_t* commits, const uint32_t* blk_author, const int32_t* blk_time,
                        const int32_t* startup, const uint32_t* faults, const uint32_t* group_of, const uint32_t* rights, uint32_t rot,
                        uint64_t commands_per_epoch, uint32_t total_votes, uint32_t quorum, uint32_t m, uint32_t n, uint32_t lcap, uint32_t blocks,
                        uint32_t groups, const int32_t* edges, uint32_t phases, uint32_t bin_width, uint32_t bins, uint32_t lds_bins, uint32_t chunk,
                        uint64_t* latency_hist, uint64_t* finality_hist, uint64_t* stats) {
  if (!chunk || chunk > 64 || !groups || !n || !commands_per_epoch || rot >= n || !phases || phases > CPH_MAX_PHASES || !bin_width || !bins || !lds_bins ||
      (uint64_t)phases * bins > 0xffffffffull || (phases > 1 && !edges))
    return -1;
  const uint32_t cpe = fin_cpe32(commands_per_epoch), t_valid = fin_valid_threshold(total_votes, quorum);
  const uint32_t n_edges = phases - 1, vbins = phases * bins, words = phases * CPH_STATS;
  std::vector<int32_t> tile((size_t)n * chunk), gt(chunk);
  std::vector<uint32_t> b_of(chunk), ph(chunk);
  for (uint32_t base = 0; base < vbins; base += lds_bins) {
    const uint32_t span = vbins - base < lds_bins ? vbins - base : lds_bins;
    const bool stat_pass = base == 0;
    for (uint32_t i = 0; i < m; i++) {
      if (faults[i]) continue;
      const uint32_t g = group_of ? group_of[i] : 0;
      if (g >= groups) return -1;
      int32_t s_edges[CPH_MAX_PHASES];  // (the kernel: the group's copy in LDS)
      for (uint32_t q = 0; q < CPH_MAX_PHASES; q++) s_edges[q] = q < n_edges ? edges[(size_t)g * n_edges + q] : CPH_NO_EDGE;
      uint64_t* lat = latency_hist + (size_t)g * vbins;
      uint64_t* fin = finality_hist + (size_t)g * vbins;
      uint64_t* w_of = stats + (size_t)g * words;
      const CwInstance v = cw_instance(ctimes, logs, commits, blk_author, blk_time, startup, i, n, lcap, blocks);
      const CwChain ch = cw_node_pass(v);
      for (uint32_t c0 = 0; c0 < ch.L; c0 += chunk) {
        const uint32_t have = cw_have(ch, c0, chunk);
        for (uint32_t l = 0; l < have; l++) {
          b_of[l] = v.logs[(size_t)ch.ref * lcap + c0 + l];
          if (!cw_proposal(v, b_of[l], gt[l])) return -2;
          ph[l] = cph_phase(s_edges, gt[l]);
          if (ph[l] >= phases) return -5;
        }
        for (uint32_t j = 0; j < n; j++) {
          if (!cw_stage(v, j, c0, chunk, have, tile.data())) return -4;
          for (uint32_t l = 0; l < have; l++) {
            const int32_t c = tile[(size_t)j * chunk + l];
            if (c < 0) continue;
            int32_t gj;
            if (!cw_own_proposal(v, j, c0 + l, b_of[l], gt[l], gj)) return -2;
            uint32_t pj = ph[l];
            if (gj != gt[l]) {  // (another block, another time: it has its own phase)
              pj = cph_phase(s_edges, gj);
              if (pj >= phases) return -5;
            }
            if (c < gj) return -3;  // a commit before the proposal: a finding, not a sample
            const uint32_t d = fin_after(c, gj), vb = cph_bin(pj, d, bin_width, bins);
            if (cph_in_pass(vb, base, span)) lat[vb]++;
            if (stat_pass) sample(w_of, pj, CPH_LATENCY, d);
          }
        }
        for (uint32_t l = 0; l < have; l++) {
          const uint32_t k = c0 + l;
          const FinEntry e = fin_entry(&tile[l], chunk, n, rights, fin_rights_shift(k, cpe, rot, n), t_valid, quorum);
          if (e.committers && e.first < gt[l]) return -3;
          if (e.quorum >= 0) {
            const uint32_t vb = cph_bin(ph[l], fin_after(e.quorum, gt[l]), bin_width, bins);
            if (cph_in_pass(vb, base, span)) fin[vb]++;
          }
          if (stat_pass) fin_samples(e, n, gt[l], [&](uint32_t family, uint32_t s) { sample(w_of, ph[l], CPH_FINALITY + family, s); });
        }
      }
    }
  }
  for (size_t q = 0; q < (size_t)groups * words / 4; q++) stats[q * 4 + 2] = stats[q * 4] ? ~stats[q * 4 + 2] : 0;  // (max(~sample) -> min)
  return 0;
}

// The phase of a time among `n_edges` edges, as the kernel looks it up, and the grid rule of the launcher as lbft_ct_launch_phases calls it.
extern "C" uint32_t cph_phase_host(const int32_t* edges, uint32_t n_edges, int32_t t) {
  int32_t padded[CPH_MAX_PHASES];
  for (uint32_t q = 0; q < CPH_MAX_PHASES; q++) padded[q] = q < n_edges ? edges[q] : CPH_NO_EDGE;
  return cph_phase(padded, t);
}
extern "C" uint64_t cph_workgroups_host(uint64_t target, uint64_t groups, uint64_t max_group, uint64_t waves, uint64_t n, uint64_t lcap) {
  return gs_workgroups(target, groups, (max_group + waves - 1) / waves, max_group * n * lcap);
}
extern "C" uint32_t cph_stats_host() { return CPH_STATS; }

#ifdef CPH_HOST_MAIN
// A stand-alone caller for a sanitizer build: the cases are read from stdin as plain numbers (tests/test_commit_phases_host.py writes
// them), the outputs are printed.  Format: m n lcap blocks groups rot cpe total quorum phases width bins lds_bins chunk has_rights, then
// the arrays in cph_host's order.
int main() {
  unsigned cases = 0;
  if (scanf("%u", &cases) != 1) return 2;
  for (unsigned q = 0; q < cases; q++) {
    unsigned m, n, lcap, blocks, groups, rot, total, quorum, phases, width, bins, lds_bins, chunk, has_rights;
    unsigned long long cpe;
    if (scanf("%u %u %u %u %u %u %llu %u %u %u %u %u %u %u %u", &m, &n, &lcap, &blocks, &groups, &rot, &cpe, &total, &quorum, &phases, &width, &bins, &lds_bins,
              &chunk, &has_rights) != 15)
      return 2;
    if (!phases || !bins || (unsigned long long)groups * phases * bins > (1u << 20)) return 2;
    CwArrays a;
    std::vector<int32_t> edges;
    if (!cw_read_arrays(a, m, n, lcap, blocks, has_rights) || !cw_read_into(edges, (size_t)groups * (phases - 1))) return 2;
    std::vector<uint64_t> lat((size_t)groups * phases * bins, 0), fin(lat.size(), 0), stats((size_t)groups * phases * CPH_STATS, 0);
    const int rc = cph_host(a.ctimes.data(), a.logs.data(), a.commits.data(), a.blk_author.data(), a.blk_time.data(), a.startup.data(), a.faults.data(),
                            a.group_of.data(), has_rights ? a.rights.data() : nullptr, rot, cpe, total, quorum, m, n, lcap, blocks, groups,
                            phases > 1 ? edges.data() : nullptr, phases, width, bins, lds_bins, chunk, lat.data(), fin.data(), stats.data());
    printf("%d", rc);
    for (const std::vector<uint64_t>* v : {&lat, &fin, &stats})
      for (uint64_t x : *v) printf(" %llu", (unsigned long long)x);
    printf("\n");
  }
  return 0;
}
#endif
