// TEST INFRASTRUCTURE: host shim over the host part of lbft_load_stats.h, the arithmetic lbft_k_ps_load turns the words of a finished
// instance into its sixteen samples with, and what becomes of the samples per group.  The shim is handed an instance's words in
// LoadWord order and its nodes' commit counts and active rounds, and does what a segment does: lane f takes its word and the nodes
// f, f + 16, ...; the sixteen lanes' parts are merged; lanes 0 to 2 give the message sum.
#include <stddef.h>

#include <vector>

#include "../librabft_simulator_amd/csrc/lbft_load_stats.h"

extern "C" int ld_rows_host(const uint32_t* words /*[m][LDW_WORDS]*/, const uint32_t* commits /*[m][n]*/, const uint32_t* rounds /*[m][n]*/, uint32_t m,
                            uint32_t n, int calendar, uint32_t* rows /*[m][LD_FAMILIES]*/) {
  if (!n || n > 128) return -1;
  for (uint32_t i = 0; i < m; i++) {
    uint32_t v[LD_SEGMENT], messages = 0;
    LdNodes nodes = ld_nodes_empty();
    for (uint32_t f = 0; f < LD_SEGMENT; f++) {
      const uint32_t w = ld_word_of(f);
      v[f] = w != LDW_NONE ? ld_word_sample(f, words[(size_t)i * LDW_WORDS + w], calendar != 0) : 0u;
      LdNodes mine = ld_nodes_empty();
      for (uint32_t q = f; q < n; q += LD_SEGMENT) ld_nodes_add(mine, commits[(size_t)i * n + q], rounds[(size_t)i * n + q]);
      nodes = ld_nodes_merge(nodes, mine);
      messages += ld_message_share(f, v[f]);
    }
    for (uint32_t f = 0; f < LD_FAMILIES; f++) rows[(size_t)i * LD_FAMILIES + f] = ld_sample(f, v[f], messages, nodes);
  }
  return 0;
}

// The grouped outputs from the rows and the fault words, as the kernel accumulates them: the census over every instance, the
// statistics (GsStat, the minimum un-complemented at the end as the library's host code does) and the histogram over the clean ones.
extern "C" int ld_group_host(const uint32_t* rows, const uint32_t* faults, const uint32_t* group_of /*NULL: one group*/, uint32_t m, uint32_t groups,
                             uint32_t hist_family, uint32_t bin_width, uint32_t bins, uint64_t* hist /*[groups][bins]*/,
                             uint64_t* census /*[groups][32]*/, uint64_t* stats /*[groups][LD_WORDS]*/) {
  if (!groups || hist_family >= LD_FAMILIES || !bin_width || !bins) return -1;
  std::vector<GsStat> st((size_t)groups * LD_FAMILIES, GsStat{0, 0, 0, 0});
  for (uint32_t i = 0; i < m; i++) {
    const uint32_t g = group_of ? group_of[i] : 0;
    if (g >= groups) return -1;
    for (uint32_t k = 0; k < LD_FAULT_BITS; k++) census[(size_t)g * LD_FAULT_BITS + k] += ld_fault_bit(faults[i], k) ? 1 : 0;
    if (!ld_clean(faults[i])) continue;
    for (uint32_t f = 0; f < LD_FAMILIES; f++) gs_stat_add(st[(size_t)g * LD_FAMILIES + f], rows[(size_t)i * LD_FAMILIES + f]);
    hist[(size_t)g * bins + gs_bin(rows[(size_t)i * LD_FAMILIES + hist_family], bin_width, bins)]++;
  }
  for (size_t q = 0; q < st.size(); q++) {
    stats[q * 4 + 0] = st[q].cnt; stats[q * 4 + 1] = st[q].sum;
    stats[q * 4 + 2] = st[q].cnt ? ~st[q].nmin : 0; stats[q * 4 + 3] = st[q].max;
  }
  return 0;
}

// The grid rule of the launcher, as lbft_ps_launch_load calls it, and the geometry.
extern "C" uint64_t ld_workgroups_host(uint64_t groups, uint64_t max_group) { return ld_workgroups(groups, max_group); }
extern "C" uint32_t ld_constant_host(uint32_t which) {
  const uint32_t c[] = {LD_FAMILIES, LD_WORDS, LD_SEGMENT, LD_FAULT_BITS, LDW_WORDS, LD_BLOCK, LD_WORKGROUPS, LD_LDS_BINS};
  return which < sizeof(c) / sizeof(c[0]) ? c[which] : 0xffffffffu;
}
extern "C" uint32_t ld_word_of_host(uint32_t family) { return ld_word_of(family); }
