// TEST INFRASTRUCTURE: host shim over lbft_instance_stats.h and the rule headers it includes, the arithmetic lbft_k_ct_instances turns a
// finished run into per-instance statistics with.  It takes the state as the device holds it -- ctimes[instance][node][lcap] (-1 = not
// recorded), logs[instance][node][lcap] of block ids (1-based), commits[instance][node] (not yet clamped), the block pool as blk_author /
// blk_time[instance][blocks + 1] (index = block id), startup[instance][node], the fault words, the rights table (NULL = unit rights) with
// its rotation and commands_per_epoch, since[group] (NULL = 0) -- and walks it the way the kernel does: the reference node by the key
// order, the chain `chunk` entries side by side, row j of a chunk staged into the [n][chunk] tile while its entries give the timeline
// samples (the predecessor is the lower lane's entry, lane 0 reads the row's word before the chunk; the chunk's CtlRow is merged into
// node j's) and the latency samples (after the proposal time of the node's own block), each lane then taking its column, the closing
// pass over the nodes, the merge of the lanes' accumulators.  Plain loops in place of the wavefront; chunk = 1 is a plain walk.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../librabft_simulator_amd/csrc/lbft_instance_stats.h"

extern "C" int ist_host(const int32_t* ctimes, const uint32_t* logs, const uint32_t* commits, const uint32_t* blk_author, const int32_t* blk_time,
                        const int32_t* startup, const uint32_t* faults, const uint32_t* group_of, const uint32_t* rights, uint32_t rot,
                        uint64_t commands_per_epoch, uint32_t total_votes, uint32_t quorum, uint32_t m, uint32_t n, uint32_t lcap, uint32_t blocks,
                        uint32_t groups, const int32_t* since_of, int32_t max_clock, uint32_t chunk, uint64_t* rows) {
  if (!chunk || chunk > 64 || !groups || !n || !commands_per_epoch || rot >= n || max_clock < 0) return -1;
  const uint32_t cpe = fin_cpe32(commands_per_epoch), t_valid = fin_valid_threshold(total_votes, quorum);
  std::vector<int32_t> tile((size_t)n * chunk), gt(chunk), c_of(chunk);
  std::vector<uint32_t> b_of(chunk);
  std::vector<IstStat> st((size_t)chunk * IST_FAMILIES);  // [lane][family]
  std::vector<CtlRow> row(n);                              // (the kernel: lane j's registers)
  for (uint32_t i = 0; i < m; i++) {
    if (faults[i]) continue;  // (the row stays as the caller zeroed it)
    const uint32_t g = group_of ? group_of[i] : 0;
    if (g >= groups) return -1;
    const int32_t since = since_of ? since_of[g] : 0;
    if (since < 0 || since > max_clock) return -1;
    const uint32_t* author = blk_author + (size_t)i * (blocks + 1);
    const int32_t* time = blk_time + (size_t)i * (blocks + 1);
    auto proposal = [&](uint32_t b, int32_t& out) {
      if (b == 0 || b > blocks || author[b] >= n) return false;
      out = startup[(size_t)i * n + author[b]] + time[b];
      return true;
    };
    uint64_t best = 0;
    for (uint32_t j = 0; j < n; j++) best = chn_ref_max(best, chn_ref_key(chn_commits(commits[(size_t)i * n + j], lcap), j));
    const uint32_t L = chn_ref_len(best), ref = chn_ref_node(best);
    for (IstStat& s : st) s = ist_empty();
    for (CtlRow& r : row) r = ctl_empty();
    uint32_t open = 0;
    for (uint32_t c0 = 0; c0 < L; c0 += chunk) {
      const uint32_t have = L - c0 < chunk ? L - c0 : chunk;  // lanes with an entry
      for (uint32_t l = 0; l < have; l++) {
        b_of[l] = logs[((size_t)i * n + ref) * lcap + c0 + l];
        if (!proposal(b_of[l], gt[l])) return -2;
      }
      for (uint32_t j = 0; j < n; j++) {
        const uint32_t ncj = chn_commits(commits[(size_t)i * n + j], lcap);
        const int32_t* ct = ctimes + ((size_t)i * n + j) * lcap;
        for (uint32_t l = 0; l < chunk; l++) {
          const uint32_t k = c0 + l;
          const int32_t c = k < ncj ? ct[k] : FIN_NONE;
          c_of[l] = fin_committer(k, ncj, c) ? c : FIN_NONE;
          tile[(size_t)j * chunk + l] = c_of[l];
        }
        CtlRow piece = ctl_empty();
        for (uint32_t l = 0; l < chunk; l++) {
          const uint32_t k = c0 + l;
          const int32_t prev = l ? c_of[l - 1] : (c0 && k < ncj ? ct[k - 1] : -1);
          CtlRow r = ctl_empty();
          const uint32_t gap = ctl_entry(r, c_of[l], prev, since);
          if (gap) ist_add(st[(size_t)l * IST_FAMILIES + IST_STALLS + CTL_GAPS], gap);
          piece = ctl_merge(piece, r);
          if (c_of[l] >= 0) {
            if (l >= have) return -4;  // (a committer's entry lies below L)
            const uint32_t bj = logs[((size_t)i * n + j) * lcap + k];
            int32_t gj = gt[l];
            if (bj != b_of[l] && !proposal(bj, gj)) return -2;
            if (c_of[l] < gj) return -3;  // a commit before the proposal: a finding, not a sample
            ist_add(st[(size_t)l * IST_FAMILIES + IST_LATENCY], ist_latency(c_of[l], gj));
          }
        }
        row[j] = ctl_merge(row[j], piece);
      }
      for (uint32_t l = 0; l < have; l++) {
        const uint32_t k = c0 + l;
        const FinEntry e = fin_entry(&tile[l], chunk, n, rights, fin_rights_shift(k, cpe, rot, n), t_valid, quorum);
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
#include <stdio.h>

template <class T>
static bool read_into(std::vector<T>& v, size_t count) {
  v.resize(count);
  for (T& x : v) {
    long long t;
    if (scanf("%lld", &t) != 1) return false;
    x = (T)t;
  }
  return true;
}

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
    std::vector<int32_t> ctimes, blk_time, startup, since;
    std::vector<uint32_t> logs, commits, blk_author, faults, group_of, rights;
    const size_t cells = (size_t)m * n * lcap, pool = (size_t)m * (blocks + 1);
    if (!read_into(ctimes, cells) || !read_into(logs, cells) || !read_into(commits, (size_t)m * n) || !read_into(blk_author, pool) ||
        !read_into(blk_time, pool) || !read_into(startup, (size_t)m * n) || !read_into(faults, m) || !read_into(group_of, m) ||
        !read_into(rights, has_rights ? n : 0) || !read_into(since, has_since ? groups : 0))
      return 2;
    std::vector<uint64_t> rows((size_t)m * IST_WORDS, 0);
    const int rc = ist_host(ctimes.data(), logs.data(), commits.data(), blk_author.data(), blk_time.data(), startup.data(), faults.data(), group_of.data(),
                            has_rights ? rights.data() : nullptr, rot, cpe, total, quorum, m, n, lcap, blocks, groups, has_since ? since.data() : nullptr,
                            max_clock, chunk, rows.data());
    printf("%d", rc);
    for (uint64_t v : rows) printf(" %llu", (unsigned long long)v);
    printf("\n");
  }
  return 0;
}
#endif
