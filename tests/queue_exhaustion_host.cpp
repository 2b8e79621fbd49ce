// queue_exhaustion_host.cpp -- TEST INFRASTRUCTURE (CPU only; tests/test_queue_exhaustion_host.py): a stand-alone host build of the kernel logic
// (oracle/host_model.cpp) with a FENCE around every instance.  The host model keeps all instances in one vector, so a sanitizer sees an access that
// leaves the vector but not one that leaves the instance: here every ld / st / ldc / stc of lbft_core.h reports its tile-relative byte offset
// (LBFT_HOOK_MEM) and the offset is compared with the rows of the instance that is running -- below total_words rows, and in the instance's own
// column of the tile.  The first violation is recorded, nothing aborts.  The branch counters of the calendar's exhausted-pool paths (LBFT_POOL_STAT)
// are reported per case.  Cases come from stdin as plain numbers, one line each after the count:
//   n delay_model mean variance lo hi commands_per_epoch quirks equivocate_every drop_per_million partition_size partition_start partition_end
//   max_clock qcap scap bcap lcap ql qheap qcal ring ring_topup tw state_fill history_cap m seed[m]
// and, optionally, after the seeds on the same line:  rights_rotation voting_right[n]  (without them: unit rights, no rotation).
// Output, per case: "case <rc> <m> <n>", then per instance one line
//   fault maxq maxsnap cal_free cal_bump cal_chunks violations first_offset first_is_store | counts[n] | rounds[n] | states[n] | per node min(count, cap) x (proposer index time)
// (without the bars), then "stats" and the six counters: exhaustion on an empty bucket, on a full tail chunk, in bulk_append for a leader that
// needed 1 / 2 / 3 new chunks, and in bulk_append with a free stack that is non-empty but too short.
//   g++ -O2 -std=c++17 -ffp-contract=off -pthread tests/queue_exhaustion_host.cpp -o queue_exhaustion_host
#define LBFT_HOST_MEMHOOK 1
#define LBFT_HOST_POOL_STATS 1
#define LBFT_HOST_FENCE 1
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace lbft { unsigned long long lbft_host_pool_stats[6]; }

#include "../oracle/host_model.cpp"

struct Fence {
  unsigned long long violations = 0;
  unsigned first_off = 0;
  int first_store = 0;
};
static std::vector<Fence> g_fence;
static unsigned long long g_tile_bytes = 0;  // total_words rows of 4 * tw bytes
static unsigned g_row_bytes = 4, g_lane4 = 0, g_inst = 0;
static bool g_fenced = false;

void lbft_host_fence_instance(const lbft::Params& p, uint32_t i) {
  g_row_bytes = 4u * p.tw;
  g_tile_bytes = (unsigned long long)p.total_words * g_row_bytes;
  g_lane4 = (i & (p.tw - 1u)) * 4u;
  g_inst = i;
  if (g_fence.size() <= i) g_fence.resize(i + 1);
  g_fenced = true;
}
namespace lbft {
void lbft_host_mem(unsigned off, int store) {
  if (!g_fenced) return;
  if (off < g_tile_bytes && off % g_row_bytes == g_lane4) return;
  Fence& f = g_fence[g_inst];
  if (!f.violations++) { f.first_off = off; f.first_store = store; }
}
}  // namespace lbft

int main() {
  std::string text;
  if (!std::getline(std::cin, text)) return 2;
  const int n_cases = atoi(text.c_str());
  for (int c = 0; c < n_cases; c++) {
    if (!std::getline(std::cin, text)) return 2;
    std::istringstream line(text);
    lbft_oracle_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    lbft_hostmodel_caps caps;
    memset(&caps, 0, sizeof(caps));
    long long max_clock = 0;
    unsigned long long cpe = 0, history_cap = 0, m = 0;
    long long lo, hi, ps, pe;
    line >> cfg.num_nodes >> cfg.delay_model >> cfg.mean >> cfg.variance >> lo >> hi >> cpe >> cfg.quirks >> cfg.equivocate_every >> cfg.drop_per_million >>
        cfg.partition_size >> ps >> pe;
    line >> max_clock >> caps.qcap >> caps.scap >> caps.bcap >> caps.lcap >> caps.ql >> caps.qheap >> caps.qcal >> caps.ring >> caps.ring_topup >> caps.tw >>
        caps.state_fill >> history_cap >> m;
    if (!line) return 2;
    cfg.uniform_lo = lo; cfg.uniform_hi = hi; cfg.partition_start = ps; cfg.partition_end = pe; cfg.commands_per_epoch = cpe;
    cfg.target_commit_interval = 100000; cfg.delta = 20; cfg.gamma = 2.0; cfg.lambda = 0.5; cfg.math_mode = 1;  // (oracle_ctypes.make_config's defaults)
    std::vector<uint64_t> seeds(m);
    for (auto& s : seeds) { unsigned long long v; if (!(line >> v)) return 2; s = v; }
    std::vector<uint64_t> rights;
    unsigned rotation = 0;
    if (line >> rotation) {  // the optional tail: rights_rotation and one voting right per node
      rights.resize(cfg.num_nodes);
      for (auto& w : rights) { unsigned long long v; if (!(line >> v)) return 2; w = v; }
      cfg.voting_rights = rights.data();
      cfg.rights_rotation = rotation;
    }
    if (!line.eof()) { line >> std::ws; if (!line.eof()) return 2; }
    const size_t n = cfg.num_nodes;
    std::vector<uint32_t> counts(m * n), faults(m), maxq(m), maxsnap(m), cal(3 * m);
    std::vector<uint64_t> rounds(m * n), states(m * n);
    std::vector<lbft_oracle_commit> hist(m * n * (history_cap ? history_cap : 1));
    g_fence.assign(m, Fence());
    for (int k = 0; k < 6; k++) lbft::lbft_host_pool_stats[k] = 0;
    lbft_hostmodel_caps_size(sizeof(caps));
    lbft_hostmodel_capture_calendar(cal.data());
    const int rc = lbft_hostmodel_run_batch(&cfg, &caps, seeds.data(), m, max_clock, 1, counts.data(), rounds.data(), states.data(), hist.data(), history_cap,
                                            nullptr, faults.data(), maxq.data(), maxsnap.data(), nullptr, nullptr, nullptr, 0);
    g_fenced = false;
    printf("case %d %llu %zu\n", rc, m, n);
    if (rc < 0) continue;
    for (size_t i = 0; i < m; i++) {
      const Fence& f = g_fence[i];
      printf("%u %u %u %u %u %u %llu %u %d", faults[i], maxq[i], maxsnap[i], cal[3 * i], cal[3 * i + 1], cal[3 * i + 2], f.violations, f.first_off, f.first_store);
      for (size_t k = 0; k < n; k++) printf(" %u", counts[i * n + k]);
      for (size_t k = 0; k < n; k++) printf(" %" PRIu64, rounds[i * n + k]);
      for (size_t k = 0; k < n; k++) printf(" %" PRIu64, states[i * n + k]);
      for (size_t k = 0; k < n; k++) {
        const size_t cnt = counts[i * n + k] < history_cap ? counts[i * n + k] : history_cap;
        for (size_t e = 0; e < cnt; e++) {
          const lbft_oracle_commit& h = hist[(i * n + k) * history_cap + e];
          printf(" %" PRIu64 " %" PRIu64 " %" PRId64, (uint64_t)h.proposer, (uint64_t)h.index, (int64_t)h.time);
        }
      }
      printf("\n");
    }
    printf("stats");
    for (int k = 0; k < 6; k++) printf(" %llu", lbft::lbft_host_pool_stats[k]);
    printf("\n");
    fflush(stdout);
  }
  return 0;
}
