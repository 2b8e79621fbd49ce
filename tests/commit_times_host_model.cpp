// commit_times_host_model.cpp -- TEST INFRASTRUCTURE (tests/test_commit_times_host_model.py compiles it with g++): the kernel logic of batches
// that record commit times (lbft_core.h's K_SMALL_TIMED / K_MID_TIMED / K_SMALL_SETS_TIMED / K_MID_SETS_TIMED classes on a SimTTimed) built
// for the host, so that the recorded times can be compared with the ones derived from the oracle on a CPU-only machine.  The kernel class
// is the planner's (csrc/lbft_plan.h, through oracle/host_model_common.h: the twins replace every class-0 / class-1 kernel); the emulated LDS queue front is a plain array per instance.
#include <thread>
#include <vector>

#include "../oracle/host_model_common.h"

using namespace lbft;

extern "C" {

// A batch of `base` (n_sets == 0: a plain batch) or of parameter sets over `base`, run to max_clock with commit times recorded.
// Returns the kernel class (K_SMALL or K_MID), < 0 on a bad argument.  commit_times: [instance][node][history_cap] (-1 padded), histories
// [instance][node][history_cap], startup times [instance][node], faults [instance].
int ct_hostmodel_run(const lbft_config* base, const lbft_param_set* sets, uint32_t n_sets, const uint32_t* set_of, const uint64_t* seeds,
                     size_t m, int64_t max_clock, uint32_t threads, uint32_t* commit_counts, int64_t* commit_times, lbft_commit* histories,
                     int64_t* startup_times, size_t history_cap, uint32_t* faults, uint32_t state_fill) {
  const u32 n = base->num_nodes;
  lbft_config fixed = *base;  // (this model keeps one assignment of the voting rights)
  fixed.rights_rotation = 0;
  TwinBatch tb;  // (quirks bit 0: every request and response in flight holds a snapshot slot as well -- the planner's pool)
  const int cls = setup_twin_batch(&fixed, sets, n_sets, (base->quirks & 1u) ? 0 : (16 * n < 64 ? 64 : 16 * n), m, max_clock, tb);
  if (cls < 0) return cls;
  const Params& p = tb.p;
  const std::vector<ParamSetDev>& dev = tb.dev;
  const RunKernel kernel = pick_run_kernel(p, n_sets != 0, true, PlanKnobs());
  // state_fill: the word the state rows and the emulated LDS hold before Simulator::new runs (0 = fresh pages; these classes never use the
  // calendar queue, the one region the device's host code clears before a run)
  std::vector<u32> state(state_words(p), state_fill);
  std::vector<i32> ct((size_t)m * n * p.lcap, -1);
  if (threads == 0) threads = 1;
  auto worker = [&](u32 tid) {
    for (size_t i = tid; i < m; i += threads) {
      const ParamSetDev* d = n_sets ? &dev[set_of[i]] : nullptr;
      init_instance(p, state.data(), (u32)i, seeds[i], d);
      run_instance<LIB_COMMIT_TIMES>(kernel, p, state.data(), (u32)i, state_fill, d, ct.data());
    }
  };
  std::vector<std::thread> ts;
  for (u32 t = 1; t < threads; t++) ts.emplace_back(worker, t);
  worker(0);
  for (auto& t : ts) t.join();
  for (size_t i = 0; i < m; i++) {
    Sim s(p, state.data(), (u32)i);
    s.load_scalars();
    faults[i] = s.fault;
    for (u32 q = 0; q < n; q++) {
      size_t o = i * n + q;
      commit_counts[o] = read_history(s, p, q, histories + o * history_cap, history_cap, (u64*)nullptr);
      startup_times[o] = (i64)(i32)s.nfm(q, NF_STARTUP);
      for (size_t k = 0; k < history_cap; k++) commit_times[o * history_cap + k] = k < p.lcap ? ct[o * p.lcap + k] : -1;
    }
  }
  return cls;
}

}  // extern "C"
