// param_sets_host_model.cpp -- TEST INFRASTRUCTURE (tests/test_param_sets_host_model.py compiles it with g++): the kernel logic of
// parameter-set batches (lbft_core.h's K_SMALL_SETS / K_MID_SETS / K_GENERIC_SETS classes on a SimTSets) built for the host, so that
// mixed-set batches can be compared with the oracle instance by instance on a CPU-only machine.  The queue discipline and kernel class are the
// planner's (csrc/lbft_plan.h, through oracle/host_model_common.h); the emulated LDS queue front is a plain array per instance.
#include <thread>
#include <vector>

#include "../oracle/host_model_common.h"

using namespace lbft;

extern "C" {

// Returns the kernel class the batch ran as (K_SMALL or K_MID), < 0 on a bad argument.  Outputs as lbft_hostmodel_run_batch.
int ps_hostmodel_run(const lbft_config* base, const lbft_param_set* sets, uint32_t n_sets, const uint32_t* set_of, const uint64_t* seeds,
                     size_t m, int64_t max_clock, uint32_t threads, uint32_t* commit_counts, uint64_t* active_rounds, uint64_t* last_states,
                     lbft_commit* histories, size_t history_cap, uint32_t* faults, uint32_t state_fill) {
  const u32 n = base->num_nodes;
  if (n_sets == 0) return -1;
  TwinBatch tb;  // (the base's voting rights and their rotation are the batch's, as on the device)
  const int cls = setup_twin_batch(base, sets, n_sets, 16 * n < 64 ? 64 : 16 * n, m, max_clock, tb);
  if (cls < 0) return cls;
  const Params& p = tb.p;
  const std::vector<ParamSetDev>& dev = tb.dev;
  const RunKernel kernel = pick_run_kernel(p, true, false, PlanKnobs());
  // state_fill: the word the state rows and the emulated LDS hold before Simulator::new runs (0 = fresh pages; these classes never use the
  // calendar queue, the one region the device's host code clears before a run)
  std::vector<u32> state(state_words(p), state_fill);
  if (threads == 0) threads = 1;
  auto worker = [&](u32 tid) {
    for (size_t i = tid; i < m; i += threads) {
      init_instance(p, state.data(), (u32)i, seeds[i], &dev[set_of[i]]);
      run_instance<LIB_PARAMSETS>(kernel, p, state.data(), (u32)i, state_fill, &dev[set_of[i]]);
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
      commit_counts[o] = read_history(s, p, q, histories + o * history_cap, history_cap, &last_states[o]);
      active_rounds[o] = s.nfm(q, NF_PM_ROUND);
    }
  }
  return cls;
}

}  // extern "C"
