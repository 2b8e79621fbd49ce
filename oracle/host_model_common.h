// host_model_common.h -- TEST INFRASTRUCTURE: what the host builds of the kernel logic share (oracle/host_model.cpp,
// tests/param_sets_host_model.cpp, tests/commit_times_host_model.cpp): the sampler tables, the leader tables, one lane's run with its
// emulated LDS, and the read-back of a node's committed history.  The batch's parameters and geometry are lbft_plan.h's.
#ifndef LBFT_HOST_MODEL_COMMON_H
#define LBFT_HOST_MODEL_COMMON_H

#include <type_traits>
#include <vector>

#include "../librabft_simulator_amd/csrc/lbft_plan.h"
#include "../librabft_simulator_amd/csrc/lbft_tables.h"

namespace lbft {

static const u64 ZX[257] = LBFT_ZIG_NORM_X_BITS_INIT;
static const u64 ZF[257] = LBFT_ZIG_NORM_F_BITS_INIT;
static const u64 ET[256] = LBFT_EXP_TAB_INIT;

// The tables `p` points into (p.weights set by the caller): the duration table of (delta, gamma), one leader table per shift of the
// rotating voting rights (4 096 rounds each), the sampler's constants
static const u32 HOST_LEADER_LEN = 4096;
inline void attach_tables(Params& p, int64_t delta, double gamma, std::vector<i64>& dur, std::vector<u8>& leaders) {
  dur.resize(LBFT_DUR_TABLE_LEN);
  fill_duration_table(delta, gamma, dur.data(), dur.size());
  const u32 tables = leader_tables(p);
  leaders.resize((size_t)HOST_LEADER_LEN * tables);
  for (u32 k = 0; k < tables; k++)
    for (u32 r = 0; r < HOST_LEADER_LEN; r++) leaders[(size_t)k * HOST_LEADER_LEN + r] = (u8)compute_leader(p.weights, p.n, p.total_votes, r, k);
  p.dur_tab = dur.data(); p.dur_len = (u32)dur.size();
  p.leader_tab = leaders.data(); p.leader_len = HOST_LEADER_LEN;
  p.exp_tab = ET; p.zig_x = ZX; p.zig_f = ZF;
}
// The tile width each class addresses at compile time (64-wide tiles or instance-major rows)
inline void set_tile_width(Params& p, u32 tw) {
  p.tw = tw;
  p.rsh = 2;
  while ((1u << p.rsh) < 4u * p.tw) p.rsh++;
}

// One instance's event loop as the device's launch structures it: the LDS front of the queue is a cache of the HBM rows.  `fill`: the
// word the emulated LDS holds before the run (it starts as the state rows do: on the device it holds an earlier kernel's leftovers).
// Returns whether the cooperative event loop ran.
template <class S>
static bool run_one(S& s, const Params& p, u32 fill) {
  std::vector<u64> keys(p.ql ? p.ql : 1, ((u64)fill << 32) | fill);
  std::vector<u32> metas(p.ql ? p.ql : 1, fill);
  s.attach_queue(keys.data(), metas.data(), 1, p.ql);
  std::vector<u32> hcbr(32, fill);  // the device's LDS copy of the hcbr buffers (class 0, n <= 4)
  if (p.ql) s.attach_hcbr(hcbr.data());
  std::vector<u32> window(32 * (1 + BC_WORDS), fill);  // the large-network kernels' LDS window of block records (32 entries, as the device's default)
  if (p.n > 32) s.attach_blk_window(window.data(), 32, 0);
  s.load_scalars();
  s.queue_to_lds();
  s.hcbr_to_lds();
  bool done, coop = false;
  if constexpr (S::COOP) { coop = p.ring != 0; done = coop ? s.run_coop(true) : s.run(); }
  else done = s.run();
  s.queue_from_lds();
  s.hcbr_from_lds();
  s.store_scalars(done);
  return coop;
}

// Simulator::new of instance `i`: the generic class, with the instance's parameter set `set` when the batch has sets
inline void init_instance(const Params& p, u32* state, u32 i, u64 seed, const ParamSetDev* set = nullptr) {
  if (set) { SimTSets<K_GENERIC_SETS> s(p, state, i); s.load_set(*set); s.init(seed); }
  else { Sim s(p, state, i); s.init(seed); }
}
// Instance `i`'s event loop as the planned run kernel `k` of library LIB runs it (run_body's lane-private branch): the class of k's row
// of lbft_plan.h's table, with the instance's set and the batch's commit-time buffer where the class reads them.  Returns as run_one.
template <RunLib LIB>
static bool run_instance(RunKernel k, const Params& p, u32* state, u32 i, u32 fill, const ParamSetDev* set = nullptr, i32* ctimes = nullptr) {
  return with_run_class<LIB>(k, [&](auto cls) {
    RunSim<decltype(cls)::value> s(p, state, i);
    if constexpr (s.PSET) s.load_set(*set);
    if constexpr (s.CTIME) s.attach_commit_times(ctimes, i * p.n);
    return run_one(s, p, fill);
  });
}

// The committed history of `node` (up to `cap` entries into `out`, a lbft_commit / lbft_oracle_commit array or NULL) and the Sip13
// State over it, as lbft_k_finalize computes it -> commit count.  `s`: the instance, scalars loaded.
template <class Commit>
static u32 read_history(Sim& s, const Params& p, u32 node, Commit* out, size_t cap, u64* last_state) {
  u32 nc = s.nfm(node, NF_NCOMMITS);
  Sip13 h;
  h.init();
  h.word(nc);
  for (u32 k = 0; k < nc; k++) {
    u32 b = s.ld(p.off_log + node * p.lcap + k);
    u64 proposer = s.blk_author(b), index = s.bf(b, B_CMD);
    i64 time = (i64)(i32)s.bf(b, B_TIME);
    h.word(proposer); h.word(index); h.word((u64)time);
    if (out && k < cap) out[k] = Commit{proposer, index, time};
  }
  if (last_state) *last_state = h.finish();
  return nc;
}

// A parameter-set (or plain: n_sets == 0) batch of at most 32 nodes as the twin host models run it: a generous event queue (the drawn
// timeouts can be far below the delays) and the model's own snapshot pool `scap` (0 = the planner's) as explicit capacities, then the
// class, queue discipline and archive lbft_plan.h chooses for them without the calendar, and an emulated LDS front.
// -> the kernel class, < 0 on a bad argument.
struct TwinBatch {
  Params p;
  std::vector<u32> weights;
  std::vector<i64> dur;
  std::vector<u8> leaders;
  std::vector<ParamSetDev> dev;
  std::vector<i64> set_dur;
};
inline int setup_twin_batch(const lbft_config* base, const lbft_param_set* sets, u32 n_sets, u32 scap, size_t m, int64_t max_clock, TwinBatch& t) {
  const u32 n = base->num_nodes;
  if (n == 0 || n > 32 || n_sets > LBFT_MAX_PARAM_SETS) return -1;
  lbft_config c = n_sets ? config_of_sets(*base, sets, n_sets) : *base;
  c.queue_capacity = n <= 4 ? 256 : (16 * n * n > 4096 ? 16 * n * n : 4096);
  c.snapshot_capacity = scap;
  c.block_capacity = c.log_capacity = 0;
  Params& p = t.p;
  if (fill_params(&c, m, p, t.weights) != LBFT_OK) return -1;
  p.weights = t.weights.data();
  bool relayout;
  std::string err;
  if (plan_layout(c, p, max_clock, 0, false, false, 0, ~0ull, PlanKnobs(), false, relayout, err) != LBFT_OK) return -1;
  t.dev.resize(n_sets);
  t.set_dur.resize((size_t)n_sets * LBFT_DUR_TABLE_LEN);
  for (u32 k = 0; k < n_sets; k++)
    t.dev[k] = param_set_dev(config_of_set(*base, sets[k]), m, &t.set_dur[(size_t)k * LBFT_DUR_TABLE_LEN], &t.set_dur[(size_t)k * LBFT_DUR_TABLE_LEN]);
  attach_tables(p, c.delta, c.gamma, t.dur, t.leaders);
  const int cls = sim_class(p);
  p.ql = cls == K_SMALL ? 32 : 16;  // an emulated LDS front (the packed class-0 queue is scanned in batches of 16)
  set_tile_width(p, layout_tile_width(p));
  return cls;
}

}  // namespace lbft
#endif  // LBFT_HOST_MODEL_COMMON_H
