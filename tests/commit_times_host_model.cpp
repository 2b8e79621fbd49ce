// commit_times_host_model.cpp -- TEST INFRASTRUCTURE (tests/test_commit_times_host_model.py compiles it with g++): the kernel logic of batches
// that record commit times (lbft_core.h's K_SMALL_TIMED / K_MID_TIMED / K_SMALL_SETS_TIMED / K_MID_SETS_TIMED classes on a SimTTimed) built
// for the host, so that the recorded times can be compared with the ones derived from the oracle on a CPU-only machine.  The kernel class
// follows prepare_run (sim_class: the twins replace every class-0 / class-1 kernel); the emulated LDS queue front is a plain array per instance.
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "../include/lbft.h"
#include "../librabft_simulator_amd/csrc/lbft_core.h"
#include "../librabft_simulator_amd/csrc/lbft_tables.h"

using namespace lbft;

static const u64 ZX[257] = LBFT_ZIG_NORM_X_BITS_INIT;
static const u64 ZF[257] = LBFT_ZIG_NORM_F_BITS_INIT;
static const u64 ET[256] = LBFT_EXP_TAB_INIT;

static i32 clamp_i32(int64_t v) { return (i32)(v < 0 ? 0 : (v > 0x7fffffff ? 0x7fffffff : v)); }

template <class S>
static void run_one(S& s, const Params& p, u32 fill) {
  // (the emulated LDS starts as the state rows do: on the device it holds an earlier kernel's leftovers)
  std::vector<u64> keys(p.ql ? p.ql : 1, ((u64)fill << 32) | fill);
  std::vector<u32> metas(p.ql ? p.ql : 1, fill);
  std::vector<u32> hcbr(32, fill);
  s.attach_queue(keys.data(), metas.data(), 1, p.ql);
  if (p.ql) s.attach_hcbr(hcbr.data());
  s.load_scalars();
  s.queue_to_lds();
  s.hcbr_to_lds();
  bool done = s.run();
  s.queue_from_lds();
  s.hcbr_from_lds();
  s.store_scalars(done);
}

template <int KCLS>
static void run_timed(const Params& p, u32* state, u32 i, const ParamSetDev* set, i32* ctimes, u32 state_fill) {
  SimTTimed<KCLS> s(p, state, i);
  if constexpr (SimT<KCLS>::PSET) s.load_set(*set);
  s.attach_commit_times(ctimes, i * p.n);
  run_one(s, p, state_fill);
}

extern "C" {

// A batch of `base` (n_sets == 0: a plain batch) or of parameter sets over `base`, run to max_clock with commit times recorded.
// Returns the kernel class (K_SMALL or K_MID), < 0 on a bad argument.  commit_times: [instance][node][history_cap] (-1 padded), histories
// [instance][node][history_cap], startup times [instance][node], faults [instance].
int ct_hostmodel_run(const lbft_config* base, const lbft_param_set* sets, uint32_t n_sets, const uint32_t* set_of, const uint64_t* seeds,
                     size_t m, int64_t max_clock, uint32_t threads, uint32_t* commit_counts, int64_t* commit_times, lbft_commit* histories,
                     int64_t* startup_times, size_t history_cap, uint32_t* faults, uint32_t state_fill) {
  const u32 n = base->num_nodes;
  if (n == 0 || n > 32 || n_sets > LBFT_MAX_PARAM_SETS) return -1;
  Params p;
  memset(&p, 0, sizeof(p));
  p.n = n;
  p.m = (u32)m;
  p.stride = (u32)((m + 63) / 64 * 64);
  // capacities: generous event queue / snapshot pools; the queue discipline follows prepare_run's rule -- an LDS-fronted array up to 256
  // slots, a heap above
  p.qcap = n <= 4 ? 256 : (16 * n * n > 4096 ? 16 * n * n : 4096);
  const bool q1 = (base->quirks & 1u) != 0;
  p.scap = q1 ? (n * n + 8 * n > 64 * n ? n * n + 8 * n : 64 * n) : (16 * n < 64 ? 64 : 16 * n);
  u64 bauto = n <= 2 ? (u64)max_clock + 64 : (u64)max_clock / 10 + 64;
  p.bcap = (u32)(bauto > 65534 ? 65534 : bauto);
  p.lcap = p.bcap;
  p.qheap = p.qcap > 256 ? 1u : 0u;
  p.max_clock = (i32)max_clock;
  p.delay_model = base->delay_model;
  p.cpe = base->commands_per_epoch;
  p.equiv = base->equivocate_every;
  p.quirks = base->quirks;
  {  // as prepare_run: the archive of retired record stores (quirks bit 0) holds every epoch a node can reach
    u64 eauto = (u64)p.bcap / (p.cpe ? p.cpe : 1) + 2;
    p.ecap = q1 ? (u32)(eauto > 4096 ? 4096 : eauto) : 0;
  }
  std::vector<u32> weights(n, 1);
  p.total_votes = 0;
  p.unit_weights = 1;
  for (u32 i = 0; i < n; i++) {
    weights[i] = base->voting_rights ? (u32)base->voting_rights[i] : 1;
    p.total_votes += weights[i];
    if (weights[i] != 1) p.unit_weights = 0;
  }
  p.weights = weights.data();
  p.rot = 0;
  p.mw = (n + 31) / 32;
  p.quorum = 2 * p.total_votes / 3 + 1;
  // the configurations: the base's (a plain batch) or one per set, as fill_params derives them, each with its duration table
  const u32 n_cfg = n_sets ? n_sets : 1;
  std::vector<ParamSetDev> dev(n_cfg);
  std::vector<std::vector<i64>> dur(n_cfg, std::vector<i64>(4096));
  for (u32 k = 0; k < n_cfg; k++) {
    lbft_param_set s;
    if (n_sets) s = sets[k];
    else {
      s.mean = base->mean; s.variance = base->variance; s.uniform_lo = base->uniform_lo; s.uniform_hi = base->uniform_hi;
      s.target_commit_interval = base->target_commit_interval; s.delta = base->delta; s.gamma = base->gamma; s.lambda = base->lambda;
      s.drop_per_million = base->drop_per_million; s.partition_size = base->partition_size;
      s.partition_start = base->partition_start; s.partition_end = base->partition_end;
    }
    ParamSetDev& d = dev[k];
    d.mu = std::log(s.mean / std::sqrt(1.0 + s.variance / (s.mean * s.mean)));
    d.sigma = std::sqrt(std::log(1.0 + s.variance / (s.mean * s.mean)));
    d.uni_lo = s.uniform_lo;
    d.uni_span = (u64)(s.uniform_hi - s.uniform_lo) + 1;
    d.tci = s.target_commit_interval;
    d.lambda = s.lambda;
    d.drop_ppm = s.drop_per_million;
    d.part_size = s.partition_size;
    d.part_start = clamp_i32(s.partition_start);
    d.part_end = clamp_i32(s.partition_end);
    for (size_t j = 0; j < dur[k].size(); j++) dur[k][j] = f64_to_i64_sat((double)s.delta * std::pow((double)j, s.gamma));
    d.dur_tab = dur[k].data();
    p.drop_ppm |= s.drop_per_million;
    if (s.partition_size > p.part_size) p.part_size = s.partition_size;
  }
  // a plain batch reads everything from Params; a parameter-set batch's step reads the varying fields from the lane's set
  p.mu = dev[0].mu; p.sigma = dev[0].sigma; p.uni_lo = dev[0].uni_lo; p.uni_span = dev[0].uni_span; p.tci = dev[0].tci; p.lambda = dev[0].lambda;
  p.part_start = dev[0].part_start; p.part_end = dev[0].part_end;
  if (!n_sets) { p.drop_ppm = dev[0].drop_ppm; p.part_size = dev[0].part_size; }
  const u32 leader_len = 4096;
  std::vector<u8> leaders(leader_len);
  for (u32 r = 0; r < leader_len; r++) leaders[r] = (u8)compute_leader(p.weights, p.n, p.total_votes, r, 0);
  p.dur_tab = dur[0].data(); p.dur_len = 4096;
  p.leader_tab = leaders.data(); p.leader_len = leader_len;
  p.exp_tab = ET; p.zig_x = ZX; p.zig_f = ZF;
  const int cls = sim_class(p);
  p.ql = cls == K_SMALL ? 32 : 16;  // an emulated LDS front (the packed class-0 queue is scanned in batches of 16)
  p.tw = layout_tile_width(p);
  p.rsh = 2;
  while ((1u << p.rsh) < 4u * p.tw) p.rsh++;
  compute_layout(p);
  // state_fill: the word the state rows and the emulated LDS hold before Simulator::new runs (0 = fresh pages; these classes never use the
  // calendar queue, the one region the device's host code clears before a run)
  std::vector<u32> state(state_words(p), state_fill);
  std::vector<i32> ct((size_t)m * n * p.lcap, -1);
  if (threads == 0) threads = 1;
  auto worker = [&](u32 tid) {
    for (size_t i = tid; i < m; i += threads) {
      const ParamSetDev* d = &dev[n_sets ? set_of[i] : 0];
      if (n_sets) { SimTSets<K_GENERIC_SETS> s0(p, state.data(), (u32)i); s0.load_set(*d); s0.init(seeds[i]); }
      else { Sim s0(p, state.data(), (u32)i); s0.init(seeds[i]); }
      if (n_sets && cls == K_SMALL) run_timed<K_SMALL_SETS_TIMED>(p, state.data(), (u32)i, d, ct.data(), state_fill);
      else if (n_sets) run_timed<K_MID_SETS_TIMED>(p, state.data(), (u32)i, d, ct.data(), state_fill);
      else if (cls == K_SMALL) run_timed<K_SMALL_TIMED>(p, state.data(), (u32)i, nullptr, ct.data(), state_fill);
      else run_timed<K_MID_TIMED>(p, state.data(), (u32)i, nullptr, ct.data(), state_fill);
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
      u32 nc = s.nfm(q, NF_NCOMMITS);
      commit_counts[o] = nc;
      startup_times[o] = (i64)(i32)s.nfm(q, NF_STARTUP);
      for (size_t k = 0; k < history_cap; k++) {
        commit_times[o * history_cap + k] = k < p.lcap ? ct[o * p.lcap + k] : -1;
        if (k < nc) {
          u32 b = s.ld(p.off_log + q * p.lcap + k);
          histories[o * history_cap + k] = lbft_commit{s.blk_author(b), s.bf(b, B_CMD), (i64)(i32)s.bf(b, B_TIME)};
        }
      }
    }
  }
  return cls;
}

}  // extern "C"
