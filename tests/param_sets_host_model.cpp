// param_sets_host_model.cpp -- TEST INFRASTRUCTURE (tests/test_param_sets_host_model.py compiles it with g++): the kernel logic of
// parameter-set batches (lbft_core.h's K_SMALL_SETS / K_MID_SETS / K_GENERIC_SETS classes on a SimTSets) built for the host, so that
// mixed-set batches can be compared with the oracle instance by instance on a CPU-only machine.  The queue discipline and kernel class follow
// lbft_hip.hip's prepare_run; the emulated LDS queue front is a plain array per instance.
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

extern "C" {

// Returns the kernel class the batch ran as (K_SMALL or K_MID), < 0 on a bad argument.  Outputs as lbft_hostmodel_run_batch.
int ps_hostmodel_run(const lbft_config* base, const lbft_param_set* sets, uint32_t n_sets, const uint32_t* set_of, const uint64_t* seeds,
                     size_t m, int64_t max_clock, uint32_t threads, uint32_t* commit_counts, uint64_t* active_rounds, uint64_t* last_states,
                     lbft_commit* histories, size_t history_cap, uint32_t* faults, uint32_t state_fill) {
  const u32 n = base->num_nodes;
  if (n == 0 || n > 32 || n_sets == 0 || n_sets > LBFT_MAX_PARAM_SETS) return -1;
  Params p;
  memset(&p, 0, sizeof(p));
  p.n = n;
  p.m = (u32)m;
  p.stride = (u32)((m + 63) / 64 * 64);
  // capacities: generous event queue / snapshot pools (the drawn timeouts can be far below the delays); the queue discipline follows
  // prepare_run's rule -- an LDS-fronted array up to 256 slots (the small class for <= 4 nodes), a heap above
  p.qcap = n <= 4 ? 256 : (16 * n * n > 4096 ? 16 * n * n : 4096);
  p.scap = 16 * n < 64 ? 64 : 16 * n;
  u64 bauto = n <= 2 ? (u64)max_clock + 64 : (u64)max_clock / 10 + 64;
  p.bcap = (u32)(bauto > 65534 ? 65534 : bauto);
  p.lcap = p.bcap;
  p.qheap = p.qcap > 256 ? 1u : 0u;
  p.max_clock = (i32)max_clock;
  p.delay_model = base->delay_model;
  p.cpe = base->commands_per_epoch;
  p.equiv = base->equivocate_every;
  p.quirks = base->quirks;
  p.rot = 0;
  p.ecap = 0;  // (no archive of retired record stores: quirks bit 0 and keep_retired_stores are not drawn)
  std::vector<u32> weights(n, 1);
  p.weights = weights.data();
  p.total_votes = n;
  p.unit_weights = 1;
  p.mw = (n + 31) / 32;
  p.quorum = 2 * p.total_votes / 3 + 1;
  // the sets: what fill_params derives, and one duration table each (host libm pow, as the device library's host code)
  std::vector<ParamSetDev> dev(n_sets);
  std::vector<std::vector<i64>> dur(n_sets, std::vector<i64>(4096));
  for (u32 k = 0; k < n_sets; k++) {
    const lbft_param_set& s = sets[k];
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
  // (the batch-wide fields the step no longer reads in these classes are left at set 0's, as the device library does)
  p.mu = dev[0].mu; p.sigma = dev[0].sigma; p.uni_lo = dev[0].uni_lo; p.uni_span = dev[0].uni_span; p.tci = dev[0].tci; p.lambda = dev[0].lambda;
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
  if (threads == 0) threads = 1;
  auto worker = [&](u32 tid) {
    for (size_t i = tid; i < m; i += threads) {
      const ParamSetDev& d = dev[set_of[i]];
      { SimTSets<K_GENERIC_SETS> s0(p, state.data(), (u32)i); s0.load_set(d); s0.init(seeds[i]); }
      if (cls == K_SMALL) { SimTSets<K_SMALL_SETS> s(p, state.data(), (u32)i); s.load_set(d); run_one(s, p, state_fill); }
      else { SimTSets<K_MID_SETS> s(p, state.data(), (u32)i); s.load_set(d); run_one(s, p, state_fill); }
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
      active_rounds[o] = s.nfm(q, NF_PM_ROUND);
      Sip13 h;
      h.init();
      h.word(nc);
      for (u32 k = 0; k < nc; k++) {
        u32 b = s.ld(p.off_log + q * p.lcap + k);
        u64 proposer = s.blk_author(b), index = s.bf(b, B_CMD);
        i64 time = (i64)(i32)s.bf(b, B_TIME);
        h.word(proposer); h.word(index); h.word((u64)time);
        if (k < history_cap) histories[o * history_cap + k] = lbft_commit{proposer, index, time};
      }
      last_states[o] = h.finish();
    }
  }
  return cls;
}

}  // extern "C"
