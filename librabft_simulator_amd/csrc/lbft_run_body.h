// lbft_run_body.h -- the body of every run kernel: Simulator::loop_until for every instance (simulator.rs:380-475).  The kernels of
// liblbft_hip.so (lbft_hip.hip), the parameter-set kernels of liblbft_paramsets.so (lbft_paramsets.hip) and the commit-time kernels of
// liblbft_commit_times.so (lbft_commit_times.hip) are run_body<CLS> under their own launch bounds, with the LDS layout of lbft_launch.h,
// so that the host code of liblbft_hip.so sizes and launches all of them alike.
//   K_PARAM_SETS classes: the lane's set (`sets`, `set_of`) is loaded at entry; there is no LDS copy of the duration table -- each lane
//                         reads its set's table from HBM (L2-resident).  The other classes keep the batch's first LBFT_LDS_DURS entries in LDS.
//   K_COMMIT_TIMES classes: the lane's rows of the commit-time buffer (`ctimes`, [instance][node][lcap] i32) are attached at entry.
// Both flags go with the lane-private classes only (run_lane_private: asserted below, and for every row of lbft_plan.h's table); the plain
// classes ignore the three arguments.
// (Included under `using namespace lbft`, after lbft_launch.h.)
#ifndef LBFT_RUN_BODY_H
#define LBFT_RUN_BODY_H

#include "lbft_core.h"

// Phase timers (-DLBFT_PHASE_TIMERS, LBFT_MARK of lbft_core.h): `wprof` = the wavefront's accumulators in LDS.  No-ops in product builds.
template <class S>
__device__ __forceinline__ u64 phase_begin(S& s, u64* wprof, u32 lane) {
#if defined(LBFT_PHASE_TIMERS)
  if (lane == 0) { for (int k = 0; k < LBFT_NPHASES; k++) wprof[k] = 0; wprof[31] = __builtin_readcyclecounter(); }
  s.wprof = wprof;
  return __builtin_readcyclecounter();
#else
  return 0;
#endif
}
// ... every lane of a wavefront sees the wavefront's clock: the first lane reports
template <class S>
__device__ __forceinline__ void phase_end(const Params& p, S& s, u32 lane, u64 t_begin) {
#if defined(LBFT_PHASE_TIMERS)
  if (p.prof && lane == 0) {
    for (int k = 0; k < 31; k++) atomicAdd(&p.prof[k], (unsigned long long)s.wprof[k]);  // 30 = wavefront loop iterations
    atomicAdd(&p.prof[31], (unsigned long long)(__builtin_readcyclecounter() - t_begin));  // total cycles
  }
#endif
}

// One atomic per wavefront: ballot of the lanes that still have pending events.
__device__ __forceinline__ void report_unfinished(u32* __restrict__ unfinished, bool pending_lane, u32 lane) {
  unsigned long long pending = __ballot(pending_lane);
  if (pending && lane == (u32)(__ffsll((long long)pending) - 1)) atomicAdd(unfinished, (u32)__popcll(pending));
}

template <int CLS>
__device__ __forceinline__ void run_body(const Params& p, u32* __restrict__ state, u32* __restrict__ unfinished,
                                         const ParamSetDev* __restrict__ sets = nullptr, const u8* __restrict__ set_of = nullptr,
                                         i32* __restrict__ ctimes = nullptr) {
  constexpr bool PSET = SimT<CLS>::PSET, CTIME = SimT<CLS>::CTIME;
  static_assert(!(PSET || CTIME) || run_lane_private<CLS>, "parameter sets and commit times: lane-private classes only");
  extern __shared__ u64 lds[];
  const u32 nwaves = blockDim.x >> 6;  // wavefronts per workgroup: 8 for the two-wavefronts-per-SIMD kernels, 4 for the full-register ones
  u64* t_zx = lds;
  u64* t_zf = lds + 257;
  u64* t_et = lds + 514;
  for (u32 t = threadIdx.x; t < 257; t += blockDim.x) { t_zx[t] = p.zig_x[t]; t_zf[t] = p.zig_f[t]; }
  for (u32 t = threadIdx.x; t < 256; t += blockDim.x) t_et[t] = p.exp_tab[t];
  i64* t_dur = reinterpret_cast<i64*>(lds + 770);
  u8* t_leader = reinterpret_cast<u8*>(lds + 770 + LBFT_LDS_DURS);
  u32 n_dur = PSET ? 0u : p.dur_len < LBFT_LDS_DURS ? p.dur_len : LBFT_LDS_DURS;
  u32 n_leader = p.leader_len < LBFT_LDS_LEADERS ? p.leader_len : LBFT_LDS_LEADERS;
  for (u32 t = threadIdx.x; t < n_dur; t += blockDim.x) t_dur[t] = p.dur_tab[t];
  for (u32 t = threadIdx.x; t < n_leader; t += blockDim.x) t_leader[t] = p.leader_tab[t];
  u32* t_weights = reinterpret_cast<u32*>(lds + 770 + LBFT_LDS_DURS + LBFT_LDS_LEADERS / 8);
  for (u32 t = threadIdx.x; t < p.n; t += blockDim.x) t_weights[t] = p.weights[t];
  __syncthreads();
  // the queue, the tables above and the voting rights of a simulation (a lambda of this body, like wprof_of below: every kernel's machine code
  // is what the four spelled-out copies gave; table pointers handed to a helper function were reported to cost every run kernel 8-44 B)
  auto attach_lds = [&](auto& s, u64* keys, u32* metas, u32 stride) {
    s.attach_queue(keys, metas, stride, p.ql);
    s.attach_tables(t_zx, t_zf, t_et);
    s.attach_round_tables(t_leader, n_leader, PSET ? nullptr : t_dur, n_dur);
    s.attach_weights(t_weights);
  };
  u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const u32 qslots = p.ql;  // u64 words per instance in the key area
  const u32 qcols = SimT<CLS>::QS32 ? 32u : p.lpw;  // queue columns per wavefront (lbft_k_run0q: always 32, see SimT::QS32)
  u64* keys = lds + LBFT_TABLE_U64 + (size_t)wave * p.ql * qcols + lane;
  u32* metas = reinterpret_cast<u32*>(lds + LBFT_TABLE_U64 + (size_t)nwaves * qslots * qcols) + (size_t)wave * p.ql * qcols + lane;  // (CLS 0: unused, not allocated)
  // diagnostic builds: per-wavefront phase accumulators behind the queue columns (8-byte aligned: the meta area is a multiple of 8 words)
  const u32 meta_words = SimT<CLS>::C0 ? 0u : nwaves * p.ql * p.lpw;
  auto wprof_of = [&](u32 w) {
    return reinterpret_cast<u64*>(reinterpret_cast<u32*>(lds + LBFT_TABLE_U64 + (size_t)nwaves * qslots * qcols) + (size_t)meta_words + (meta_words & 1u)) +
           w * LBFT_NPHASES;
  };
  // Only the first p.lpw lanes of a wavefront carry an instance (occupancy vs lane-utilisation knob).
  u32 i = (blockIdx.x * nwaves + wave) * p.lpw + lane;
  bool active = lane < p.lpw && i < p.m;
  bool done = true;
  // lpw divides 64, so a wavefront's instances share one tile: its base is wavefront-uniform (SGPRs) and every row access is saddr + 32-bit
  // voffset (tile width tw: 64 for the mid-size classes; class 0 and the large networks are instance-major, tw = 1)
  const u32 tw = SimT<CLS>::TILE64 ? 64u : SimT<CLS>::IMAJOR ? 1u : p.tw;
  u32 tile_idx = __builtin_amdgcn_readfirstlane(((blockIdx.x * nwaves + wave) * p.lpw) / tw);
  char* tile = reinterpret_cast<char*>(state) + (size_t)tile_idx * p.total_words * ((size_t)4 * tw);
  if constexpr (SimT<CLS>::COOP) {
    // Large networks: EVERY lane of the wavefront runs the event loop; the first lpw lanes carry a network each, all 64
    // cooperate on the bulk sends of those networks (SimT::run_coop / coop_bulk).
    // (tw may be narrower than the lanes that carry a network: lane j's instance then sits j / tw tiles behind the wavefront's
    // first tile -- folded into the lane's 32-bit column offset, the tile base stays wavefront-uniform)
    const u32 li = active ? (i - ((blockIdx.x * nwaves + wave) * p.lpw)) : (lane & (p.lpw - 1u));
    SimT<CLS> s(p, tile, (li / tw) * (p.total_words * 4u * tw) + (li & (tw - 1u)) * 4u, 0);
    bool lead = false;
    if (active) lead = s.ld(I_DONE) == 0;
    attach_lds(s, keys, metas, p.lpw);
    {  // [receiver lists: nwaves * lpw * LBFT_MAX_NODES bytes][block-record windows: lane-private columns per wavefront]
      u8* lists = reinterpret_cast<u8*>(lds) + run_lds_bytes_dev(p.ql, p.lpw, 12u, nwaves);
      u32* win = reinterpret_cast<u32*>(lists + (size_t)nwaves * p.lpw * LBFT_MAX_NODES) + (size_t)wave * p.lpw * p.blw * (1u + BC_WORDS);
      u32 wsh = 0;
      while ((1u << wsh) < p.lpw) wsh++;
      s.attach_blk_window(win + (lane & (p.lpw - 1u)), p.blw, wsh);
      if (lane < p.lpw) s.blw_reset();
    }
    if (lead) {
      u8* lists = reinterpret_cast<u8*>(lds) + run_lds_bytes_dev(p.ql, p.lpw, 12u, nwaves);
      s.attach_peer_list(lists + ((size_t)wave * p.lpw + lane) * LBFT_MAX_NODES);
      s.load_scalars();
      s.queue_to_lds();
    }
    const u64 t_begin = phase_begin(s, wprof_of(wave), lane);
    bool drained = s.run_coop(lead);
    if (lead) {
      done = drained;
      s.queue_from_lds();
      s.store_scalars(done);
    }
    phase_end(p, s, lane, t_begin);
  } else if constexpr (SimT<CLS>::WUNI) {
    // ONE network per wavefront as wavefront-uniform code (SimT<K_SMALL_UNIFORM>, lbft_k_run0u; p.lpw == 1): nothing below depends on the lane -- the
    // network's index, rows and LDS columns come from the wavefront's index through readfirstlane -- so all 64 lanes run the event loop
    // with the same values and the compiler keeps the protocol logic on the scalar unit (lbft_core.h, SimT::WUNI); only the pop's scan
    // (coop_find) reads per-lane slots.  Stores / LDS writes: the same address and value in every lane.
    const u32 uwave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 ui = __builtin_amdgcn_readfirstlane(blockIdx.x * nwaves + uwave);  // (p.lpw == 1: the wavefront's network)
    u64* ukeys = lds + LBFT_TABLE_U64 + (size_t)uwave * p.ql;
    SimT<CLS> s(p, tile, 0u, 0);
    bool lead = false;
    if (ui < p.m) lead = s.ld(I_DONE) == 0;
    attach_lds(s, ukeys, nullptr, 1u);
    if (p.n <= 4) {  // the nodes' hcbr buffers
      u32* hcb = reinterpret_cast<u32*>(reinterpret_cast<u8*>(lds) + run_lds_bytes_dev(p.ql, 1u, 8u, nwaves));
      s.attach_hcbr(hcb + (size_t)uwave * LBFT_LDS_HCBR_WORDS);
    }
    s.qlen = 0;
    if (lead) {
      s.load_scalars();
      s.queue_to_lds();
      s.hcbr_to_lds();
    }
    const u64 t_begin = phase_begin(s, wprof_of(uwave), lane);
    bool drained = s.run_popc(lead, ukeys);
    if (lead) {
      done = drained;
      s.queue_from_lds();
      s.hcbr_from_lds();
      s.store_scalars(done);
    }
    phase_end(p, s, lane, t_begin);
    active = lane == 0 && ui < p.m;  // (one report per wavefront below)
  } else if constexpr (SimT<CLS>::POPC) {
    // Class 0 with the wavefront-wide pop (SimT::run_popc): every lane runs the event loop and scans the wavefront's queue columns;
    // the lanes that carry a network execute its events.
    SimT<CLS> s(p, tile, SimT<CLS>::IMAJOR ? lane * (p.total_words * 4u) : (i & (tw - 1u)) * 4u, 0);
    bool lead = false;
    if (active) lead = s.ld(I_DONE) == 0;
    attach_lds(s, keys, metas, p.lpw);
    if (p.n <= 4 && !SimT<CLS>::HCREG) {  // the nodes' hcbr buffers
      u32* hcb = reinterpret_cast<u32*>(reinterpret_cast<u8*>(lds) + run_lds_bytes_dev(p.ql, p.lpw, 8u, nwaves));
      s.attach_hcbr(hcb + (size_t)wave * LBFT_LDS_HCBR_WORDS * p.lpw + lane);
    }
    s.qlen = 0;
    if (lead) {
      s.load_scalars();
      s.queue_to_lds();
      s.hcbr_to_lds();
    }
    const u64 t_begin = phase_begin(s, wprof_of(wave), lane);
    bool drained = s.run_popc(lead, keys - lane);
    if (lead) {
      done = drained;
      s.queue_from_lds();
      s.hcbr_from_lds();
      s.store_scalars(done);
    }
    phase_end(p, s, lane, t_begin);
  } else
  if (active) {
    // Every lane its own event loop: SimT, with the lane's parameter set (SimTSets) or also its commit-time rows (SimTTimed).
    // (instance-major classes: lane j's instance sits j instances behind the wavefront's first one -- folded into the lane's 32-bit column offset)
    RunSim<CLS> s(p, tile, SimT<CLS>::IMAJOR ? lane * (p.total_words * 4u) : (i & (tw - 1u)) * 4u, 0);
    if (s.ld(I_DONE) == 0) {
      if constexpr (PSET) s.load_set(sets[set_of[i]]);
      if constexpr (CTIME) s.attach_commit_times(ctimes, i * p.n);
      attach_lds(s, keys, metas, p.lpw);
      if (p.n > 16) {  // receiver / sender lists of process_node_actions: LDS instead of HBM rows
        u8* lists = reinterpret_cast<u8*>(lds) + run_lds_bytes_dev(p.ql, p.lpw, SimT<CLS>::C0 ? 8u : 12u, nwaves);
        s.attach_peer_list(lists + ((size_t)wave * p.lpw + lane) * LBFT_MAX_NODES);
      }
      if (SimT<CLS>::C0 && p.n <= 4 && !SimT<CLS>::HCREG) {  // the nodes' hcbr buffers (same place as the receiver lists of large networks)
        u32* hcb = reinterpret_cast<u32*>(reinterpret_cast<u8*>(lds) + run_lds_bytes_dev(p.ql, p.lpw, 8u, nwaves));
        s.attach_hcbr(hcb + (size_t)wave * LBFT_LDS_HCBR_WORDS * p.lpw + lane);
      }
      s.load_scalars();
      s.queue_to_lds();
      s.hcbr_to_lds();
      const u64 t_begin = phase_begin(s, wprof_of(wave), lane);
      done = s.run();
      s.queue_from_lds();
      s.hcbr_from_lds();
      s.store_scalars(done);
      phase_end(p, s, lane, t_begin);
    }
  }
  report_unfinished(unfinished, active && !done, lane);
}

#endif  // LBFT_RUN_BODY_H
