// lbft_lane_run.h -- the run body of the lane-private kernels of the side libraries: the parameter-set kernels of liblbft_paramsets.so
// (lbft_paramsets.hip) and the commit-time kernels of liblbft_commit_times.so (lbft_commit_times.hip).  Simulator::loop_until for every
// instance: the lane-private event loop of lbft_k_run0 / lbft_k_run<1> (lbft_hip.hip, run_body's last branch) with the same LDS layout
// (lbft_launch.h), so that the host code of liblbft_hip.so sizes and launches them as those two.
//   K_PARAM_SETS classes: the lane's set is loaded at entry; there is no LDS copy of the duration table -- each lane reads its set's
//                         table from HBM (L2-resident).  The other classes keep the batch's first LBFT_LDS_DURS entries in LDS, as
//                         lbft_k_run0 / lbft_k_run<1> do.
//   K_COMMIT_TIMES classes: the lane's rows of the commit-time buffer (`ctimes`, [instance][node][lcap] i32) are attached at entry.
#ifndef LBFT_LANE_RUN_H
#define LBFT_LANE_RUN_H

#include <type_traits>

#include "lbft_core.h"  // (and lbft_launch.h, which the includer brings in under `using namespace lbft`)

template <int CLS>
__device__ __forceinline__ void ps_run_body(const lbft::Params& p, lbft::u32* __restrict__ state, lbft::u32* __restrict__ unfinished,
                                            const lbft::ParamSetDev* __restrict__ sets, const lbft::u8* __restrict__ set_of,
                                            lbft::i32* __restrict__ ctimes) {
  using namespace lbft;
  static_assert(!SimT<CLS>::COOP && !SimT<CLS>::POPC && !SimT<CLS>::WUNI && !SimT<CLS>::QUAD && (SimT<CLS>::PSET || SimT<CLS>::CTIME),
                "lane-private classes only");
  using S = typename std::conditional<SimT<CLS>::CTIME, SimTTimed<CLS>, SimTSets<CLS>>::type;
  extern __shared__ u64 lds[];
  const u32 nwaves = blockDim.x >> 6;
  u64* t_zx = lds;
  u64* t_zf = lds + 257;
  u64* t_et = lds + 514;
  for (u32 t = threadIdx.x; t < 257; t += blockDim.x) { t_zx[t] = p.zig_x[t]; t_zf[t] = p.zig_f[t]; }
  for (u32 t = threadIdx.x; t < 256; t += blockDim.x) t_et[t] = p.exp_tab[t];
  u8* t_leader = reinterpret_cast<u8*>(lds + 770 + LBFT_LDS_DURS);
  u32 n_leader = p.leader_len < LBFT_LDS_LEADERS ? p.leader_len : LBFT_LDS_LEADERS;
  i64* t_dur = reinterpret_cast<i64*>(lds + 770);
  u32 n_dur = 0;
  if constexpr (!SimT<CLS>::PSET) {
    n_dur = p.dur_len < LBFT_LDS_DURS ? p.dur_len : LBFT_LDS_DURS;
    for (u32 t = threadIdx.x; t < n_dur; t += blockDim.x) t_dur[t] = p.dur_tab[t];
  }
  for (u32 t = threadIdx.x; t < n_leader; t += blockDim.x) t_leader[t] = p.leader_tab[t];
  u32* t_weights = reinterpret_cast<u32*>(lds + 770 + LBFT_LDS_DURS + LBFT_LDS_LEADERS / 8);
  for (u32 t = threadIdx.x; t < p.n; t += blockDim.x) t_weights[t] = p.weights[t];
  __syncthreads();
  u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  u64* keys = lds + LBFT_TABLE_U64 + (size_t)wave * p.ql * p.lpw + lane;
  u32* metas = reinterpret_cast<u32*>(lds + LBFT_TABLE_U64 + (size_t)nwaves * p.ql * p.lpw) + (size_t)wave * p.ql * p.lpw + lane;  // (class 0: unused)
  u32 i = (blockIdx.x * nwaves + wave) * p.lpw + lane;
  bool active = lane < p.lpw && i < p.m;
  bool done = true;
  const u32 tw = SimT<CLS>::TILE64 ? 64u : SimT<CLS>::IMAJOR ? 1u : p.tw;
  u32 tile_idx = __builtin_amdgcn_readfirstlane(((blockIdx.x * nwaves + wave) * p.lpw) / tw);
  char* tile = reinterpret_cast<char*>(state) + (size_t)tile_idx * p.total_words * ((size_t)4 * tw);
  if (active) {
    S s(p, tile, SimT<CLS>::IMAJOR ? lane * (p.total_words * 4u) : (i & (tw - 1u)) * 4u, 0);
    if (s.ld(I_DONE) == 0) {
      if constexpr (SimT<CLS>::PSET) s.load_set(sets[set_of[i]]);
      if constexpr (SimT<CLS>::CTIME) s.attach_commit_times(ctimes, i * p.n);
      s.attach_queue(keys, metas, p.lpw, p.ql);
      s.attach_tables(t_zx, t_zf, t_et);
      s.attach_round_tables(t_leader, n_leader, SimT<CLS>::PSET ? nullptr : t_dur, n_dur);
      s.attach_weights(t_weights);
      if (p.n > 16) {  // receiver / sender lists of process_node_actions
        u8* lists = reinterpret_cast<u8*>(lds) + run_lds_bytes_dev(p.ql, p.lpw, SimT<CLS>::C0 ? 8u : 12u, nwaves);
        s.attach_peer_list(lists + ((size_t)wave * p.lpw + lane) * LBFT_MAX_NODES);
      }
      if (SimT<CLS>::C0 && p.n <= 4) {  // the nodes' hcbr buffers
        u32* hcb = reinterpret_cast<u32*>(reinterpret_cast<u8*>(lds) + run_lds_bytes_dev(p.ql, p.lpw, 8u, nwaves));
        s.attach_hcbr(hcb + (size_t)wave * LBFT_LDS_HCBR_WORDS * p.lpw + lane);
      }
      s.load_scalars();
      s.queue_to_lds();
      s.hcbr_to_lds();
      done = s.run();
      s.queue_from_lds();
      s.hcbr_from_lds();
      s.store_scalars(done);
    }
  }
  unsigned long long pending = __ballot(active && !done);
  if (pending && lane == (u32)(__ffsll((long long)pending) - 1)) atomicAdd(unfinished, (u32)__popcll(pending));
}

#endif  // LBFT_LANE_RUN_H
