// lbft_paramsets.hip -- HIP kernels (gfx950) of parameter-set batches (lbft_batch_create_param_sets): one batch in which every instance
// runs one of up to LBFT_MAX_PARAM_SETS sets of delay, pacemaker and loss parameters.
//
// The step is lbft_core.h's, instantiated for the classes K_SMALL_SETS / K_MID_SETS / K_GENERIC_SETS: the K_SMALL / K_MID / K_GENERIC
// step whose accessors of those parameters (SimT::MU, LAMBDA, DUR_TAB, DROP_PPM, ...) read the lane's own set, loaded once at kernel entry
// (SimT::load_set), instead of the batch-wide Params.  Everything else -- network size, voting rights, protocol mode, capacities, state
// layout, LDS layout (lbft_launch.h) -- is the batch's, so the host side of liblbft_hip.so sizes and reads back these batches as any other.
// Built as a library of its own (build.py): the code object of liblbft_hip.so, whose kernels are pinned byte for byte by the codegen
// manifest, does not change.
#include <hip/hip_runtime.h>

#include "../../include/lbft.h"
#include "lbft_core.h"
#include "lbft_paramsets.h"

using namespace lbft;

#include "lbft_launch.h"

// Simulator::new for every instance: init() draws the startup times with the set's delay parameters.
__global__ __launch_bounds__(LBFT_BLOCK) void lbft_k_ps_init(Params p, u32* __restrict__ state, const u64* __restrict__ seeds,
                                                              const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of) {
  u32 i = blockIdx.x * p.lpw + threadIdx.x;
  if (threadIdx.x >= p.lpw || i >= p.m) return;
  SimTSets<K_GENERIC_SETS> s(p, state, i);
  s.load_set(sets[set_of[i]]);
  s.init(seeds[i]);
}

// Simulator::loop_until for every instance: the lane-private event loop of lbft_k_run0 / lbft_k_run<1> (lbft_hip.hip, run_body's last
// branch) with the same LDS layout.  The LDS copy of the duration table is not used: each lane reads its set's table from HBM (L2-resident).
template <int CLS>
__device__ __forceinline__ void ps_run_body(const Params& p, u32* __restrict__ state, u32* __restrict__ unfinished, const ParamSetDev* __restrict__ sets,
                                            const u8* __restrict__ set_of) {
  static_assert(!SimT<CLS>::COOP && !SimT<CLS>::POPC && !SimT<CLS>::WUNI && !SimT<CLS>::QUAD && SimT<CLS>::PSET, "lane-private classes only");
  extern __shared__ u64 lds[];
  const u32 nwaves = blockDim.x >> 6;
  u64* t_zx = lds;
  u64* t_zf = lds + 257;
  u64* t_et = lds + 514;
  for (u32 t = threadIdx.x; t < 257; t += blockDim.x) { t_zx[t] = p.zig_x[t]; t_zf[t] = p.zig_f[t]; }
  for (u32 t = threadIdx.x; t < 256; t += blockDim.x) t_et[t] = p.exp_tab[t];
  u8* t_leader = reinterpret_cast<u8*>(lds + 770 + LBFT_LDS_DURS);
  u32 n_leader = p.leader_len < LBFT_LDS_LEADERS ? p.leader_len : LBFT_LDS_LEADERS;
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
    SimTSets<CLS> s(p, tile, SimT<CLS>::IMAJOR ? lane * (p.total_words * 4u) : (i & (tw - 1u)) * 4u, 0);
    if (s.ld(I_DONE) == 0) {
      s.load_set(sets[set_of[i]]);
      s.attach_queue(keys, metas, p.lpw, p.ql);
      s.attach_tables(t_zx, t_zf, t_et);
      s.attach_round_tables(t_leader, n_leader, nullptr, 0);
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

// Small class (lbft_k_run0's geometry: two wavefronts per SIMD): n <= 16, honest, lossless, no trace, reference routing.
__global__ __launch_bounds__(LBFT_RUN_BLOCK) __attribute__((amdgpu_waves_per_eu(LBFT_RUN_WAVES_PER_SIMD, LBFT_RUN_WAVES_PER_SIMD)))
void lbft_k_ps_run0(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of) {
  ps_run_body<K_SMALL_SETS>(p, state, unfinished, sets, set_of);
}
// Mid class (lbft_k_run<1>'s geometry: one wavefront per SIMD, the whole register file): n <= 32, every feature.
__global__ __launch_bounds__(64 * LBFT_RUN_WAVES_FULL)
void lbft_k_ps_run1(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of) {
  ps_run_body<K_MID_SETS>(p, state, unfinished, sets, set_of);
}

extern "C" {

__attribute__((visibility("default"))) hipError_t lbft_ps_launch_init(const Params* p, u32* state, const u64* seeds, const ParamSetDev* sets, const u8* set_of,
                                                                     u32 grid, hipStream_t stream) {
  lbft_k_ps_init<<<grid, LBFT_BLOCK, 0, stream>>>(*p, state, seeds, sets, set_of);
  return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t lbft_ps_launch_run(int cls, const Params* p, u32* state, u32* unfinished, const ParamSetDev* sets,
                                                                    const u8* set_of, u32 grid, u32 block, size_t lds_bytes, hipStream_t stream) {
  if (cls != K_SMALL && cls != K_MID) return hipErrorInvalidValue;
  const void* fn = cls == K_SMALL ? reinterpret_cast<const void*>(lbft_k_ps_run0) : reinterpret_cast<const void*>(lbft_k_ps_run1);
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return e;
  if (cls == K_SMALL) lbft_k_ps_run0<<<grid, block, lds_bytes, stream>>>(*p, state, unfinished, sets, set_of);
  else lbft_k_ps_run1<<<grid, block, lds_bytes, stream>>>(*p, state, unfinished, sets, set_of);
  return hipGetLastError();
}

}  // extern "C"
