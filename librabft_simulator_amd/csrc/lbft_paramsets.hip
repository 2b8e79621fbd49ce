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
#include "lbft_run_body.h"  // run_body

// Simulator::new for every instance: init() draws the startup times with the set's delay parameters.
__global__ __launch_bounds__(LBFT_BLOCK) void lbft_k_ps_init(Params p, u32* __restrict__ state, const u64* __restrict__ seeds,
                                                              const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of) {
  u32 i = blockIdx.x * p.lpw + threadIdx.x;
  if (threadIdx.x >= p.lpw || i >= p.m) return;
  SimTSets<K_GENERIC_SETS> s(p, state, i);
  s.load_set(sets[set_of[i]]);
  s.init(seeds[i]);
}

// Small class (lbft_k_run0's geometry: two wavefronts per SIMD): n <= 16, honest, lossless, no trace, reference routing.
__global__ LBFT_TWO_WAVE_BOUNDS void lbft_k_ps_run0(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of) {
  run_body<K_SMALL_SETS>(p, state, unfinished, sets, set_of);
}
// Mid class (lbft_k_run<1>'s geometry: one wavefront per SIMD, the whole register file): n <= 32, every feature.
__global__ __launch_bounds__(64 * LBFT_RUN_WAVES_FULL)
void lbft_k_ps_run1(Params p, u32* __restrict__ state, u32* __restrict__ unfinished, const ParamSetDev* __restrict__ sets, const u8* __restrict__ set_of) {
  run_body<K_MID_SETS>(p, state, unfinished, sets, set_of);
}

// The batch counters of a finished run without the State hashes: the tail of lbft_k_finalize (liblbft_hip.so) as a kernel of its own, for
// batches of every kind -- it reads the instance's scalar rows and two words per node through the generic accessors, whatever kernel ran.
// One lane per instance; a workgroup of LBFT_COUNTER_WAVES wavefronts reduces its instances' words (shuffles within a wavefront, then
// LDS across the wavefronts) and adds them to the batch's with ONE atomic per counter: the atomics of a run all go to one 128-byte line.
#include "lbft_batch_counters.h"
#define LBFT_COUNTER_WAVES 16
__global__ __launch_bounds__(64 * LBFT_COUNTER_WAVES) void lbft_k_ps_counters(Params p, const u32* __restrict__ state, unsigned long long* __restrict__ counters) {
  __shared__ u64 part[LBFT_COUNTER_WAVES][C_WORDS];
  u64 c[C_WORDS];
  instance_counter_words(p, state, blockIdx.x * (64 * LBFT_COUNTER_WAVES) + threadIdx.x, c);
  for (int k = 0; k < C_WORDS; k++) {
    u64 r = k >= C_MAXQ ? wave_max(c[k]) : wave_sum(c[k]);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = r;
  }
  __syncthreads();
  if (threadIdx.x >= C_WORDS) return;
  const u32 k = threadIdx.x;
  const bool is_max = k >= C_MAXQ;
  u64 r = part[0][k];
  for (int w = 1; w < LBFT_COUNTER_WAVES; w++) r = is_max ? (part[w][k] > r ? part[w][k] : r) : r + part[w][k];
  if (is_max) atomicMax(&counters[k], (unsigned long long)r);
  else atomicAdd(&counters[k], (unsigned long long)r);
}

extern "C" {

__attribute__((visibility("default"))) hipError_t lbft_ps_launch_counters(const Params* p, const u32* state, unsigned long long* counters, hipStream_t stream) {
  const u32 per_group = 64 * LBFT_COUNTER_WAVES;
  lbft_k_ps_counters<<<(p->m + per_group - 1) / per_group, per_group, 0, stream>>>(*p, state, counters);
  return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t lbft_ps_launch_init(const Params* p, u32* state, const u64* seeds, const ParamSetDev* sets, const u8* set_of,
                                                                     u32 grid, hipStream_t stream) {
  lbft_k_ps_init<<<grid, LBFT_BLOCK, 0, stream>>>(*p, state, seeds, sets, set_of);
  return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t lbft_ps_launch_run(int cls, const Params* p, u32* state, u32* unfinished, const ParamSetDev* sets,
                                                                    const u8* set_of, u32 grid, u32 block, size_t lds_bytes, hipStream_t stream) {
  if (cls != K_SMALL && cls != K_MID) return hipErrorInvalidValue;
  return launch_run_kernel(cls == K_SMALL ? lbft_k_ps_run0 : lbft_k_ps_run1, grid, block, lds_bytes, stream, *p, state, unfinished, sets, set_of);
}

}  // extern "C"
