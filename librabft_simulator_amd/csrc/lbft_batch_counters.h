// lbft_batch_counters.h -- the fourteen batch counters of a finished run (lbft_counters), as both kernels that reduce them see them:
// lbft_k_finalize (lbft_hip.hip: the State hashes, then the counters) and lbft_k_ps_counters (lbft_paramsets.hip: the counters alone).
// One lane = one instance; a wavefront reduces its lanes' words by shuffles.  lbft_k_finalize then adds them to the batch's with one
// atomic per wavefront and counter, lbft_k_ps_counters per workgroup of sixteen wavefronts: the atomics of one run all go to one
// 128-byte line and are served one after the other (65 536 instances: 0.136 ms with a wavefront's 14 336 atomics, 0.023 ms with a
// workgroup's 896; EXPERIMENTS.md "Step tail").
// lbft_hip.hip includes it at the place where it used to define the slots and the wavefront reductions: the machine code of
// lbft_k_finalize is pinned byte for byte (tests/golden/kernel_manifest.json) and stays what it was.  For the same reason that kernel
// keeps its own written-out copy of instance_counter_words' body (calling a shared function gave it another instruction schedule);
// whoever changes one changes the other, and every request for State hashes compares the two kernels' words (materialise_hashes).
#ifndef LBFT_BATCH_COUNTERS_H
#define LBFT_BATCH_COUNTERS_H

#include "lbft_core.h"

__device__ __forceinline__ lbft::u64 wave_sum(lbft::u64 v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ lbft::u64 wave_max(lbft::u64 v) {
  for (int off = 32; off > 0; off >>= 1) { lbft::u64 o = __shfl_down(v, off, 64); v = o > v ? o : v; }
  return v;
}

// [C_EV0, C_MAXQ): summed over the instances; [C_MAXQ, C_WORDS): high-water marks, the largest of any instance
enum CounterSlot { C_EV0 = 0, C_EV1, C_EV2, C_EV3, C_DRAWS, C_ROUNDS, C_COMMITS, C_SCHED, C_FAULTED, C_NFOLD, C_NUPD, C_MAXQ, C_MAXSNAP, C_MAXBLK, C_WORDS };

// Lane i's words of the fourteen counters: what instance i contributes (nothing for i >= p.m).
__device__ __forceinline__ void instance_counter_words(const lbft::Params& p, const lbft::u32* __restrict__ state, lbft::u32 i, lbft::u64 (&c)[C_WORDS]) {
  using namespace lbft;
  for (int k = 0; k < C_WORDS; k++) c[k] = 0;
  if (i < p.m) {
    Sim s(p, const_cast<u32*>(state), i);
    u64 min_round = ~0ULL, min_commits = ~0ULL;
    for (u32 q = 0; q < p.n; q++) {
      u64 nc = s.nfm(q, NF_NCOMMITS), ar = s.nfm(q, NF_PM_ROUND);
      min_round = ar < min_round ? ar : min_round;
      min_commits = nc < min_commits ? nc : min_commits;
    }
    c[C_EV0] = s.ld(I_EV0); c[C_EV1] = s.ld(I_EV1); c[C_EV2] = s.ld(I_EV2); c[C_EV3] = s.ld(I_EV3);
    c[C_DRAWS] = s.ld(I_DRAWS); c[C_ROUNDS] = min_round; c[C_COMMITS] = min_commits; c[C_SCHED] = s.ld(I_STAMP);
    c[C_FAULTED] = s.ld(I_FAULT) ? 1 : 0;
    c[C_NFOLD] = s.ld(I_NFOLD); c[C_NUPD] = s.ld(I_NUPD);
    c[C_MAXQ] = s.ld(I_MAXQ); c[C_MAXSNAP] = s.ld(I_MAXSNAP); c[C_MAXBLK] = s.ld(I_NBLOCKS);
  }
}

#endif  // LBFT_BATCH_COUNTERS_H
