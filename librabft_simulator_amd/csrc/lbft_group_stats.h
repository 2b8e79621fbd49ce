// lbft_group_stats.h -- the one accumulation scheme of the statistics per group that are computed on the device
// (lbft_batch_commit_latency_histogram, lbft_batch_commit_series / lbft_batch_commit_stalls, lbft_batch_round_stats; include/lbft.h).
// The kernels (lbft_k_ct_latency_hist, lbft_k_ct_timeline, lbft_k_rs_rounds) differ in how they turn a finished run into u32 samples;
// what they do with a sample is here, and the host shims of the CPU tests compile the same arithmetic.  The first part needs nothing
// but <stdint.h>.
//
// What makes the results bit-reproducible and safe:
//   - every accumulation is an integer add or an integer max, so the order of the atomics does not matter;
//   - the minimum is carried as max(~v): zero-initialised and combined by max like the rest (the host un-complements it where the
//     sample count is non-zero);
//   - a workgroup counts into u32 LDS bins, so a grid has at least gs_workgroups()'s floor of workgroups per group: none can see
//     2^32 samples;
//   - a histogram wider than the LDS holds is binned in passes (for base = 0; base < bins; base += LDS bins), each pass between
//     barriers: gs_lds_clear, barrier, gs_lds_count of every sample, (first pass: gs_reduce_to_lds), barrier, gs_lds_flush,
//     (first pass: gs_stats_out), barrier.  The statistics are taken in the first pass alone.
#ifndef LBFT_GROUP_STATS_H
#define LBFT_GROUP_STATS_H

#include <stdint.h>

#ifndef LBFT_HD  // (lbft_math.h's, when that came first)
#if defined(__HIPCC__)
#define LBFT_HD __host__ __device__ __forceinline__
#else
#define LBFT_HD inline
#endif
#endif

// One sample family's statistics as they are accumulated: samples, sum, max(~value) and max.  A call's stats are families x these 4.
struct GsStat {
  uint64_t cnt, sum, nmin, max;
};
LBFT_HD void gs_stat_add(GsStat& s, uint32_t v) {
  s.cnt++; s.sum += v;
  s.nmin = ~(uint64_t)v > s.nmin ? ~(uint64_t)v : s.nmin;
  s.max = v > s.max ? v : s.max;
}
// min(v / bin_width, bins - 1): the last bin also counts everything above it.  bin_width >= 1, bins >= 1.  (Every sample is a clock
// difference, a round count or a node count below 2^31: a 32-bit division, which the GPU emulates in a fraction of a 64-bit one's
// instructions.)
LBFT_HD uint32_t gs_bin(uint32_t v, uint32_t bin_width, uint32_t bins) {
  const uint32_t q = v / bin_width;
  return q < bins - 1u ? q : bins - 1u;
}
// Workgroups per group (gridDim.x): about `target` workgroups in all -- each adds its LDS histogram to the global one, so fewer,
// longer-running workgroups mean fewer global atomics per bin --, never so few that one could count 2^32 of a group's at most
// max_samples samples into a bin of its u32 LDS histogram, never more than the `steps` a workgroup's stride over its group has.
LBFT_HD uint64_t gs_workgroups(uint64_t target, uint64_t n_groups, uint64_t steps, uint64_t max_samples) {
  uint64_t gx = target / n_groups ? target / n_groups : 1;
  const uint64_t least = (max_samples >> 31) + 1;
  if (gx < least) gx = least;
  if (gx > steps) gx = steps;
  return gx;
}

#if defined(__HIPCC__)
// The instances of group g: grp_inst[first .. first + cnt), or every instance of a batch of m without an index (grp_inst == NULL).
__device__ __forceinline__ uint2 gs_group(const uint32_t* grp_inst, const uint32_t* grp_off, uint32_t g, uint32_t m) {  // {first, cnt}
  const uint32_t first = grp_inst ? grp_off[g] : 0u, cnt = grp_inst ? grp_off[g + 1] - first : m;
  return make_uint2(first, cnt);
}
__device__ __forceinline__ uint32_t gs_instance(const uint32_t* grp_inst, uint32_t first, uint32_t k) {
  return grp_inst ? grp_inst[first + k] : k;
}

// One pass [base, base + span) of a histogram through the workgroup's LDS bins h (BLOCK = the workgroup's threads).
template <uint32_t BLOCK>
__device__ __forceinline__ void gs_lds_clear(uint32_t* h, uint32_t span) {
  for (uint32_t k = threadIdx.x; k < span; k += BLOCK) h[k] = 0;
}
__device__ __forceinline__ void gs_lds_count(uint32_t* h, uint32_t v, uint32_t bin_width, uint32_t bins, uint32_t base, uint32_t span) {
  const uint32_t bin = gs_bin(v, bin_width, bins);
  if (bin >= base && bin - base < span) atomicAdd(&h[bin - base], 1u);
}
// hist = the global histograms [group][bins]: one atomic per non-zero bin.
template <uint32_t BLOCK>
__device__ __forceinline__ void gs_lds_flush(const uint32_t* h, unsigned long long* hist, uint32_t g, uint32_t bins, uint32_t base, uint32_t span) {
  for (uint32_t k = threadIdx.x; k < span; k += BLOCK)
    if (h[k]) atomicAdd(&hist[(size_t)g * bins + base + k], (unsigned long long)h[k]);
}

// The statistics: registers (GsStat st[FAMILIES] of every lane, over the workgroup's whole stride) -> wavefront (butterfly; all 64
// lanes call) -> workgroup (s_stat[FAMILIES * 4] in LDS, by the wavefront's `leader` lane) -> stats[g * WORDS ..] (one global atomic
// per word of a family with samples).  Barriers lie between gs_stats_clear, gs_reduce_to_lds and gs_stats_out: the pass loop's.
template <uint32_t WORDS>
__device__ __forceinline__ void gs_stats_clear(unsigned long long* s_stat) {
  if (threadIdx.x < WORDS) s_stat[threadIdx.x] = 0;
}
template <uint32_t FAMILIES>
__device__ __forceinline__ void gs_reduce_to_lds(const GsStat* st, unsigned long long* s_stat, bool leader) {
  for (uint32_t f = 0; f < FAMILIES; f++) {
    unsigned long long cnt = st[f].cnt, sum = st[f].sum, nmin = st[f].nmin, max = st[f].max;
    for (int d = 32; d; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(nmin, d, 64); nmin = o > nmin ? o : nmin; }
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(max, d, 64); max = o > max ? o : max; }
    if (leader && cnt) {
      atomicAdd(&s_stat[f * 4 + 0], cnt); atomicAdd(&s_stat[f * 4 + 1], sum);
      atomicMax(&s_stat[f * 4 + 2], nmin); atomicMax(&s_stat[f * 4 + 3], max);
    }
  }
}
template <uint32_t WORDS>
__device__ __forceinline__ void gs_stats_out(const unsigned long long* s_stat, unsigned long long* stats, uint32_t g) {
  if (threadIdx.x < WORDS && s_stat[threadIdx.x & ~3u]) {
    if ((threadIdx.x & 3u) < 2u) atomicAdd(&stats[g * WORDS + threadIdx.x], s_stat[threadIdx.x]);
    else atomicMax(&stats[g * WORDS + threadIdx.x], s_stat[threadIdx.x]);
  }
}
#endif  // __HIPCC__

#endif  // LBFT_GROUP_STATS_H
