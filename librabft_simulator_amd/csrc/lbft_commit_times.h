// lbft_commit_times.h -- the interface between liblbft_hip.so and liblbft_commit_times.so (the kernels of batches that record commit
// times, lbft_batch_record_commit_times).  As liblbft_paramsets.so, the second library is a code object of its own so that the machine code
// of the first stays exactly what it was; liblbft_hip.so opens it on first use (dlopen beside itself) and calls these launchers on the
// batch's stream.
#ifndef LBFT_COMMIT_TIMES_H
#define LBFT_COMMIT_TIMES_H

#include <hip/hip_runtime.h>

#include "lbft_core.h"

#define LBFT_COMMIT_TIMES_LIB "liblbft_commit_times.so"

extern "C" {
// One launch of the commit-time twin of the run kernel of class `cls` (K_SMALL: lbft_k_run0's geometry, K_MID: lbft_k_run<1>'s) with the
// geometry prepare_run chose.  sets / set_of: a parameter-set batch's (both NULL for a plain batch).  ctimes: the batch's commit-time
// buffer, [instance][node][p->lcap] i32.
typedef hipError_t (*lbft_ct_run_fn)(int cls, const lbft::Params* p, lbft::u32* state, lbft::u32* unfinished, const lbft::ParamSetDev* sets,
                                     const lbft::u8* set_of, lbft::i32* ctimes, lbft::u32 grid, lbft::u32 block, size_t lds_bytes,
                                     hipStream_t stream);
// Commit-latency histogram of a finished run, accumulated into hist[group * bins + bin] and stats[group * 4 + {samples, sum, ~min, max}]
// (both zeroed by the caller; the minimum is accumulated as the maximum of its complement).  Groups: grp_inst lists the instances of
// group g at [grp_off[g], grp_off[g + 1]); grp_inst == NULL = one group of every instance.  max_group: instances of the largest group.
typedef hipError_t (*lbft_ct_hist_fn)(const lbft::Params* p, const lbft::u32* state, const lbft::i32* ctimes, const lbft::u32* grp_inst,
                                      const lbft::u32* grp_off, lbft::u32 n_groups, lbft::u32 max_group, lbft::u32 bin_width, lbft::u32 bins,
                                      unsigned long long* hist, unsigned long long* stats, hipStream_t stream);
// Commit timelines of a finished run (lbft_k_ct_timeline; groups as above, hist and stats zeroed by the caller).  stalls == 0: the
// series, hist[group * bins + bin of the commit time] per committed entry (since_of and stats unused).  stalls != 0: the histogram of
// the gaps between a node's commit instants and stats[group * LBFT_STALL_STATS + family * 4 + {samples, sum, ~min, max}] of the gaps /
// first / tail / longest families (lbft_commit_timeline.h); since_of[group] in [0, p->max_clock], NULL = 0 for every group.
typedef hipError_t (*lbft_ct_timeline_fn)(const lbft::Params* p, const lbft::u32* state, const lbft::i32* ctimes, const lbft::u32* grp_inst,
                                          const lbft::u32* grp_off, lbft::u32 n_groups, lbft::u32 max_group, int stalls,
                                          const lbft::i32* since_of, lbft::u32 bin_width, lbft::u32 bins, unsigned long long* hist,
                                          unsigned long long* stats, hipStream_t stream);
// Commit finality of a finished run (lbft_k_ct_finality; groups as above, every output zeroed by the caller): per entry of an instance's
// chain the times at which the first node, nodes holding `valid` and `quorum` voting rights and every node had committed it
// (lbft_commit_finality.h; include/lbft.h: lbft_batch_commit_finality).  finality_hist / spread_hist[group * bins + bin],
// first_committer[group * p->n + node], stats[group * LBFT_FINALITY_STATS + family * 4 + {samples, sum, ~min, max}].  p->n <= 32.
typedef hipError_t (*lbft_ct_finality_fn)(const lbft::Params* p, const lbft::u32* state, const lbft::i32* ctimes, const lbft::u32* grp_inst,
                                          const lbft::u32* grp_off, lbft::u32 n_groups, lbft::u32 max_group, lbft::u32 bin_width, lbft::u32 bins,
                                          unsigned long long* finality_hist, unsigned long long* spread_hist, unsigned long long* first_committer,
                                          unsigned long long* stats, hipStream_t stream);
// Per-instance statistics of a finished run (lbft_k_ct_instances; groups as above, rows zeroed by the caller): rows[instance *
// LBFT_INSTANCE_STATS + family * 4 + {samples, sum, min, max}] of the latency, the four stall and the six finality families, the minimum
// as itself (include/lbft.h: lbft_batch_instance_stats).  since_of[group] in [0, p->max_clock], NULL = 0 for every group.  p->n <= 32.
typedef hipError_t (*lbft_ct_instances_fn)(const lbft::Params* p, const lbft::u32* state, const lbft::i32* ctimes, const lbft::u32* grp_inst,
                                           const lbft::u32* grp_off, lbft::u32 n_groups, lbft::u32 max_group, const lbft::i32* since_of,
                                           unsigned long long* rows, hipStream_t stream);
// Commit phases of a finished run (lbft_k_ct_phases; groups as above, every output zeroed by the caller): the latency histogram's samples
// and the finality's families first .. spread per (group, phase), the phase of an entry being that of its proposal time among the
// group's edges (lbft_commit_phases.h; include/lbft.h: lbft_batch_commit_phases).  edges[group * (phases - 1) + q], checked by the caller:
// each in [0, p->max_clock + 1], none below its predecessor; NULL with phases == 1.  latency_hist / finality_hist[(group * phases +
// phase) * bins + bin], stats[(group * phases + phase) * LBFT_PHASE_STATS + family * 4 + {samples, sum, ~min, max}].  1 <= phases <=
// LBFT_MAX_PHASES, phases x bins < 2^32, p->n <= 32.
typedef hipError_t (*lbft_ct_phases_fn)(const lbft::Params* p, const lbft::u32* state, const lbft::i32* ctimes, const lbft::u32* grp_inst,
                                        const lbft::u32* grp_off, lbft::u32 n_groups, lbft::u32 max_group, const lbft::i32* edges, lbft::u32 phases,
                                        lbft::u32 bin_width, lbft::u32 bins, unsigned long long* latency_hist, unsigned long long* finality_hist,
                                        unsigned long long* stats, hipStream_t stream);
}

#endif  // LBFT_COMMIT_TIMES_H
