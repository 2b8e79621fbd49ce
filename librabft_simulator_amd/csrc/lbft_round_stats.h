// lbft_round_stats.h -- the interface between liblbft_hip.so and liblbft_round_stats.so (the kernel of lbft_batch_round_stats).  As
// liblbft_paramsets.so and liblbft_commit_times.so, the library is a code object of its own so that the machine code of liblbft_hip.so
// stays exactly what it was; liblbft_hip.so opens it on first use (dlopen beside itself) and calls the launcher on the batch's stream.
#ifndef LBFT_ROUND_STATS_H
#define LBFT_ROUND_STATS_H

#include <hip/hip_runtime.h>

#include "lbft_core.h"

#define LBFT_ROUND_STATS_LIB "liblbft_round_stats.so"

extern "C" {
// Round statistics of a finished run with the round trace enabled (p->rcap != 0), accumulated into stay_hist / skew_hist
// [group * bins + bin] and stats[group * LBFT_ROUND_STATS + family * 4 + {samples, sum, ~min, max}] of the stay / skipped / skew / reach
// families (lbft_round_timeline.h); all three zeroed by the caller, the minimum accumulated as the maximum of its complement.  Groups:
// grp_inst lists the instances of group g at [grp_off[g], grp_off[g + 1]); grp_inst == NULL = one group of every instance.  max_group:
// instances of the largest group.
typedef hipError_t (*lbft_rs_rounds_fn)(const lbft::Params* p, const lbft::u32* state, const lbft::u32* grp_inst, const lbft::u32* grp_off,
                                        lbft::u32 n_groups, lbft::u32 max_group, lbft::u32 bin_width, lbft::u32 bins,
                                        unsigned long long* stay_hist, unsigned long long* skew_hist, unsigned long long* stats,
                                        hipStream_t stream);
}

#endif  // LBFT_ROUND_STATS_H
