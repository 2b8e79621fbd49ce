// lbft_chain_stats.h -- the interface between liblbft_hip.so and liblbft_chain_stats.so (the kernel of lbft_batch_chain_stats).  As
// the other side libraries, it is a code object of its own so that the machine code of liblbft_hip.so stays exactly what it was;
// liblbft_hip.so opens it on first use (dlopen beside itself) and calls the launcher on the batch's stream.
#ifndef LBFT_CHAIN_STATS_H
#define LBFT_CHAIN_STATS_H

#include <hip/hip_runtime.h>

#include "lbft_core.h"

#define LBFT_CHAIN_STATS_LIB "liblbft_chain_stats.so"

extern "C" {
// Chain statistics of a finished run, accumulated into interval_hist[group * bins + bin], author_blocks[group * p->n + author] and
// stats[group * LBFT_CHAIN_STATS + family * 4 + {samples, sum, ~min, max}] of the interval / length / lag / tenure / differing /
// inversions families (lbft_chain_rules.h); all three zeroed by the caller, the minimum accumulated as the maximum of its complement.
// Groups: grp_inst lists the instances of group g at [grp_off[g], grp_off[g + 1]); grp_inst == NULL = one group of every instance.
// max_group: instances of the largest group.
typedef hipError_t (*lbft_cs_chain_fn)(const lbft::Params* p, const lbft::u32* state, const lbft::u32* grp_inst, const lbft::u32* grp_off,
                                       lbft::u32 n_groups, lbft::u32 max_group, lbft::u32 bin_width, lbft::u32 bins,
                                       unsigned long long* interval_hist, unsigned long long* author_blocks, unsigned long long* stats,
                                       hipStream_t stream);
}

#endif  // LBFT_CHAIN_STATS_H
