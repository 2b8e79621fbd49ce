// lbft_paramsets.h -- the interface between liblbft_hip.so and liblbft_paramsets.so (the kernels of parameter-set batches,
// lbft_batch_create_param_sets).  The second library is a code object of its own so that the machine code of the first stays exactly
// what it was; liblbft_hip.so opens it on first use (dlopen beside itself) and calls these launchers on the batch's stream.
#ifndef LBFT_PARAMSETS_H
#define LBFT_PARAMSETS_H

#include <hip/hip_runtime.h>

#include "lbft_core.h"

#define LBFT_PARAMSETS_LIB "liblbft_paramsets.so"

extern "C" {
// Simulator::new for every instance with its set's delay parameters (grid = instances / p->lpw workgroups of LBFT_BLOCK lanes).
// sets: device array of the batch's sets; set_of: device array, set_of[instance] < number of sets.
typedef hipError_t (*lbft_ps_init_fn)(const lbft::Params* p, lbft::u32* state, const lbft::u64* seeds, const lbft::ParamSetDev* sets,
                                      const lbft::u8* set_of, lbft::u32 grid, hipStream_t stream);
// One launch of the run kernel of class `cls` (K_SMALL or K_MID) with the geometry prepare_run chose.
typedef hipError_t (*lbft_ps_run_fn)(int cls, const lbft::Params* p, lbft::u32* state, lbft::u32* unfinished, const lbft::ParamSetDev* sets,
                                     const lbft::u8* set_of, lbft::u32 grid, lbft::u32 block, size_t lds_bytes, hipStream_t stream);
// The fourteen batch counters of a finished run (lbft_batch_counters.h) added to counters[], which the caller zeroed: for batches of
// every kind, plain ones included -- those fall back to lbft_k_finalize when this library is missing.
typedef hipError_t (*lbft_ps_counters_fn)(const lbft::Params* p, const lbft::u32* state, unsigned long long* counters, hipStream_t stream);
// The run load of a finished run (lbft_load_stats.h; lbft_k_ps_load), for batches of every kind.  grp_inst / grp_off: the group index
// (NULL: one group of every instance).  stats != NULL: hist[groups * bins], faults[groups * 32] and stats[groups * 64], which the caller
// zeroed, and rows[m * 16] when that is not NULL; stats == NULL: the rows alone (hist and faults NULL, bins 1).
// A liblbft_paramsets.so built before this launcher existed lacks it and is refused as a whole (load_side_lib fills every slot or
// none): parameter-set batches and the run load then report LBFT_ERR_UNSUPPORTED, and plain batches reduce their counters with
// lbft_k_finalize, as they do when the library is missing.
typedef hipError_t (*lbft_ps_load_fn)(const lbft::Params* p, const lbft::u32* state, const lbft::u32* grp_inst, const lbft::u32* grp_off,
                                      lbft::u32 n_groups, lbft::u32 max_group, lbft::u32 hist_family, lbft::u32 bin_width, lbft::u32 bins,
                                      unsigned long long* hist, unsigned long long* faults, unsigned long long* stats, lbft::u32* rows,
                                      hipStream_t stream);
// The vote statistics of a finished run (lbft_vote_rules.h; lbft_k_ps_votes), for batches of every kind.  grp_inst / grp_off: the group
// index (NULL: one group of every instance).  margin_hist[groups * bins], votes_hist[groups * (n + 1)], node_table[groups * n * 3] and
// stats[groups * 32], which the caller zeroed.  A library built before this launcher existed is refused as a whole, as above.
typedef hipError_t (*lbft_ps_votes_fn)(const lbft::Params* p, const lbft::u32* state, const lbft::u32* grp_inst, const lbft::u32* grp_off,
                                       lbft::u32 n_groups, lbft::u32 max_group, lbft::u32 bin_width, lbft::u32 bins,
                                       unsigned long long* margin_hist, unsigned long long* votes_hist, unsigned long long* node_table,
                                       unsigned long long* stats, hipStream_t stream);
// The epoch statistics of a finished run (lbft_epoch_rules.h; lbft_k_ps_epochs), for batches of every kind.  grp_inst / grp_off: the group
// index (NULL: one group of every instance).  handover_hist[groups * bins], epoch_table[groups * epoch_bins * 7] and stats[groups * 40],
// which the caller zeroed; 1 <= epoch_bins <= 512.  A library built before this launcher existed is refused as a whole, as above.
typedef hipError_t (*lbft_ps_epochs_fn)(const lbft::Params* p, const lbft::u32* state, const lbft::u32* grp_inst, const lbft::u32* grp_off,
                                        lbft::u32 n_groups, lbft::u32 max_group, lbft::u32 bin_width, lbft::u32 bins, lbft::u32 epoch_bins,
                                        unsigned long long* handover_hist, unsigned long long* epoch_table, unsigned long long* stats,
                                        hipStream_t stream);
}

#endif  // LBFT_PARAMSETS_H
