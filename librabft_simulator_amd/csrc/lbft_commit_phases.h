// lbft_commit_phases.h -- the arithmetic of the commit phases (lbft_batch_commit_phases, include/lbft.h): the second grouping axis of the
// commit statistics.  A group's edges e_0 <= e_1 <= ... cut the clock into phases; a sample of the latency histogram or of the commit
// finality belongs to the phase of its entry's PROPOSAL time, and each (group, phase) has its own statistics and its own slice of the
// histograms.  The samples themselves are made by the rule headers of those calls (lbft_commit_finality.h, lbft_chain_rules.h); here is
// the phase of a time, the bin of a (phase, sample) pair in the virtual histogram of phases x bins bins, the order of the families and
// the place of a family's words in a group's block of statistics.  Compiled by the device kernel (lbft_k_ct_phases,
// lbft_commit_times.hip) and by a plain C++ host shim (tests/commit_phases_host.cpp), so the CPU tests check the same code the GPU runs.
// Needs nothing but <stdint.h> and lbft_group_stats.h, which says what becomes of a sample.
#ifndef LBFT_COMMIT_PHASES_H
#define LBFT_COMMIT_PHASES_H

#include <stdint.h>

#include "lbft_group_stats.h"  // LBFT_HD; gs_bin

#define CPH_MAX_PHASES 8u  // LBFT_MAX_PHASES: at most 7 edges per group

// The families of a (group, phase), stats[(g * phases + p) * CPH_STATS + 4 * family + {samples, sum, min, max}]: the latency histogram's
// sample, then families 0 .. 4 of the commit finality (FIN_FIRST .. FIN_SPREAD, in their order: CPH_FINALITY + FIN_*).
enum { CPH_LATENCY = 0, CPH_FINALITY = 1, CPH_FAMILIES = 6, CPH_STATS = CPH_FAMILIES * 4 };

// The phase of a time t: the number of edges at or below it, so phase p covers [e_{p-1}, e_p).  Equal edges give an empty phase, an
// edge 0 leaves phase 0 empty, an edge above every time is never reached.  A count without a branch and without the number of edges:
// edges holds CPH_MAX_PHASES - 1 words (the kernel's copy in LDS, the shim's array), the group's phases - 1 edges and CPH_NO_EDGE in the
// rest, which lies above every time (a clock is at most LBFT_MAX_CLOCK = 2^31 - 3, an edge at most one more).
#define CPH_NO_EDGE 0x7fffffff
LBFT_HD uint32_t cph_phase(const int32_t* edges, int32_t t) {
  uint32_t p = 0;
  for (uint32_t q = 0; q < CPH_MAX_PHASES - 1u; q++) p += (uint32_t)(edges[q] <= t);
  return p;
}

// The two histograms of a group are one virtual histogram each, of phases x bins bins: phase p's slice starts at p * bins.  (groups x
// phases x bins <= 2^31: 32-bit.)  It is binned in passes [base, base + span) of the workgroup's LDS bins like any other.
LBFT_HD uint32_t cph_bin(uint32_t phase, uint32_t v, uint32_t bin_width, uint32_t bins) { return phase * bins + gs_bin(v, bin_width, bins); }
LBFT_HD bool cph_in_pass(uint32_t vbin, uint32_t base, uint32_t span) { return vbin >= base && vbin - base < span; }

// Word w of family f of phase p in a group's block of phases x CPH_STATS words.
LBFT_HD uint32_t cph_word(uint32_t phase, uint32_t family, uint32_t w) { return phase * CPH_STATS + family * 4u + w; }

#endif  // LBFT_COMMIT_PHASES_H
