// epoch_stats_host_model.cpp -- TEST INFRASTRUCTURE (tests/test_epoch_stats_host.py compiles it with g++): plain batches run through the
// kernel logic on the host (oracle/host_model_common.h; networks above 32 nodes as the run-time-generic class on the planner's own
// capacities), then every instance's nodes, chain and block pool walked the way lbft_k_ps_epochs (csrc/lbft_paramsets.hip) walks them --
// the node pass, the chain pass, the pool pass, the same steps in the same order over csrc/lbft_epoch_rules.h -- with the chunk width W
// a parameter: a lane is an array element, a shuffle an index, a ballot a loop.  The model, its accessors and the shared steps of the
// walk are tests/pool_walk_host.h's; every read of a block record goes through its counted reader: the walk must give 0.  The state
// stays in the handle, so a test can edit log entries, block fields and fault words and walk again.
// With -DEPM_MAIN the file is a program of its own (for a run under the address and undefined-behaviour sanitizers).
#include "pool_walk_host.h"
#include "../librabft_simulator_amd/csrc/lbft_epoch_rules.h"

static_assert(LBFT_EPOCH_STATS == EP_FAMILIES * 4 && LBFT_EPOCH_FAMILIES == EP_FAMILIES && LBFT_EPOCH_COLUMNS == EP_COLUMNS && LBFT_EPOCH_MAX_BINS == EP_MAX_BINS, "lbft.h");

struct EpOut {
  u32 bin_width, bins, epoch_bins;
  u64 *hist, *table;
  GsStat st[EP_FAMILIES];
  u64 unchecked;
};

// One instance, as one wavefront of the kernel with W lanes.
static void walk_instance(const Params& p, u32* state, u32 i, u32 W, EpOut& o) {
  const u32 n = p.n, lcap = p.lcap, lg = p.off_log, eb = o.epoch_bins;
  Sim s(p, state, i);
  if (s.ld(I_FAULT) != 0) return;
  // node pass
  const CwChain ch = cw_chain_of(s, n, lcap);
  u32 e_max = 0;
  for (u32 j = 0; j < n; j++) e_max = s.nfm(j, NF_EPOCH) > e_max ? s.nfm(j, NF_EPOCH) : e_max;
  for (u32 j = 0; j < n; j++) { gs_stat_add(o.st[EP_NODE_EPOCH], s.nfm(j, NF_EPOCH)); gs_stat_add(o.st[EP_BEHIND], e_max - s.nfm(j, NF_EPOCH)); }
  const u32 row = lg + ch.ref * lcap, nb = cw_pool_blocks(s, p);
  const CwRec rec{s, nb, o.unchecked};
  // chain pass
  u32 L = ch.L;
  u32 carry_e = 0, carry_r = 0, carry_start = 0, tip_e = 0, segments = 0;
  i32 carry_g = 0, carry_first_g = 0;
  struct Lane { u32 epoch, round; i32 g; bool start; };
  for (u32 c0 = 0; c0 < L; c0 += W) {
    std::vector<Lane> ln(W, Lane{});
    const CwChunk ck = cw_chunk(s, row, c0, L, nb, W);
    const u32 nv = ck.nv;
    for (u32 sl = 0; sl < nv; sl++) {
      Lane& l = ln[sl];
      const u32 y = ck.y[sl];
      l.epoch = rec(y, B_EPOCH); l.round = rec(y, B_ROUND);
      const u32 author = rec(y, B_LINK) >> 16;
      l.g = (i32)(s.nfm(author, NF_STARTUP) + rec(y, B_TIME));  // cw_proposal
    }
    u64 starts = 0;
    for (u32 sl = 0; sl < nv; sl++) {
      ln[sl].start = ep_segment_start(c0 + sl, ln[sl].epoch, sl == 0 ? carry_e : ln[sl - 1].epoch);
      if (ln[sl].start) starts |= 1ull << sl;
    }
    for (u32 sl = 0; sl < nv; sl++) {
      const Lane& l = ln[sl];
      const u32 k = c0 + sl;
      const u32 pe = sl == 0 ? carry_e : ln[sl - 1].epoch, pr = sl == 0 ? carry_r : ln[sl - 1].round;
      const i32 pg = sl == 0 ? carry_g : ln[sl - 1].g;
      const u64 below = starts & ((1ull << sl) - 1ull);
      const i32 first_g = below ? ln[ep_start_lane(below)].g : carry_first_g;
      if (l.start && k > 0) {
        const u32 handover = ep_clamped(l.g, pg), duration = ep_clamped(pg, first_g), x_prev = ep_bin(pe, eb);
        o.hist[gs_bin(handover, o.bin_width, o.bins)]++;
        gs_stat_add(o.st[EP_LENGTH], k - ep_segment_first(below, c0, carry_start));
        gs_stat_add(o.st[EP_DURATION], duration); gs_stat_add(o.st[EP_LAST_ROUND], pr); gs_stat_add(o.st[EP_HANDOVER], handover);
        o.table[ep_cell(x_prev, EP_COL_COMPLETE)]++;
        o.table[ep_cell(x_prev, EP_COL_DURATION)] += duration;
        o.table[ep_cell(ep_bin(l.epoch, eb), EP_COL_HANDOVER)] += handover;
      }
      const u32 x = ep_bin(l.epoch, eb);
      o.table[ep_cell(x, EP_COL_ENTRIES)]++;
      if (l.start) { gs_stat_add(o.st[EP_FIRST_ROUND], l.round); o.table[ep_cell(x, EP_COL_SEGMENTS)]++; }
    }
    if (starts) carry_first_g = ln[ep_highest(starts)].g;
    carry_start = ep_carry_start(starts, c0, carry_start);
    segments += (u32)__builtin_popcountll(starts);
    carry_e = ln[W - 1].epoch; carry_r = ln[W - 1].round; carry_g = ln[W - 1].g;
    if (nv) tip_e = ln[nv - 1].epoch;
    if (cw_ends(ck)) L = c0 + nv;
  }
  // pool pass
  u32 stranded = 0;
  for (u32 b0 = 1; b0 <= nb; b0 += W)
    for (u32 sl = 0; sl < W && b0 + sl <= nb; sl++) {
      const u32 b = b0 + sl;
      const u32 epoch = rec(b, B_EPOCH), x = ep_bin(epoch, eb);
      const bool off = ep_stranded(cw_pool_member(s, row, rec(b, B_DEPTH), L, b), L != 0, epoch, tip_e);
      o.table[ep_cell(x, EP_COL_BLOCKS)]++;
      if (off) { o.table[ep_cell(x, EP_COL_STRANDED)]++; stranded++; }
    }
  gs_stat_add(o.st[EP_SEGMENTS], segments); gs_stat_add(o.st[EP_STRANDED], stranded); gs_stat_add(o.st[EP_BLOCKS], nb);
}

extern "C" {

void* epm_create(const lbft_config* base, const uint64_t* seeds, size_t m, int64_t max_clock, uint32_t threads, uint32_t* info) { return pw_create(base, seeds, m, max_clock, threads, info, true); }
void epm_destroy(void* handle) { pw_destroy(handle); }
void epm_counts(void* handle, uint32_t* commit_counts, uint32_t* faults, uint32_t* nblocks, int32_t* startup, uint32_t* epochs) { pw_counts(handle, commit_counts, faults, nblocks, startup, epochs); }
void epm_chain(void* handle, uint32_t inst, uint32_t* ref, uint32_t* length) { pw_chain(handle, inst, ref, length); }
uint32_t epm_log(void* handle, uint32_t inst, uint32_t node, uint32_t k, int set, uint32_t value) { return pw_log(handle, inst, node, k, set, value); }
void epm_set_fault(void* handle, uint32_t inst, uint32_t value) { pw_set_fault(handle, inst, value); }
uint32_t epm_block(void* handle, uint32_t inst, uint32_t b, uint32_t what, int set, uint32_t value) { return pw_block(handle, inst, b, what, set, value); }

// Every instance walked in chunks of W lanes (1 .. 64), one group: hist [bins], table [epoch_bins * 7], stats [40], all zeroed here
// first.  check[0] = block-record reads with an unchecked id (0 is right).  -> 0, < 0 on a bad argument
int epm_walk(void* handle, uint32_t W, uint32_t bin_width, uint32_t bins, uint32_t epoch_bins, uint64_t* hist, uint64_t* table, uint64_t* stats,
             uint64_t* check) {
  PwModel* h = static_cast<PwModel*>(handle);
  if (!h || W == 0 || W > 64 || bin_width == 0 || bins == 0 || epoch_bins == 0 || epoch_bins > EP_MAX_BINS || !hist || !table || !stats || !check) return -1;
  const Params& p = h->tb.p;
  EpOut o = {};
  o.bin_width = bin_width; o.bins = bins; o.epoch_bins = epoch_bins; o.hist = hist; o.table = table;
  for (u32 k = 0; k < bins; k++) hist[k] = 0;
  for (u32 k = 0; k < epoch_bins * EP_COLUMNS; k++) table[k] = 0;
  for (size_t i = 0; i < h->m; i++) walk_instance(p, h->state.data(), (u32)i, W, o);
  for (u32 f = 0; f < EP_FAMILIES; f++) {
    const GsStat& g = o.st[f];
    stats[4 * f] = g.cnt; stats[4 * f + 1] = g.sum; stats[4 * f + 2] = g.cnt ? ~g.nmin : 0; stats[4 * f + 3] = g.max;
  }
  check[0] = o.unchecked;
  return 0;
}

}  // extern "C"

#ifdef EPM_MAIN
#include <stdio.h>
#include <string.h>

// 4 nodes, an epoch every 5 commands, to clock 1000: every W gives the same arrays and the identities hold -- as the run left the state,
// then with a log entry of 0, one far above the pool, epochs that fall and one of 2^31, times near 2^30 and a fault word
int main() {
  lbft_config c;
  memset(&c, 0, sizeof(c));
  c.num_nodes = 4; c.mean = 10.0; c.variance = 4.0; c.commands_per_epoch = 5; c.target_commit_interval = 100000;
  c.delta = 20; c.gamma = 2.0; c.lambda = 0.5; c.quirks = 3;
  const uint64_t seeds[3] = {1, 2, 3};
  uint32_t info[4];
  void* h = epm_create(&c, seeds, 3, 1000, 1, info);
  if (!h) { printf("no batch\n"); return 2; }
  const u32 bins = 3, eb = 4;
  int bad = 0;
  for (int pass = 0; pass < 6; pass++) {
    u32 ref, len;
    epm_chain(h, 0, &ref, &len);
    if (pass == 1) epm_log(h, 0, ref, 12, 1, 0);
    if (pass == 2) { epm_chain(h, 1, &ref, &len); epm_log(h, 1, ref, 7, 1, 0xfffffff0u); }
    if (pass == 3) { epm_block(h, 0, epm_log(h, 0, ref, 3, 0, 0), 0, 1, 0x80000000u); epm_block(h, 0, epm_log(h, 0, ref, 8, 0, 0), 0, 1, 0); }
    if (pass == 4) for (u32 k = 0; k < 12; k += 2) epm_block(h, 0, epm_log(h, 0, ref, k, 0, 0), 3, 1, 0x3fffff00u);
    if (pass == 5) epm_set_fault(h, 2, 8);
    std::vector<u64> first;
    for (u32 W : {1u, 7u, 64u}) {
      std::vector<u64> out(bins + eb * EP_COLUMNS + LBFT_EPOCH_STATS);
      u64 check[1];
      u64 *hist = out.data(), *table = hist + bins, *stats = table + eb * EP_COLUMNS;
      if (epm_walk(h, W, 400, bins, eb, hist, table, stats, check) != 0 || check[0]) bad++;
      if (first.empty()) first = out; else if (first != out) bad++;
      u64 col[EP_COLUMNS] = {}, binned = 0;
      for (u32 x = 0; x < eb; x++) for (u32 q = 0; q < EP_COLUMNS; q++) col[q] += table[ep_cell(x, q)];
      for (u32 k = 0; k < bins; k++) binned += hist[k];
      if (col[EP_COL_SEGMENTS] != stats[4 * EP_FIRST_ROUND] || col[EP_COL_SEGMENTS] != stats[4 * EP_SEGMENTS + 1] || col[EP_COL_COMPLETE] != stats[4 * EP_LENGTH]) bad++;
      if (col[EP_COL_DURATION] != stats[4 * EP_DURATION + 1] || col[EP_COL_HANDOVER] != stats[4 * EP_HANDOVER + 1] || binned != stats[4 * EP_HANDOVER]) bad++;
      if (col[EP_COL_STRANDED] != stats[4 * EP_STRANDED + 1] || col[EP_COL_BLOCKS] != stats[4 * EP_BLOCKS + 1]) bad++;
      if (stats[4 * EP_BLOCKS] != (pass == 5 ? 2u : 3u) || stats[4 * EP_SEGMENTS + 1] < 6) bad++;
      if (pass == 4 && stats[4 * EP_HANDOVER + 3] < 0x3f000000u && stats[4 * EP_DURATION + 3] < 0x3f000000u) bad++;
    }
  }
  epm_destroy(h);
  printf("%s\n", bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
#endif
