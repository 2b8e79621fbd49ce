// vote_stats_host_model.cpp -- TEST INFRASTRUCTURE (tests/test_vote_stats_host.py compiles it with g++): plain batches run through the
// kernel logic on the host (oracle/host_model_common.h; networks above 32 nodes as the run-time-generic class on the planner's own
// capacities), then every instance's chain and block pool walked the way lbft_k_ps_votes (csrc/lbft_paramsets.hip) walks them -- the
// node pass, the chain pass, the pool pass, the same steps in the same order over csrc/lbft_vote_rules.h -- with the chunk width W a
// parameter: a lane is an array element, a shuffle an index, a ballot a loop.  The model, its accessors and the shared steps of the
// walk are tests/pool_walk_host.h's; every read of a block record goes through its counted reader: the walk must give 0.  The pool pass
// also holds the membership rule (one gather by ledger depth) against set membership in the chain and counts the blocks on which the two
// differ: 0 as well.  The state stays in the handle, so a test can edit log entries, voter words and fault words and walk again.
// With -DVTM_MAIN the file is a program of its own (for a run under the address and undefined-behaviour sanitizers).
#include <set>

#include "pool_walk_host.h"

struct VtOut {
  u32 bin_width, bins;
  u64 *margin_hist, *votes_hist, *node_table;
  GsStat st[VT_FAMILIES];
  u64 unchecked, membership;
};

// One instance, as one wavefront of the kernel with W lanes.
static void walk_instance(const Params& p, u32* state, u32 i, u32 W, VtOut& o) {
  const u32 n = p.n, lcap = p.lcap, lg = p.off_log, mw = p.mw, quorum = p.quorum, rot = p.rot;
  const bool unit = p.unit_weights != 0;
  Sim s(p, state, i);
  if (s.ld(I_FAULT) != 0) return;
  // node pass
  const CwChain ch = cw_chain_of(s, n, lcap);
  const u32 row = lg + ch.ref * lcap, nb = cw_pool_blocks(s, p);
  const CwRec rec{s, nb, o.unchecked};
  // chain pass
  u32 L = ch.L;
  u32 carry_r = 0, carry_e = 0, tip_r = 0, tip_e = 0;
  struct Lane { u32 round, epoch, votes, weight; };
  for (u32 c0 = 0; c0 < L; c0 += W) {
    std::vector<Lane> ln(W, Lane{});
    const CwChunk ck = cw_chunk(s, row, c0, L, nb, W);
    const u32 nv = ck.nv;
    for (u32 sl = 0; sl < nv; sl++) {
      Lane& l = ln[sl];
      const u32 y = ck.y[sl];
      l.round = rec(y, B_ROUND); l.epoch = rec(y, B_EPOCH);
      const u32 shift = vt_rights_shift(l.epoch, rot, n);
      for (u32 w = 0; w < mw; w++) {
        const u32 v = rec(y, rh_voter_field(w, mw)) & rh_author_bits(w, n);
        l.votes += (u32)__builtin_popcount(v);
        for (u32 m = v; m; m &= m - 1u) {
          const u32 a = 32 * w + (u32)ctz32(m);
          if (!unit) l.weight += p.weights[vt_right_index(a, shift, n)];
          o.node_table[vt_node_cell(a, VT_COL_VOTED)]++;
        }
      }
      if (unit) l.weight = l.votes;
    }
    for (u32 sl = 0; sl < nv; sl++) {
      const Lane& l = ln[sl];
      const u32 k = c0 + sl;
      const u32 pr = sl == 0 ? carry_r : ln[sl - 1].round, pe = sl == 0 ? carry_e : ln[sl - 1].epoch;
      if (l.votes) {
        const u32 margin = vt_margin(l.weight, quorum);
        o.margin_hist[gs_bin(margin, o.bin_width, o.bins)]++;
        gs_stat_add(o.st[VT_VOTES], l.votes); gs_stat_add(o.st[VT_WEIGHT], l.weight); gs_stat_add(o.st[VT_MARGIN], margin);
        o.votes_hist[l.votes]++;
      }
      if (k > 0 && vt_same_epoch(pe, l.epoch)) gs_stat_add(o.st[VT_SKIPPED], vt_skipped(pr, l.round));
    }
    carry_r = ln[W - 1].round; carry_e = ln[W - 1].epoch;
    if (nv) { tip_r = ln[nv - 1].round; tip_e = ln[nv - 1].epoch; }
    if (cw_ends(ck)) L = c0 + nv;
  }
  // pool pass
  std::set<u32> on_chain;  // (the statement the membership rule is held to, not the kernel's way)
  for (u32 k = 0; k < L; k++) on_chain.insert(s.ld(row + k));
  u32 orphaned = 0, pending = 0, certified_off = 0;
  for (u32 b0 = 1; b0 <= nb; b0 += W)
    for (u32 sl = 0; sl < W && b0 + sl <= nb; sl++) {
      const u32 b = b0 + sl;
      const u32 author = rec(b, B_LINK) >> 16, round = rec(b, B_ROUND), epoch = rec(b, B_EPOCH);
      bool certified = false;
      for (u32 w = 0; w < mw; w++) certified |= (rec(b, rh_voter_field(w, mw)) & rh_author_bits(w, n)) != 0;
      const bool member = cw_pool_member(s, row, rec(b, B_DEPTH), L, b);
      if (member != (on_chain.count(b) != 0)) o.membership++;
      const u32 cls = vt_classify(member, L != 0, epoch, round, tip_e, tip_r);
      if (author < n) {
        o.node_table[vt_node_cell(author, VT_COL_PROPOSED)]++;
        if (cls == VT_ORPHAN) o.node_table[vt_node_cell(author, VT_COL_ORPHANED)]++;
      }
      orphaned += cls == VT_ORPHAN; pending += cls == VT_PENDING_BLOCK; certified_off += cls != VT_ON_CHAIN && certified;
    }
  gs_stat_add(o.st[VT_BLOCKS], nb); gs_stat_add(o.st[VT_ORPHANED], orphaned);
  gs_stat_add(o.st[VT_PENDING], pending); gs_stat_add(o.st[VT_CERTIFIED_OFF], certified_off);
}

extern "C" {

void* vtm_create(const lbft_config* base, const uint64_t* seeds, size_t m, int64_t max_clock, uint32_t threads, uint32_t* info) { return pw_create(base, seeds, m, max_clock, threads, info, true); }
void vtm_destroy(void* handle) { pw_destroy(handle); }
void vtm_counts(void* handle, uint32_t* commit_counts, uint32_t* faults, uint32_t* nblocks) { pw_counts(handle, commit_counts, faults, nblocks, nullptr, nullptr); }
void vtm_chain(void* handle, uint32_t inst, uint32_t* ref, uint32_t* length) { pw_chain(handle, inst, ref, length); }
uint32_t vtm_log(void* handle, uint32_t inst, uint32_t node, uint32_t k, int set, uint32_t value) { return pw_log(handle, inst, node, k, set, value); }
void vtm_set_fault(void* handle, uint32_t inst, uint32_t value) { pw_set_fault(handle, inst, value); }

// Every instance walked in chunks of W lanes (1 .. 64), one group: margin_hist [bins], votes_hist [n + 1], node_table [n * 3],
// stats [32], all zeroed here first.  check[0] = block-record reads with an unchecked id, check[1] = pool blocks on which the
// membership rule and set membership differ (0 and 0 are right).  -> 0, < 0 on a bad argument
int vtm_walk(void* handle, uint32_t W, uint32_t bin_width, uint32_t bins, uint64_t* margin_hist, uint64_t* votes_hist, uint64_t* node_table,
             uint64_t* stats, uint64_t* check) {
  PwModel* h = static_cast<PwModel*>(handle);
  if (!h || W == 0 || W > 64 || bin_width == 0 || bins == 0 || !margin_hist || !votes_hist || !node_table || !stats || !check) return -1;
  const Params& p = h->tb.p;
  VtOut o = {};
  o.bin_width = bin_width; o.bins = bins; o.margin_hist = margin_hist; o.votes_hist = votes_hist; o.node_table = node_table;
  for (u32 k = 0; k < bins; k++) margin_hist[k] = 0;
  for (u32 k = 0; k <= p.n; k++) votes_hist[k] = 0;
  for (u32 k = 0; k < p.n * VT_NODE_COLUMNS; k++) node_table[k] = 0;
  for (size_t i = 0; i < h->m; i++) walk_instance(p, h->state.data(), (u32)i, W, o);
  for (u32 f = 0; f < VT_FAMILIES; f++) {
    const GsStat& g = o.st[f];
    stats[4 * f] = g.cnt; stats[4 * f + 1] = g.sum; stats[4 * f + 2] = g.cnt ? ~g.nmin : 0; stats[4 * f + 3] = g.max;
  }
  check[0] = o.unchecked; check[1] = o.membership;
  return 0;
}

// Empties the voter words of pool block b -> the votes it held
uint32_t vtm_clear_voters(void* handle, uint32_t inst, uint32_t b) {
  const Params& p = static_cast<PwModel*>(handle)->tb.p;
  Sim s = pw_sim(handle, inst);
  u32 votes = 0;
  for (u32 w = 0; w < p.mw; w++) {
    votes += (u32)__builtin_popcount(s.bf(b, rh_voter_field(w, p.mw)) & rh_author_bits(w, p.n));
    s.bfs(b, rh_voter_field(w, p.mw), 0);
  }
  return votes;
}

}  // extern "C"

#ifdef VTM_MAIN
#include <stdio.h>
#include <string.h>

// 4 nodes to clock 1000: every W gives the same arrays and the identities hold; then a log entry of 0 and one far above the pool
int main() {
  lbft_config c;
  memset(&c, 0, sizeof(c));
  c.num_nodes = 4; c.mean = 10.0; c.variance = 4.0; c.commands_per_epoch = 30000; c.target_commit_interval = 100000;
  c.delta = 20; c.gamma = 2.0; c.lambda = 0.5;
  const uint64_t seeds[3] = {1, 2, 3};
  uint32_t info[4];
  void* h = vtm_create(&c, seeds, 3, 1000, 1, info);
  if (!h) { printf("no batch\n"); return 2; }
  const u32 n = info[0], bins = 2;
  int bad = 0;
  for (int pass = 0; pass < 3; pass++) {
    u32 ref, len;
    if (pass == 1) { vtm_chain(h, 0, &ref, &len); vtm_log(h, 0, ref, 5, 1, 0); }
    if (pass == 2) { vtm_chain(h, 1, &ref, &len); vtm_log(h, 1, ref, 2, 1, 0xfffffff0u); }
    std::vector<u64> first;
    for (u32 W : {1u, 7u, 64u}) {
      std::vector<u64> out(bins + (n + 1) + n * VT_NODE_COLUMNS + LBFT_VOTE_STATS);
      u64 check[2];
      u64 *margin = out.data(), *votes = margin + bins, *nodes = votes + n + 1, *stats = nodes + n * VT_NODE_COLUMNS;
      if (vtm_walk(h, W, 1, bins, margin, votes, nodes, stats, check) != 0 || check[0] || check[1]) bad++;
      if (first.empty()) first = out; else if (first != out) bad++;
      u64 proposed = 0, orphaned = 0, voted = 0;
      for (u32 a = 0; a < n; a++) { proposed += nodes[a * 3]; orphaned += nodes[a * 3 + 1]; voted += nodes[a * 3 + 2]; }
      if (proposed != stats[4 * VT_BLOCKS + 1] || orphaned != stats[4 * VT_ORPHANED + 1] || voted != stats[4 * VT_VOTES + 1]) bad++;
      if (stats[4 * VT_BLOCKS] != 3 || stats[4 * VT_VOTES] < 20) bad++;
    }
  }
  vtm_destroy(h);
  printf("%s\n", bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
#endif
