// record_hashes_host_model.cpp -- TEST INFRASTRUCTURE (tests/test_record_hashes_host_model.py compiles it with g++): plain batches of at
// most 32 nodes run through the kernel logic on the host (oracle/host_model_common.h), then every instance's committed chain walked the
// way lbft_k_rh_chain (csrc/lbft_record_hashes.hip) walks it -- a segment of W lanes, the chain in blocks of W entries, the same steps
// in the same order with csrc/lbft_record_hash_rules.h -- with W a parameter: a lane is an array element, a shuffle an index, a ballot a
// loop.  (The kernel takes W >= n, up to two rounds of 64; here nodes and authors take as many rounds of W as they need, so any power of
// two walks any network.)  The model, its accessors and the shared steps of the walk are tests/pool_walk_host.h's; every read of a block
// record goes through its counted reader: the walk must give 0.  The state stays in the handle, so a test can edit log entries and fault
// words and walk again.
// With -DRHM_MAIN the file is a program of its own (for a run under the address and undefined-behaviour sanitizers).
#include "pool_walk_host.h"

// One instance, as one segment of the kernel.  -> reads of block records with an unchecked id
static u64 walk_instance(const Params& p, u32* state, u32 i, u32 W, lbft_record_hash* out, size_t cap, lbft_chain_head* head, u32* node_prefix) {
  const u32 n = p.n, lcap = p.lcap, lg = p.off_log, mw = p.mw;
  Sim s(p, state, i);
  if (s.ld(I_FAULT) != 0) return 0;
  u64 unchecked = 0;
  const u32 rounds = (n + W - 1) / W;
  // node pass
  std::vector<u32> nc(n, 0);
  for (u32 j = 0; j < n; j++) nc[j] = chn_commits(s.nfm(j, NF_NCOMMITS), lcap);
  const CwChain ch = cw_chain_of(s, n, lcap);
  const u32 L = ch.L, ref = ch.ref, nb = cw_pool_blocks(s, p), row = lg + ref * lcap;
  const CwRec rec{s, nb, unchecked};
  u64 qc_prev = 0, st_prev = 0, st_prev2 = 0;
  u32 y_prev = 0, y_prev2 = 0;
  std::vector<u32> pfx(n, 0xffffffffu);
  u32 Lw = L;
  lbft_record_hash last = {};
  struct Lane { u32 y, link, round, prev_round, pp, pp_round, epoch, cmd, tm, vw[LBFT_MAX_NODES / 32]; bool ok; u64 state; lbft_record_hash mine; };
  for (u32 c0 = 0; c0 < L; c0 += W) {
    std::vector<Lane> ln(W, Lane{});
    const CwChunk ck = cw_chunk(s, row, c0, L, nb, W);
    const u32 jb = ck.jb, nv = ck.nv, nx = cw_ends(ck) ? nv + 1 : nv;
    for (u32 sl = 0; sl < W; sl++) {
      ln[sl].y = ck.y[sl];
      ln[sl].ok = c0 + sl < L && rh_valid_id(ck.y[sl], nb);
    }
    for (u32 sl = 0; sl < W; sl++) {
      Lane& l = ln[sl];
      if (!l.ok) continue;
      l.link = rec(l.y, B_LINK); l.round = rec(l.y, B_ROUND); l.prev_round = rec(l.y, B_PREV_ROUND); l.pp = rec(l.y, B_PP) & 0xffffu;
      l.pp_round = rec(l.y, B_PP_ROUND); l.epoch = rec(l.y, B_EPOCH); l.cmd = rec(l.y, B_CMD); l.tm = rec(l.y, B_TIME);
      for (u32 w = 0; w < mw; w++) l.vw[w] = rec(l.y, rh_voter_field(w, mw)) & rh_author_bits(w, n);
    }
    // audit
    if (node_prefix)
      for (u32 j = 0; j < n; j++) {
        if (j == ref) continue;
        u64 diff = 0;
        for (u32 sl = 0; sl < nx; sl++) {
          const u32 k = c0 + sl;
          const u32 other = s.ld(lg + j * lcap + k);
          if (k < nc[j] && other != ln[sl].y) diff |= 1ull << sl;
        }
        if (diff) { const u32 at = c0 + (u32)__builtin_ctzll(diff); pfx[j] = at < pfx[j] ? at : pfx[j]; }
      }
    // state step
    const u32 upto = c0 + nv;
    std::vector<Sip13> hs(W);
    for (u32 sl = 0; sl < W; sl++) hs[sl] = rh_state_begin(c0 + sl + 1);
    for (u32 g0 = 0; g0 < upto; g0 += W) {
      std::vector<u32> a(W, 0), c(W, 0), t(W, 0);
      for (u32 sl = 0; sl < W; sl++) {
        const u32 kk = g0 + sl;
        if (kk >= upto) continue;
        const u32 b = s.ld(row + kk);
        if (rh_valid_id(b, nb)) { a[sl] = rec(b, B_LINK) >> 16; c[sl] = rec(b, B_CMD); t[sl] = rec(b, B_TIME); }
      }
      const u32 cnt = upto - g0 < W ? upto - g0 : W;
      for (u32 jj = 0; jj < cnt; jj++)
        for (u32 sl = 0; sl < W; sl++)
          if (g0 + jj <= c0 + sl) rh_state_entry(hs[sl], a[jj], c[jj], t[jj]);
    }
    for (u32 sl = 0; sl < W; sl++) ln[sl].state = hs[sl].finish();
    // chain step
    for (u32 j = 0; j < nv; j++) {
      const Lane& e = ln[j];
      const u32 prev = e.link & 0xffffu, author = e.link >> 16;
      u32 flags = 0;
      if (prev && prev != y_prev) flags |= RH_INCONSISTENT;
      const u64 prev_qc_hash = prev ? qc_prev : rh_epoch_id(e.epoch);
      const u64 bh = rh_block(author, e.cmd, e.tm, prev_qc_hash, e.round, author);
      const bool has_cs = rh_has_cs(prev, e.pp, e.round, e.prev_round, e.pp_round);
      if (has_cs && e.pp != y_prev2) flags |= RH_INCONSISTENT;
      const u64 cs = has_cs ? st_prev2 : 0;
      u32 votes = 0;
      for (u32 w = 0; w < mw; w++) votes += (u32)__builtin_popcount(e.vw[w]);
      const RhStream vs = rh_vote_begin(e.epoch, e.round, bh, e.state, has_cs, cs);
      std::vector<u64> vh((size_t)rounds * W);  // lane = author, a round of W at a time
      for (u32 r = 0; r < rounds; r++)
        for (u32 sl = 0; sl < W; sl++) vh[(size_t)r * W + sl] = rh_vote_end(vs, r * W + sl);
      RhStream qs = rh_qc_begin(e.epoch, e.round, bh, e.state, has_cs, cs, votes);
      for (u32 w = 0; w < mw; w++)
        for (u32 m = e.vw[w]; m; m &= m - 1u) {
          const u32 a = 32 * w + (u32)ctz32(m);
          rh_qc_vote(qs, a, vh[a]);
        }
      u64 qh = rh_qc_end(qs, author);
      if (!votes) { flags |= RH_NO_QC; qh = 0; }
      last = lbft_record_hash{bh, e.state, qh, votes, flags};
      ln[j].mine = last;
      y_prev2 = y_prev; y_prev = e.y; st_prev2 = st_prev; st_prev = e.state; qc_prev = qh;
    }
    if (nx > nv) {
      last = lbft_record_hash{0, 0, 0, 0, RH_BAD_ID};
      ln[jb].mine = last;
      Lw = c0 + nx;
    }
    for (u32 sl = 0; sl < nx; sl++)
      if (out && c0 + sl < cap) out[c0 + sl] = ln[sl].mine;
    if (nx > nv) break;
  }
  if (node_prefix)
    for (u32 j = 0; j < n; j++) {
      u32 v = nc[j] < Lw ? nc[j] : Lw;
      node_prefix[j] = pfx[j] < v ? pfx[j] : v;
    }
  if (L) *head = lbft_chain_head{last.block_hash, last.state, last.qc_hash, Lw, ref, last.num_votes, last.flags};
  return unchecked;
}

extern "C" {

void* rhm_create(const lbft_config* base, const uint64_t* seeds, size_t m, int64_t max_clock, uint32_t threads, uint32_t* info) { return pw_create(base, seeds, m, max_clock, threads, info, false); }
void rhm_destroy(void* handle) { pw_destroy(handle); }
void rhm_counts(void* handle, uint32_t* commit_counts, uint32_t* faults, uint32_t* nblocks) { pw_counts(handle, commit_counts, faults, nblocks, nullptr, nullptr); }
uint32_t rhm_log(void* handle, uint32_t inst, uint32_t node, uint32_t k, int set, uint32_t value) { return pw_log(handle, inst, node, k, set, value); }
void rhm_set_fault(void* handle, uint32_t inst, uint32_t value) { pw_set_fault(handle, inst, value); }

// Every instance walked with segments of W lanes (a power of two, 1 .. 64): out [m][cap] (may be NULL), heads [m], node_prefix [m][n]
// (may be NULL), all zeroed here first.  -> the number of block-record reads with an unchecked id (0 is right), < 0 on a bad argument
int64_t rhm_walk(void* handle, uint32_t W, lbft_record_hash* out, size_t cap, lbft_chain_head* heads, uint32_t* node_prefix) {
  PwModel* h = static_cast<PwModel*>(handle);
  if (!h || !heads || W == 0 || W > 64 || (W & (W - 1)) || (out && cap == 0)) return -1;
  const Params& p = h->tb.p;
  u64 unchecked = 0;
  for (size_t i = 0; i < h->m; i++) {
    heads[i] = lbft_chain_head{};
    for (size_t k = 0; out && k < cap; k++) out[i * cap + k] = lbft_record_hash{};
    for (u32 q = 0; node_prefix && q < p.n; q++) node_prefix[i * p.n + q] = 0;
    unchecked += walk_instance(p, h->state.data(), (u32)i, W, out ? out + i * cap : nullptr, cap, &heads[i], node_prefix ? node_prefix + i * p.n : nullptr);
  }
  return (int64_t)unchecked;
}

// SimT::committed_record_hashes of one node (what lbft_batch_committed_record_hashes runs) -> its commit count
uint32_t rhm_node(void* handle, uint32_t inst, uint32_t node, lbft_record_hash* out, uint32_t cap) {
  Sim s = pw_sim(handle, inst);
  std::vector<u64> raw((size_t)4 * (cap ? cap : 1));
  const u32 nc = s.committed_record_hashes(node, raw.data(), cap);
  for (u32 k = 0; k < nc && k < cap; k++)
    out[k] = lbft_record_hash{raw[4 * k], raw[4 * k + 1], raw[4 * k + 2], (uint32_t)raw[4 * k + 3], (uint32_t)(raw[4 * k + 3] >> 32)};
  return nc;
}

}  // extern "C"

#ifdef RHM_MAIN
#include <stdio.h>
#include <string.h>

// 4 nodes to clock 1000: every W against every node's own hashes, then a log entry of 0 and one above the pool
int main() {
  lbft_config c;
  memset(&c, 0, sizeof(c));
  c.num_nodes = 4; c.mean = 10.0; c.variance = 4.0; c.commands_per_epoch = 30000; c.target_commit_interval = 100000;
  c.delta = 20; c.gamma = 2.0; c.lambda = 0.5;
  const uint64_t seeds[3] = {52, 7, 1234567};
  uint32_t info[4];
  void* h = rhm_create(&c, seeds, 3, 1000, 1, info);
  if (!h) { printf("no batch\n"); return 2; }
  const u32 n = info[0], lcap = info[1];
  std::vector<lbft_record_hash> out((size_t)3 * lcap), mine(lcap);
  std::vector<lbft_chain_head> heads(3);
  std::vector<u32> prefix(3 * n);
  int bad = 0;
  for (int pass = 0; pass < 3; pass++) {
    if (pass == 1) rhm_log(h, 0, heads[0].ref_node, 5, 1, 0);
    if (pass == 2) rhm_log(h, 1, heads[1].ref_node, 2, 1, 0xfffffff0u);
    for (u32 W : {4u, 8u, 64u}) {
      if (rhm_walk(h, W, out.data(), lcap, heads.data(), prefix.data()) != 0) bad++;
      for (u32 i = 0; i < 3; i++) {
        if ((pass >= 1 && i == 0) || (pass == 2 && i == 1)) {
          const u32 at = i == 0 ? 5 : 2;
          if (heads[i].length != at + 1 || heads[i].flags != RH_BAD_ID || out[(size_t)i * lcap + at].flags != RH_BAD_ID) bad++;
          continue;
        }
        for (u32 q = 0; q < n; q++) {
          const u32 nc = rhm_node(h, i, q, mine.data(), lcap);
          if (prefix[i * n + q] != nc || nc > heads[i].length || (nc && memcmp(mine.data(), &out[(size_t)i * lcap], nc * sizeof(lbft_record_hash)))) bad++;
        }
        if (heads[i].length < 20) bad++;
      }
    }
  }
  rhm_destroy(h);
  printf("%s\n", bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
#endif
