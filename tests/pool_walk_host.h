// TEST INFRASTRUCTURE: what the host models of the pool-and-chain kernels share (vote_stats_host_model.cpp, epoch_stats_host_model.cpp,
// record_hashes_host_model.cpp), the counterpart of csrc/lbft_chain_walk.h name for name.  A plain batch run through the kernel logic on
// the host stays in a handle (PwModel); the accessors read and edit its state; the rules of the walk -- the node pass, the pool bound,
// the chunk head, the membership gather -- are stated once, with the chunk width W a parameter: a lane is an array element, a ballot a
// loop.  Every read of a block record goes through CwRec, which counts the reads whose id was not checked against the pool first: a walk
// must give 0.
#ifndef POOL_WALK_HOST_H
#define POOL_WALK_HOST_H

#include <thread>
#include <vector>

#include "../oracle/host_model_common.h"
#include "../librabft_simulator_amd/csrc/lbft_chain_rules.h"
#include "../librabft_simulator_amd/csrc/lbft_record_hash_rules.h"
#include "../librabft_simulator_amd/csrc/lbft_vote_rules.h"

using namespace lbft;

struct PwModel {
  TwinBatch tb;
  std::vector<u32> state;
  size_t m;
  int cls;
};

// Networks above 32 nodes: the planner's capacities for a run to max_clock without the calendar queue, stepped as the generic class.
static int setup_large(const lbft_config* base, size_t m, int64_t max_clock, TwinBatch& t) {
  lbft_config c = *base;
  c.queue_capacity = c.snapshot_capacity = c.block_capacity = c.log_capacity = 0;
  Params& p = t.p;
  if (fill_params(&c, m, p, t.weights) != LBFT_OK) return -1;
  p.weights = t.weights.data();
  bool relayout;
  std::string err;
  if (plan_layout(c, p, max_clock, 0, false, false, 0, ~0ull, PlanKnobs(), false, relayout, err) != LBFT_OK) return -1;
  attach_tables(p, c.delta, c.gamma, t.dur, t.leaders);
  p.ql = 0;
  set_tile_width(p, layout_tile_width(p));
  return K_GENERIC;
}

// A plain batch of `base` run to max_clock on `threads` threads; NULL on a bad argument (`large` = false: more than 32 nodes are one).
// info: num_nodes, log capacity, block capacity, kernel class.
static void* pw_create(const lbft_config* base, const uint64_t* seeds, size_t m, int64_t max_clock, uint32_t threads, uint32_t* info, bool large) {
  const u32 n = base->num_nodes;
  if (n == 0 || n > LBFT_MAX_NODES) return nullptr;
  PwModel* h = new PwModel;
  h->m = m;
  h->cls = n <= 32 || !large ? setup_twin_batch(base, nullptr, 0, (base->quirks & 1u) ? 0 : (16 * n < 64 ? 64 : 16 * n), m, max_clock, h->tb)
                             : setup_large(base, m, max_clock, h->tb);
  if (h->cls < 0) { delete h; return nullptr; }
  const Params& p = h->tb.p;
  h->state.assign(state_words(p), 0);
  if (threads == 0) threads = 1;
  auto worker = [&](u32 tid) {
    for (size_t i = tid; i < m; i += threads) {
      { Sim s0(p, h->state.data(), (u32)i); s0.init(seeds[i]); }
      if (h->cls == K_SMALL) { SimT<K_SMALL> s(p, h->state.data(), (u32)i); run_one(s, p, 0); }
      else if (h->cls == K_MID) { SimT<K_MID> s(p, h->state.data(), (u32)i); run_one(s, p, 0); }
      else { Sim s(p, h->state.data(), (u32)i); run_one(s, p, 0); }
    }
  };
  std::vector<std::thread> ts;
  for (u32 t = 1; t < threads; t++) ts.emplace_back(worker, t);
  worker(0);
  for (auto& t : ts) t.join();
  if (info) { info[0] = n; info[1] = p.lcap; info[2] = p.bcap; info[3] = (u32)h->cls; }
  return h;
}
static void pw_destroy(void* handle) { delete static_cast<PwModel*>(handle); }
static Sim pw_sim(void* handle, uint32_t inst) {
  PwModel* h = static_cast<PwModel*>(handle);
  return Sim(h->tb.p, h->state.data(), inst);
}

// commit_counts [m][n] (as stored, not clamped), faults [m], nblocks [m]; startup [m][n] and epochs [m][n] where not NULL
static void pw_counts(void* handle, uint32_t* commit_counts, uint32_t* faults, uint32_t* nblocks, int32_t* startup, uint32_t* epochs) {
  PwModel* h = static_cast<PwModel*>(handle);
  const u32 n = h->tb.p.n;
  for (size_t i = 0; i < h->m; i++) {
    Sim s = pw_sim(handle, (u32)i);
    faults[i] = s.ld(I_FAULT);
    nblocks[i] = s.ld(I_NBLOCKS);
    for (u32 q = 0; q < n; q++) {
      commit_counts[i * n + q] = s.nfm(q, NF_NCOMMITS);
      if (startup) startup[i * n + q] = (i32)s.nfm(q, NF_STARTUP);
      if (epochs) epochs[i * n + q] = s.nfm(q, NF_EPOCH);
    }
  }
}
// Entry k of a node's log: returns it, and stores `value` there when `set` is not 0
static uint32_t pw_log(void* handle, uint32_t inst, uint32_t node, uint32_t k, int set, uint32_t value) {
  const Params& p = static_cast<PwModel*>(handle)->tb.p;
  Sim s = pw_sim(handle, inst);
  const u32 w = p.off_log + node * p.lcap + k;
  const u32 old = s.ld(w);
  if (set) s.st(w, value);
  return old;
}
static void pw_set_fault(void* handle, uint32_t inst, uint32_t value) { pw_sim(handle, inst).st(I_FAULT, value); }
// A field of pool block b (1 .. block count; what: 0 epoch, 1 round, 2 author, 3 time, 4 ledger depth): returns it, and stores `value`
// there when `set` is not 0 (epoch, round and time only)
static uint32_t pw_block(void* handle, uint32_t inst, uint32_t b, uint32_t what, int set, uint32_t value) {
  Sim s = pw_sim(handle, inst);
  const u32 f = what == 0 ? (u32)B_EPOCH : what == 1 ? (u32)B_ROUND : what == 2 ? (u32)B_LINK : what == 3 ? (u32)B_TIME : (u32)B_DEPTH;
  const u32 old = s.bf(b, f);
  if (set && what != 2 && what != 4) s.bfs(b, f, value);
  return what == 2 ? old >> 16 : old;
}

// Node pass: nc_j = min(NF_NCOMMITS, lcap); the chain's length L and the reference node, the lowest-numbered longest log.
struct CwChain {
  u32 L, ref;
};
static CwChain cw_chain_of(const Sim& s, u32 n, u32 lcap) {
  u64 best = 0;
  for (u32 j = 0; j < n; j++) best = chn_ref_max(best, chn_ref_key(chn_commits(s.nfm(j, NF_NCOMMITS), lcap), j));
  return CwChain{chn_ref_len(best), chn_ref_node(best)};
}
static void pw_chain(void* handle, uint32_t inst, uint32_t* ref, uint32_t* length) {
  const Params& p = static_cast<PwModel*>(handle)->tb.p;
  const CwChain ch = cw_chain_of(pw_sim(handle, inst), p.n, p.lcap);
  *ref = ch.ref; *length = ch.L;
}

// Pool bound: the ids 1 .. nb are block records; nothing else is ever an address.  CwRec: field f of record b, counted when b is none.
static u32 cw_pool_blocks(const Sim& s, const Params& p) { return s.ld(I_NBLOCKS) < p.bcap ? s.ld(I_NBLOCKS) : p.bcap; }
struct CwRec {
  const Sim& s;
  u32 nb;
  u64& unchecked;
  u32 operator()(u32 b, u32 f) const {
    if (!rh_valid_id(b, nb)) { unchecked++; return 0; }
    return s.bf(b, f);
  }
};

// Chunk head of the chain pass: the ids y[sl] of the entries c0 + sl < L of the log row at `row` (0 beyond L).  The first id outside
// the pool ends the chain: jb = its lane (W: none), inblk = the entries the chunk has, nv = those before jb.  cw_ends: this chunk is the
// last, the chain has c0 + nv entries.
struct CwChunk {
  std::vector<u32> y;
  u32 inblk, jb, nv;
};
static CwChunk cw_chunk(const Sim& s, u32 row, u32 c0, u32 L, u32 nb, u32 W) {
  CwChunk c{std::vector<u32>(W, 0), L - c0 < W ? L - c0 : W, W, 0};
  for (u32 sl = 0; sl < W; sl++) {
    const u32 k = c0 + sl;
    c.y[sl] = k < L ? s.ld(row + k) : 0;
    if (k < L && !rh_valid_id(c.y[sl], nb) && c.jb == W) c.jb = sl;
  }
  c.nv = c.jb < c.inblk ? c.jb : c.inblk;
  return c;
}
static bool cw_ends(const CwChunk& c) { return c.nv < c.inblk; }

// Pool pass: is pool block b, of ledger depth `depth`, entry depth - 1 of the chain of L entries at `row`?  One guarded gather.
static bool cw_pool_member(const Sim& s, u32 row, u32 depth, u32 L, u32 b) {
  const u32 slot = vt_chain_slot(depth, L);
  const u32 at = slot < L ? s.ld(row + slot) : 0;
  return vt_member(slot, L, at, b);
}

extern "C" {

// The chunk head alone, for tests/test_pool_walk_host.py: the ids the walk of an instance yields in chunks of W lanes (1 .. 64), up to
// `cap` of them into ids, with one counted read of every yielded id's record -> their number; *unchecked = reads with an unchecked id.
uint32_t pw_chain_entries(void* handle, uint32_t inst, uint32_t W, uint32_t* ids, uint32_t cap, uint64_t* unchecked) {
  const Params& p = static_cast<PwModel*>(handle)->tb.p;
  Sim s = pw_sim(handle, inst);
  const CwChain ch = cw_chain_of(s, p.n, p.lcap);
  const u32 row = p.off_log + ch.ref * p.lcap, nb = cw_pool_blocks(s, p);
  *unchecked = 0;
  CwRec rec{s, nb, *unchecked};
  u32 L = ch.L;
  for (u32 c0 = 0; c0 < L; c0 += W) {
    const CwChunk c = cw_chunk(s, row, c0, L, nb, W);
    for (u32 sl = 0; sl < c.nv; sl++) {
      rec(c.y[sl], B_LINK);
      if (c0 + sl < cap) ids[c0 + sl] = c.y[sl];
    }
    if (cw_ends(c)) L = c0 + c.nv;
  }
  return L;
}
// Cuts an instance's chain to `length` entries: no node's commit count stays above it.
void pw_cut(void* handle, uint32_t inst, uint32_t length) {
  Sim s = pw_sim(handle, inst);
  for (u32 q = 0; q < static_cast<PwModel*>(handle)->tb.p.n; q++)
    if (s.nfm(q, NF_NCOMMITS) > length) s.nfms(q, NF_NCOMMITS, length);
}

}  // extern "C"

#endif  // POOL_WALK_HOST_H
