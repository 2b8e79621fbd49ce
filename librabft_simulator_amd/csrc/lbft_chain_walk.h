// lbft_chain_walk.h -- the walk over the committed chain of an instance, one wavefront per instance, that the per-entry kernels share
// (DESIGN.md "The chain walk"): lbft_k_ct_finality, lbft_k_ct_instances and lbft_k_ct_phases take the node pass, the tile and the origin
// of a latency sample, lbft_k_ct_latency_hist the proposal time, lbft_k_ct_timeline the CtlRow exchange; the pool-and-chain kernels
// lbft_k_cs_chain, lbft_k_rh_chain, lbft_k_ps_votes and lbft_k_ps_epochs take the workgroup prologue, the node pass, the pool bound, the
// chunk head, the predecessor by shuffle and the membership gather (the rule headers come along whole, so that the walk has one file;
// lbft_vote_rules.h alone stays with liblbft_paramsets.so, whose kernels include it first and get cw_pool_member).
// tests/chain_walk_host.h and tests/pool_walk_host.h state the same rules for the host tier, name for name.  The __shared__ arrays, the
// pass loop and the loop over the instances stay with the kernels.
// (Included under `using namespace lbft`.)
#ifndef LBFT_CHAIN_WALK_H
#define LBFT_CHAIN_WALK_H

#include "lbft_core.h"
#include "lbft_chain_rules.h"
#include "lbft_commit_finality.h"
#include "lbft_commit_timeline.h"
#include "lbft_group_stats.h"
#include "lbft_record_hash_rules.h"  // rh_valid_id

// The workgroup of a grouped kernel: group g = blockIdx.y holds the instances gs_instance(grp_inst, first, 0 .. cnt), over which the
// WAVES wavefronts of its workgroups stride.  false: the whole workgroup returns (its group has fewer instances).
struct CwGroup {
  u32 g, first, cnt;
  u32 wave, lane;
};
template <u32 WAVES>
__device__ __forceinline__ bool cw_group_begin(CwGroup& w, const Params& p, const u32* grp_inst, const u32* grp_off) {
  w = CwGroup{};  // (a member left undefined on the idle path costs the kernels registers: 10 in lbft_k_ct_finality)
  w.g = blockIdx.y;
  const uint2 grp = gs_group(grp_inst, grp_off, w.g, p.m);
  w.first = grp.x; w.cnt = grp.y;
  if (blockIdx.x * WAVES >= w.cnt) return false;
  w.wave = threadIdx.x / 64; w.lane = threadIdx.x % 64;
  return true;
}

// Node pass.  Lane sl's node in round r is r * 64 + sl; nc[r] = its cw_commits.  A butterfly over the keys (nc_j, ~j) of a segment of
// `width` lanes (a power of two <= 64) gives the chain's length L (<= lcap) and the reference node: the lowest-numbered longest log.
template <class S>
__device__ __forceinline__ u32 cw_commits(const S& s, u32 j, u32 n, u32 lcap) { return j < n ? chn_commits(s.nfm(j, NF_NCOMMITS), lcap) : 0; }
struct CwChain {
  u32 L, ref;
};
template <u32 ROUNDS>
__device__ __forceinline__ CwChain cw_node_pass(const u32* nc, u32 sl, u32 n, u32 width) {
  u64 best = 0;
#pragma unroll
  for (u32 r = 0; r < ROUNDS; r++)
    if (r * 64 + sl < n) best = chn_ref_max(best, chn_ref_key(nc[r], r * 64 + sl));
  for (u32 d = width >> 1; d; d >>= 1) best = chn_ref_max(best, (u64)__shfl_xor((unsigned long long)best, (int)d, (int)width));
  return CwChain{chn_ref_len(best), chn_ref_node(best)};
}
// Both steps for the lane sl of a segment: fills nc[] (the callers keep it: the lag, the audit) and gives L <= lcap and ref < n.
template <u32 ROUNDS, class S>
__device__ __forceinline__ CwChain cw_chain_of(const S& s, u32 sl, u32 n, u32 lcap, u32 width, u32 (&nc)[ROUNDS]) {
#pragma unroll
  for (u32 r = 0; r < ROUNDS; r++) nc[r] = cw_commits(s, r * 64 + sl, n, lcap);
  return cw_node_pass<ROUNDS>(nc, sl, n, width);
}

// Pool bound: the ids 1 .. nb are block records; nothing else is ever an address.
template <class S>
__device__ __forceinline__ u32 cw_pool_blocks(const S& s, const Params& p) { return s.ld(I_NBLOCKS) < p.bcap ? s.ld(I_NBLOCKS) : p.bcap; }

// Chunk head of the chain pass.  Lane sl of a segment of W lanes that begins at lane seg0 of the wavefront (the whole wavefront: W = 64,
// seg0 = 0) has entry k = c0 + sl of the log row at `row` when k < L (have; k < L <= lcap: inside the row) and loads its id y.  The ids
// are checked (rh_valid_id) before any record is read, by the callers too.  The first id outside the pool ends the chain: jb = its lane
// by ballot (W: none), inblk = the entries the chunk has, nv = those before jb.  cw_ends: this chunk is the last, the chain has c0 + nv
// entries (and the bad id lies at c0 + nv).
struct CwChunk {
  u32 y;
  bool have;
  u32 inblk, jb, nv;
};
template <class S>
__device__ __forceinline__ CwChunk cw_chunk(const S& s, u32 row, u32 c0, u32 L, u32 nb, u32 sl, u32 W, u32 seg0) {
  CwChunk c;
  const u32 k = c0 + sl;
  c.have = k < L;
  c.y = c.have ? s.ld(row + k) : 0;
  const u64 segmask = W == 64 ? ~0ull : (1ull << W) - 1ull;
  const u64 bad = (__ballot(c.have && !rh_valid_id(c.y, nb)) >> seg0) & segmask;
  c.inblk = L - c0 < W ? L - c0 : W;
  c.jb = bad ? (u32)__builtin_ctzll(bad) : W;
  c.nv = c.jb < c.inblk ? c.jb : c.inblk;
  return c;
}
__device__ __forceinline__ bool cw_ends(const CwChunk& c) { return c.nv < c.inblk; }

// Predecessor by shuffle: the value of the lane below, lane 0 takes what the previous chunk carried; the carry becomes lane 63's (of a
// chunk that is not full: the last one, nothing reads it).  cw_tip: the value of the chunk's last entry, lane nv - 1 (nv > 0).
__device__ __forceinline__ u32 cw_prev(u32 v, u32& carry, u32 lane) {
  u32 pv = (u32)__shfl_up((int)v, 1, 64);
  if (lane == 0) pv = carry;
  carry = (u32)__shfl((int)v, 63, 64);
  return pv;
}
__device__ __forceinline__ i32 cw_prev(i32 v, i32& carry, u32 lane) {
  i32 pv = __shfl_up(v, 1, 64);
  if (lane == 0) pv = carry;
  carry = __shfl(v, 63, 64);
  return pv;
}
__device__ __forceinline__ u32 cw_tip(u32 v, u32 nv) { return (u32)__shfl((int)v, (int)nv - 1, 64); }

// Pool pass: is pool block b, of ledger depth `depth`, entry depth - 1 of the chain of L entries at `row`?  One dependent gather, guarded
// (slot < L <= lcap: inside the row).  cw_ballot_count: the lanes of the wavefront for which v holds.
#ifdef LBFT_VOTE_RULES_H  // (vt_chain_slot, vt_member: the header is liblbft_paramsets.so's alone, whose kernels include it before this one)
template <class S>
__device__ __forceinline__ bool cw_pool_member(const S& s, u32 row, u32 depth, u32 L, u32 b) {
  const u32 slot = vt_chain_slot(depth, L);
  const u32 at = slot < L ? s.ld(row + slot) : 0;
  return vt_member(slot, L, at, b);
}
#endif
__device__ __forceinline__ u32 cw_ballot_count(bool v) { return (u32)__popcll(__ballot(v)); }

// The global proposal time of block b: its proposer's clock (B_TIME) on top of the proposer's startup time.
template <class S>
__device__ __forceinline__ i32 cw_proposal(const S& s, u32 b, u32 author) { return (i32)(s.nfm(author, NF_STARTUP) + s.bf(b, B_TIME)); }
template <class S>
__device__ __forceinline__ i32 cw_proposal(const S& s, u32 b) { return cw_proposal(s, b, s.blk_author(b)); }

// The per-workgroup context of the commit-time kernels' walk: the group (CwGroup) and what their entries need.
#define CW_MAX_NODES 32  // (timed batches have at most 32 nodes: lbft_batch_record_commit_times)
struct CwWalk : CwGroup {
  u32 n, lcap, lg;  // lg: the first word of the logs
  u32 cpe, rot, t_quorum, t_valid;  // the voting rights' rotation and the two thresholds
  const u32* rights;  // the rights table in LDS, NULL = every right is 1
  i32* col;  // this lane's column of the wavefront's [n][64] tile: node j at col[j * 64]
};
// false: the whole workgroup returns (its group has fewer instances).  The rights table's copy is read after the caller's next barrier.
template <u32 WAVES>
__device__ __forceinline__ bool cw_begin(CwWalk& w, const Params& p, const u32* grp_inst, const u32* grp_off, i32 (&tile)[WAVES][CW_MAX_NODES][64],
                                         u32 (&s_rights)[CW_MAX_NODES]) {
  w = CwWalk{};  // (zero first, as in cw_group_begin)
  if (!cw_group_begin<WAVES>(w, p, grp_inst, grp_off)) return false;
  w.n = p.n; w.lcap = p.lcap; w.lg = p.off_log;
  w.cpe = fin_cpe32(p.cpe); w.rot = p.rot;
  w.t_quorum = p.quorum; w.t_valid = fin_valid_threshold(p.total_votes, p.quorum);
  w.rights = p.unit_weights ? nullptr : s_rights;
  w.col = &tile[w.wave][0][w.lane];
  if (threadIdx.x < w.n) s_rights[threadIdx.x] = p.weights[threadIdx.x];
  return true;
}

// Row j of the chunk into the tile: lane k's entry of node j, FIN_NONE where node j is no committer of entry k, goes into the lane's
// column; nc = the lane's own count from the node pass (lane = node).  A lane reads only the LDS words it wrote itself: no barrier.
struct CwStaged {
  i32 c;          // the entry as staged
  const i32* ct;  // ctimes[i][j]
  u32 commits;    // nc_j
};
__device__ __forceinline__ CwStaged cw_stage(const CwWalk& w, const i32* __restrict__ ctimes, u32 i, u32 nc, u32 j, u32 k) {
  CwStaged e;
  e.commits = (u32)__shfl((int)nc, (int)j, 64);
  e.ct = ctimes + ((size_t)i * w.n + j) * w.lcap;
  e.c = k < e.commits ? e.ct[k] : FIN_NONE;  // (k < nc_j <= lcap: inside the row)
  e.c = fin_committer(k, e.commits, e.c) ? e.c : FIN_NONE;
  w.col[j * 64] = e.c;
  return e;
}
// The column of entry k, once its n rows are staged.
__device__ __forceinline__ FinEntry cw_column(const CwWalk& w, u32 k) {
  return fin_entry(w.col, 64u, w.n, w.rights, fin_rights_shift(k, w.cpe, w.rot, w.n), w.t_valid, w.t_quorum);
}

// The origin of a latency sample: node j committed entry k (then k < nc_j <= L: b and g are the chain's b_k and g_k) and counts from the
// proposal time of the block in its OWN log.
template <class S>
__device__ __forceinline__ i32 cw_own_proposal(const S& s, const CwWalk& w, u32 j, u32 k, u32 b, i32 g) {
  const u32 bj = s.ld(w.lg + j * w.lcap + k);
  return bj != b ? cw_proposal(s, bj) : g;
}

// One step of the CtlRow butterfly over a segment of WIDTH lanes: the lane's piece merged with that of lane ^ d.  The caller loops
// for (d = WIDTH / 2; d; d >>= 1): with the loop in here the timeline kernel takes two more vector registers.
template <int WIDTH>
__device__ __forceinline__ CtlRow ctl_merge_step(const CtlRow& r, int d) {
  CtlRow o;
  o.longest = (u32)__shfl_xor((int)r.longest, d, WIDTH);
  o.last = __shfl_xor(r.last, d, WIDTH);
  o.first = (u32)__shfl_xor((int)r.first, d, WIDTH);
  return ctl_merge(r, o);
}

#endif  // LBFT_CHAIN_WALK_H
