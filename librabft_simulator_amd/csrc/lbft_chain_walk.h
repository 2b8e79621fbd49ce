// lbft_chain_walk.h -- the walk over the committed chain of an instance, one wavefront per instance, that the per-entry kernels share
// (DESIGN.md "The chain walk"): lbft_k_ct_finality, lbft_k_ct_instances and lbft_k_ct_phases take all of it, lbft_k_cs_chain and
// lbft_k_rh_chain the node pass and the proposal time (the other rule headers come along unused, so that the walk has one file),
// lbft_k_ct_latency_hist the proposal time, lbft_k_ct_timeline the CtlRow exchange.  tests/chain_walk_host.h states the same rules for
// the host shims, name for name.  The __shared__ arrays and the loop over the instances stay with the kernels.
// (Included under `using namespace lbft`.)
#ifndef LBFT_CHAIN_WALK_H
#define LBFT_CHAIN_WALK_H

#include "lbft_core.h"
#include "lbft_chain_rules.h"
#include "lbft_commit_finality.h"
#include "lbft_commit_timeline.h"
#include "lbft_group_stats.h"

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

// The global proposal time of block b: its proposer's clock (B_TIME) on top of the proposer's startup time.
template <class S>
__device__ __forceinline__ i32 cw_proposal(const S& s, u32 b, u32 author) { return (i32)(s.nfm(author, NF_STARTUP) + s.bf(b, B_TIME)); }
template <class S>
__device__ __forceinline__ i32 cw_proposal(const S& s, u32 b) { return cw_proposal(s, b, s.blk_author(b)); }

// The walk's per-workgroup context.
#define CW_MAX_NODES 32  // (timed batches have at most 32 nodes: lbft_batch_record_commit_times)
struct CwWalk {
  u32 g, first, cnt;  // the workgroup's group: instances gs_instance(grp_inst, first, 0 .. cnt)
  u32 wave, lane;
  u32 n, lcap, lg;  // lg: the first word of the logs
  u32 cpe, rot, t_quorum, t_valid;  // the voting rights' rotation and the two thresholds
  const u32* rights;  // the rights table in LDS, NULL = every right is 1
  i32* col;  // this lane's column of the wavefront's [n][64] tile: node j at col[j * 64]
};
// false: the whole workgroup returns (its group has fewer instances).  The rights table's copy is read after the caller's next barrier.
template <u32 WAVES>
__device__ __forceinline__ bool cw_begin(CwWalk& w, const Params& p, const u32* grp_inst, const u32* grp_off, i32 (&tile)[WAVES][CW_MAX_NODES][64],
                                         u32 (&s_rights)[CW_MAX_NODES]) {
  w = CwWalk{};  // (a member left undefined on the idle path costs the kernels registers: 10 in lbft_k_ct_finality)
  w.g = blockIdx.y;
  const uint2 grp = gs_group(grp_inst, grp_off, w.g, p.m);
  w.first = grp.x; w.cnt = grp.y;
  if (blockIdx.x * WAVES >= w.cnt) return false;
  w.wave = threadIdx.x / 64; w.lane = threadIdx.x % 64;
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
