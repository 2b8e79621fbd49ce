// lbft_record_hashes.hip -- the HIP kernel (gfx950) of lbft_batch_chain_record_hashes: for every instance of a batch, the hashes the
// reference gives the records behind its committed chain -- the Block_ of every entry, the State after it, the QuorumCertificate_ over
// the Vote_s it carries -- computed from what every run leaves in HBM: the commit logs, the shared block pool and the fault words.
// Built as a library of its own (build.py), opened by liblbft_hip.so on first use: the code object of liblbft_hip.so, whose kernels are
// pinned byte for byte by the codegen manifest, does not change.
#include <hip/hip_runtime.h>

#include "../../include/lbft.h"
#include "lbft_core.h"
#include "lbft_chain_rules.h"
#include "lbft_record_hash_rules.h"
#include "lbft_record_hashes.h"

using namespace lbft;

#include "lbft_chain_walk.h"  // the node pass, the pool bound, the chunk head

// One segment of W = rh_width(n) lanes per instance, 64 / W instances per wavefront, LBFT_RH_BLOCK / 64 wavefronts per workgroup; no
// LDS, no atomics.  State is read through the generic Sim accessors (every layout).  The lanes of a segment run the same control flow;
// every shuffle and ballot is read inside the segment only.  Node pass and chunk head are lbft_chain_walk.h's, at the segment's width.
//   the chain in blocks of W entries (lane = entry k = c0 + lane): a lane whose id is one of the pool's loads the record's fields.  The
//     id that ends the walk is an entry of its own (nx = nv + 1), flagged RH_BAD_ID.
//     state step: lane k hashes (k + 1, entries 0 .. k); the entries (author, B_CMD, B_TIME) are gathered W at a time by the segment,
//       from the chain's start, and broadcast by __shfl.
//     chain step, entry by entry: the values of entry k come from lane k, the block hash is computed by every lane alike, the vote
//       hashes with lane = author, the QC stream by every lane alike with author a's vote hash from lane a.  The previous QC hash, the
//       two previous states and block ids are carried.  Lane k keeps entry k and stores it after the block: W x 32 contiguous bytes.
//     audit: the same W entries of every other node's row against the block's ids; the first difference below nc_j, by ballot.
#define LBFT_RH_BLOCK 256
#define LBFT_RH_NODE_ROUNDS ((LBFT_MAX_NODES + 63) / 64)
#define LBFT_RH_MASK_WORDS ((LBFT_MAX_NODES + 31) / 32)

__device__ __forceinline__ u64 rh_shfl64(u64 v, u32 src, u32 W) { return (u64)__shfl((unsigned long long)v, (int)src, (int)W); }
__device__ __forceinline__ u32 rh_shfl32(u32 v, u32 src, u32 W) { return (u32)__shfl((int)v, (int)src, (int)W); }

__global__ __launch_bounds__(LBFT_RH_BLOCK) void lbft_k_rh_chain(Params p, const u32* __restrict__ state, u32 first, u32 count, u32 W,
                                                                 lbft_record_hash* __restrict__ out, u32 cap, lbft_chain_head* __restrict__ heads,
                                                                 u32* __restrict__ node_prefix) {
  const u32 lane = threadIdx.x % 64, sl = lane & (W - 1u), seg0 = lane - sl;
  const u32 q = (blockIdx.x * LBFT_RH_BLOCK + threadIdx.x) / W;  // (uniform in the segment)
  if (q >= count) return;
  const u32 i = first + q;
  const u32 n = p.n, lcap = p.lcap, lg = p.off_log, mw = p.mw;
  const u64 segmask = W == 64 ? ~0ull : (1ull << W) - 1ull;
  Sim s(p, const_cast<u32*>(state), i);
  if (s.ld(I_FAULT) != 0) return;
  // node pass
  u32 nc[LBFT_RH_NODE_ROUNDS];
  const CwChain ch = cw_chain_of(s, sl, n, lcap, W, nc);
  const u32 L = ch.L, ref = ch.ref;
  const u32 nb = cw_pool_blocks(s, p);
  const u32 row = lg + ref * lcap;

  u64 qc_prev = 0, st_prev = 0, st_prev2 = 0;
  u32 y_prev = 0, y_prev2 = 0;
  u32 pfx[LBFT_RH_NODE_ROUNDS];
#pragma unroll
  for (u32 r = 0; r < LBFT_RH_NODE_ROUNDS; r++) pfx[r] = 0xffffffffu;
  u32 Lw = L;  // the entries the walk gives
  u64 last_bh = 0, last_state = 0, last_qh = 0;
  u32 last_votes = 0, last_flags = 0;
  for (u32 c0 = 0; c0 < L; c0 += W) {
    const u32 k = c0 + sl;
    const CwChunk ck = cw_chunk(s, row, c0, L, nb, sl, W, seg0);
    const u32 y = ck.y, jb = ck.jb, nv = ck.nv;
    const bool ok = ck.have && rh_valid_id(y, nb);
    const u32 nx = cw_ends(ck) ? nv + 1 : nv;  // the block's entries with the bad id that ends the walk
    u32 link = 0, round = 0, prev_round = 0, pp = 0, pp_round = 0, epoch = 0, cmd = 0, tm = 0;
    u32 vw[LBFT_RH_MASK_WORDS] = {};
    if (ok) {
      link = s.bf(y, B_LINK); round = s.bf(y, B_ROUND); prev_round = s.bf(y, B_PREV_ROUND); pp = s.bf(y, B_PP) & 0xffffu;
      pp_round = s.bf(y, B_PP_ROUND); epoch = s.bf(y, B_EPOCH); cmd = s.bf(y, B_CMD); tm = s.bf(y, B_TIME);
#pragma unroll
      for (u32 w = 0; w < LBFT_RH_MASK_WORDS; w++)
        if (w < mw) vw[w] = s.bf(y, rh_voter_field(w, mw)) & rh_author_bits(w, n);
    }
    // audit
    if (node_prefix) {
#pragma unroll
      for (u32 r = 0; r < LBFT_RH_NODE_ROUNDS; r++) {
        const u32 left = n > r * 64 ? n - r * 64 : 0, nj = left < 64 ? left : 64;
        for (u32 jj = 0; jj < nj; jj++) {
          const u32 j = r * 64 + jj;
          if (j == ref) continue;
          const u32 ncj = rh_shfl32(nc[r], jj, W);
          const u32 other = sl < nx ? s.ld(lg + j * lcap + k) : y;  // (k < L <= lcap: inside the row)
          const u64 diff = (__ballot(sl < nx && k < ncj && other != y) >> seg0) & segmask;
          if (diff && sl == (jj & (W - 1u))) { const u32 at = c0 + (u32)__builtin_ctzll(diff); pfx[r] = at < pfx[r] ? at : pfx[r]; }
        }
      }
    }
    // state step
    Sip13 hs = rh_state_begin(k + 1);
    const u32 upto = c0 + nv;
    for (u32 g0 = 0; g0 < upto; g0 += W) {
      const u32 kk = g0 + sl;
      u32 a = 0, c = 0, t = 0;
      if (kk < upto) {
        const u32 b = s.ld(row + kk);
        if (rh_valid_id(b, nb)) { a = s.blk_author(b); c = s.bf(b, B_CMD); t = s.bf(b, B_TIME); }
      }
      const u32 cnt = upto - g0 < W ? upto - g0 : W;
      for (u32 jj = 0; jj < cnt; jj++) {
        const u32 aj = rh_shfl32(a, jj, W), cj = rh_shfl32(c, jj, W), tj = rh_shfl32(t, jj, W);
        if (g0 + jj <= k) rh_state_entry(hs, aj, cj, tj);
      }
    }
    const u64 state_k = hs.finish();
    // chain step
    u64 my_bh = 0, my_state = 0, my_qh = 0;
    u32 my_votes = 0, my_flags = 0;
    for (u32 j = 0; j < nv; j++) {
      const u32 yj = rh_shfl32(y, j, W), linkj = rh_shfl32(link, j, W), roundj = rh_shfl32(round, j, W), prj = rh_shfl32(prev_round, j, W);
      const u32 ppj = rh_shfl32(pp, j, W), pprj = rh_shfl32(pp_round, j, W), epochj = rh_shfl32(epoch, j, W);
      const u32 cmdj = rh_shfl32(cmd, j, W), tmj = rh_shfl32(tm, j, W);
      const u64 statej = rh_shfl64(state_k, j, W);
      const u32 prev = linkj & 0xffffu, author = linkj >> 16;
      u32 flags = 0;
      if (prev && prev != y_prev) flags |= RH_INCONSISTENT;
      const u64 prev_qc_hash = prev ? qc_prev : rh_epoch_id(epochj);
      const u64 bh = rh_block(author, cmdj, tmj, prev_qc_hash, roundj, author);
      const bool has_cs = rh_has_cs(prev, ppj, roundj, prj, pprj);
      if (has_cs && ppj != y_prev2) flags |= RH_INCONSISTENT;
      const u64 cs = has_cs ? st_prev2 : 0;
      u32 vj[LBFT_RH_MASK_WORDS], votes = 0;
#pragma unroll
      for (u32 w = 0; w < LBFT_RH_MASK_WORDS; w++) {
        vj[w] = w < mw ? rh_shfl32(vw[w], j, W) : 0;
        votes += (u32)__popc(vj[w]);
      }
      const RhStream vs = rh_vote_begin(epochj, roundj, bh, statej, has_cs, cs);
      u64 vh[LBFT_RH_NODE_ROUNDS];
#pragma unroll
      for (u32 r = 0; r < LBFT_RH_NODE_ROUNDS; r++) vh[r] = r * 64 < n ? rh_vote_end(vs, r * 64 + sl) : 0;
      RhStream qs = rh_qc_begin(epochj, roundj, bh, statej, has_cs, cs, votes);
#pragma unroll
      for (u32 w = 0; w < LBFT_RH_MASK_WORDS; w++)
        for (u32 m = vj[w]; m; m &= m - 1u) {  // (uniform in the segment)
          const u32 a = 32 * w + (u32)ctz32(m);
          rh_qc_vote(qs, a, rh_shfl64(vh[w / 2], a & 63u, W));
        }
      u64 qh = rh_qc_end(qs, author);
      if (!votes) { flags |= RH_NO_QC; qh = 0; }
      if (sl == j) { my_bh = bh; my_state = statej; my_qh = qh; my_votes = votes; my_flags = flags; }
      last_bh = bh; last_state = statej; last_qh = qh; last_votes = votes; last_flags = flags;
      y_prev2 = y_prev; y_prev = yj; st_prev2 = st_prev; st_prev = statej; qc_prev = qh;
    }
    if (nx > nv) {  // the id at c0 + jb is none of the pool's: the walk ends with this entry
      if (sl == jb) { my_bh = my_state = my_qh = 0; my_votes = 0; my_flags = RH_BAD_ID; }
      last_bh = last_state = last_qh = 0; last_votes = 0; last_flags = RH_BAD_ID;
      Lw = c0 + nx;
    }
    if (out && sl < nx && k < cap) out[(size_t)q * cap + k] = lbft_record_hash{my_bh, my_state, my_qh, my_votes, my_flags};
    if (nx > nv) break;
  }
  if (node_prefix) {
#pragma unroll
    for (u32 r = 0; r < LBFT_RH_NODE_ROUNDS; r++) {
      const u32 j = r * 64 + sl;
      if (j < n) {
        u32 v = nc[r] < Lw ? nc[r] : Lw;
        v = pfx[r] < v ? pfx[r] : v;
        node_prefix[(size_t)i * n + j] = v;
      }
    }
  }
  if (sl == 0 && L) heads[i] = lbft_chain_head{last_bh, last_state, last_qh, Lw, ref, last_votes, last_flags};
}

extern "C" {

__attribute__((visibility("default"))) hipError_t lbft_rh_launch_chain(const Params* p, const u32* state, u32 first, u32 count, lbft_record_hash* out,
                                                                      u32 cap, lbft_chain_head* heads, u32* node_prefix, hipStream_t stream) {
  if (!p || !state || !heads || count == 0 || p->n == 0 || p->n > LBFT_MAX_NODES || (u64)first + count > p->m || (out && cap == 0))
    return hipErrorInvalidValue;
  const u32 W = rh_width(p->n), per_block = LBFT_RH_BLOCK / W;
  lbft_k_rh_chain<<<(count + per_block - 1) / per_block, LBFT_RH_BLOCK, 0, stream>>>(*p, state, first, count, W, out, cap, heads, node_prefix);
  return hipGetLastError();
}

}  // extern "C"
