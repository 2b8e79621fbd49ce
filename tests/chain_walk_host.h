// TEST INFRASTRUCTURE: the host shims' counterpart of csrc/lbft_chain_walk.h, name for name: the reference node, an entry's proposal
// time, which node is a committer of entry k, which block gives a latency sample its origin.  The state comes as the device holds it --
// ctimes[instance][node][lcap] (-1 = not recorded), logs[instance][node][lcap] of block ids (1-based), commits[instance][node] (not yet
// clamped), the block pool as blk_author / blk_time[instance][blocks + 1] (index = block id), startup[instance][node].  The chain is
// walked `chunk` entries side by side (the kernel: the 64 lanes of a wavefront), the n rows of a chunk staged as an [n][chunk] tile, lane
// l then taking its column &tile[l] with stride chunk.  Plain loops in place of the wavefront; chunk = 1 is a plain walk.
#ifndef CHAIN_WALK_HOST_H
#define CHAIN_WALK_HOST_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../librabft_simulator_amd/csrc/lbft_chain_rules.h"
#include "../librabft_simulator_amd/csrc/lbft_commit_finality.h"

// Instance i of the arrays every shim takes, in their common order (ctimes = NULL where a shim has none).
struct CwInstance {
  const int32_t* ctimes;    // [n][lcap]
  const uint32_t* logs;     // [n][lcap]
  const uint32_t* commits;  // [n]
  const uint32_t* author;   // [blocks + 1]
  const int32_t* time;      // [blocks + 1]
  const int32_t* startup;   // [n]
  uint32_t n, lcap, blocks;
};
inline CwInstance cw_instance(const int32_t* ctimes, const uint32_t* logs, const uint32_t* commits, const uint32_t* blk_author, const int32_t* blk_time,
                              const int32_t* startup, uint32_t i, uint32_t n, uint32_t lcap, uint32_t blocks) {
  const size_t rows = (size_t)i * n, pool = (size_t)i * (blocks + 1);
  return CwInstance{ctimes ? ctimes + rows * lcap : nullptr, logs + rows * lcap, commits + rows, blk_author + pool, blk_time + pool, startup + rows,
                    n, lcap, blocks};
}

// nc_j; the node pass: the chain's length and the reference node; the lanes of the chunk at c0 that have an entry.
inline uint32_t cw_commits(const CwInstance& v, uint32_t j) { return chn_commits(v.commits[j], v.lcap); }
struct CwChain {
  uint32_t L, ref;
};
inline CwChain cw_node_pass(const CwInstance& v) {
  uint64_t best = 0;
  for (uint32_t j = 0; j < v.n; j++) best = chn_ref_max(best, chn_ref_key(cw_commits(v, j), j));
  return CwChain{chn_ref_len(best), chn_ref_node(best)};
}
inline uint32_t cw_have(const CwChain& ch, uint32_t c0, uint32_t chunk) { return ch.L - c0 < chunk ? ch.L - c0 : chunk; }

// The proposal time of block b; false: b is none of the pool's, or its author is no node (the shims' finding -2).
inline bool cw_proposal(const CwInstance& v, uint32_t b, int32_t& out) {
  if (b == 0 || b > v.blocks || v.author[b] >= v.n) return false;
  out = v.startup[v.author[b]] + v.time[b];
  return true;
}

// Row j of the chunk at c0 into the [n][chunk] tile, FIN_NONE where node j is no committer of the entry.  false: a committer's entry
// lies at or beyond L (lane >= have) -- the finding -4 of the shims that had it; nc_j <= L by the node pass, so it cannot fire.
inline bool cw_stage(const CwInstance& v, uint32_t j, uint32_t c0, uint32_t chunk, uint32_t have, int32_t* tile) {
  const uint32_t ncj = cw_commits(v, j);
  bool inside = true;
  for (uint32_t l = 0; l < chunk; l++) {
    const uint32_t k = c0 + l;
    const int32_t c = k < ncj ? v.ctimes[(size_t)j * v.lcap + k] : FIN_NONE;
    tile[(size_t)j * chunk + l] = fin_committer(k, ncj, c) ? c : FIN_NONE;
    inside = inside && (tile[(size_t)j * chunk + l] < 0 || l < have);
  }
  return inside;
}

// The origin of the latency sample of node j at entry k: the proposal time of the block in its own log -- g, the chain's, where that
// is the chain's block b.  false: that block is none of the pool's (-2).  A commit before its origin is the shims' finding -3.
inline bool cw_own_proposal(const CwInstance& v, uint32_t j, uint32_t k, uint32_t b, int32_t g, int32_t& origin) {
  const uint32_t bj = v.logs[(size_t)j * v.lcap + k];
  origin = g;
  return bj == b || cw_proposal(v, bj, origin);
}

// For the stand-alone callers of the sanitizer builds: a case's arrays come from stdin as plain numbers, ctimes .. group_of in the
// shims' common order, then the rights table (n words, or none).
template <class T>
inline bool cw_read_into(std::vector<T>& v, size_t count) {
  v.resize(count);
  for (T& x : v) {
    long long t;
    if (scanf("%lld", &t) != 1) return false;
    x = (T)t;
  }
  return true;
}
struct CwArrays {
  std::vector<int32_t> ctimes, blk_time, startup;
  std::vector<uint32_t> logs, commits, blk_author, faults, group_of, rights;
};
inline bool cw_read_arrays(CwArrays& a, size_t m, size_t n, size_t lcap, size_t blocks, bool has_rights) {
  const size_t cells = m * n * lcap, pool = m * (blocks + 1);
  return cw_read_into(a.ctimes, cells) && cw_read_into(a.logs, cells) && cw_read_into(a.commits, m * n) && cw_read_into(a.blk_author, pool) &&
         cw_read_into(a.blk_time, pool) && cw_read_into(a.startup, m * n) && cw_read_into(a.faults, m) && cw_read_into(a.group_of, m) &&
         cw_read_into(a.rights, has_rights ? n : 0);
}

#endif  // CHAIN_WALK_HOST_H
