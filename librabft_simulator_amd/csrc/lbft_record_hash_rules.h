// lbft_record_hash_rules.h -- how the records behind a committed chain are hashed a word at a time (lbft_batch_chain_record_hashes,
// include/lbft.h).  Compiled by the device kernel (lbft_k_rh_chain, lbft_record_hashes.hip) and by plain C++ host shims
// (tests/record_hash_rules_host.cpp, tests/record_hashes_host_model.cpp), so the CPU tests check the same code the GPU runs.  Needs
// nothing but <stdint.h> and lbft_core.h (LBFT_HD, the SipHash round, Sip13, the block record's field names).
//
// The reference hashes a record as SipHash-1-3 (keys 0, 0) over "Name::" followed by its BCS bytes; lbft_core.h's SipBytes restates that
// byte by byte.  Every record hashed here is a name of known length followed by u64 fields, one Option<u64> (a tag byte, then the u64 if
// the tag is 1) and one ULEB128 sequence length, so a writer that carries (the bytes not yet hashed, how many they are) appends a u64
// with one pair of shifts and one SipRound:
//   Block_::              8 bytes, then 6 u64: every field is a SipHash word of its own
//   Vote_::               7 bytes, 4 u64, the Option (1 or 9 bytes: 40 or 48 bytes so far, a word boundary), the author
//   QuorumCertificate_::  20 bytes, 4 u64, the Option, the ULEB of the number of votes (1 byte below 128 votes, else 2), then
//                         (author, author, hash of the author's Vote_) per vote in ascending author order, then the QC's author
//   EpochId::             9 bytes, 1 u64
#ifndef LBFT_RECORD_HASH_RULES_H
#define LBFT_RECORD_HASH_RULES_H

#include <stdint.h>

#include "lbft_core.h"

namespace lbft {

// Flag bits of an entry (lbft_record_hash.flags): the first two are SimT::committed_record_hashes'.
enum { RH_NO_QC = 1u, RH_INCONSISTENT = 2u, RH_BAD_ID = 4u };

// The names as little-endian words.
#define LBFT_RH_NAME_BLOCK 0x3a3a5f6b636f6c42ULL /* "Block_::" */
#define LBFT_RH_NAME_VOTE 0x003a3a5f65746f56ULL  /* "Vote_::", 7 bytes */
#define LBFT_RH_NAME_QC0 0x65436d75726f7551ULL   /* "QuorumCe" */
#define LBFT_RH_NAME_QC1 0x7461636966697472ULL   /* "rtificat" */
#define LBFT_RH_NAME_QC2 0x3a3a5f65ULL           /* "e_::", 4 bytes */
#define LBFT_RH_NAME_EPOCH0 0x3a644968636f7045ULL /* "EpochId:" */
#define LBFT_RH_NAME_EPOCH1 0x3aULL               /* ":", 1 byte */

// SipHash-1-3 over a byte stream, written a word at a time: `buf` holds the `held` (0..7) bytes that do not fill a word yet.
struct RhStream {
  u64 v0, v1, v2, v3, buf;
  u32 held, total;
  LBFT_HD void init() {
    v0 = 0x736f6d6570736575ULL; v1 = 0x646f72616e646f6dULL; v2 = 0x6c7967656e657261ULL; v3 = 0x7465646279746573ULL;
    buf = 0; held = 0; total = 0;
  }
  LBFT_HD void round(u64 m) { v3 ^= m; LBFT_SIPROUND v0 ^= m; }
  // the first `bytes` (1..8) bytes of a name, on a word boundary
  LBFT_HD void name(u64 w, u32 bytes) {
    if (bytes == 8) round(w); else { buf = w; held = bytes; }
    total += bytes;
  }
  LBFT_HD void word(u64 x) {  // BCS u64 / usize
    const u32 s = 8 * held;
    round(buf | (x << s));
    buf = held ? x >> (64 - s) : 0;
    total += 8;
  }
  LBFT_HD void byte(u32 c) {
    buf |= (u64)(c & 0xffu) << (8 * held);
    total++;
    if (++held == 8) { round(buf); buf = 0; held = 0; }
  }
  LBFT_HD void option(bool some, u64 v) { byte(some ? 1u : 0u); if (some) word(v); }  // BCS Option<u64>
  LBFT_HD void uleb(u32 v) {  // BCS sequence length below 2^14
    if (v >= 0x80u) { byte(v | 0x80u); v >>= 7; }
    byte(v);
  }
  LBFT_HD u64 finish() {
    const u64 b = ((u64)total << 56) | buf;
    v3 ^= b; LBFT_SIPROUND v0 ^= b;
    v2 ^= 0xff;
    LBFT_SIPROUND LBFT_SIPROUND LBFT_SIPROUND
    return v0 ^ v1 ^ v2 ^ v3;
  }
};

// context.hash(&EpochId(e)): what the first block of an epoch takes for its previous QC hash
LBFT_HD u64 rh_epoch_id(u64 e) {
  RhStream h; h.init();
  h.name(LBFT_RH_NAME_EPOCH0, 8); h.name(LBFT_RH_NAME_EPOCH1, 1);
  h.word(e);
  return h.finish();
}
// Block_: command (proposer, index), time, previous_quorum_certificate_hash, round, author.  `time`: the block record's B_TIME word.
LBFT_HD u64 rh_time(u32 time_word) { return (u64)(i64)(i32)time_word; }
LBFT_HD u64 rh_block(u64 proposer, u64 index, u32 time_word, u64 prev_qc_hash, u64 round, u64 author) {
  RhStream h; h.init();
  h.name(LBFT_RH_NAME_BLOCK, 8);
  h.word(proposer); h.word(index); h.word(rh_time(time_word)); h.word(prev_qc_hash); h.word(round); h.word(author);
  return h.finish();
}
// Vote_: epoch_id, round, certified_block_hash, state, committed_state -- what every vote for one block shares -- then the author
LBFT_HD RhStream rh_vote_begin(u64 epoch, u64 round, u64 block_hash, u64 state, bool has_cs, u64 cs) {
  RhStream h; h.init();
  h.name(LBFT_RH_NAME_VOTE, 7);
  h.word(epoch); h.word(round); h.word(block_hash); h.word(state); h.option(has_cs, cs);
  return h;
}
LBFT_HD u64 rh_vote_end(RhStream h, u64 author) { h.word(author); return h.finish(); }
LBFT_HD u64 rh_vote(u64 epoch, u64 round, u64 block_hash, u64 state, bool has_cs, u64 cs, u64 author) {
  return rh_vote_end(rh_vote_begin(epoch, round, block_hash, state, has_cs, cs), author);
}
// QuorumCertificate_: epoch_id, round, certified_block_hash, state, committed_state, votes, author
LBFT_HD RhStream rh_qc_begin(u64 epoch, u64 round, u64 block_hash, u64 state, bool has_cs, u64 cs, u32 votes) {
  RhStream h; h.init();
  h.name(LBFT_RH_NAME_QC0, 8); h.name(LBFT_RH_NAME_QC1, 8); h.name(LBFT_RH_NAME_QC2, 4);
  h.word(epoch); h.word(round); h.word(block_hash); h.word(state); h.option(has_cs, cs);
  h.uleb(votes);
  return h;
}
LBFT_HD void rh_qc_vote(RhStream& h, u64 author, u64 vote_hash) { h.word(author); h.word(author); h.word(vote_hash); }  // (Author, Signature{author, hash})
LBFT_HD u64 rh_qc_end(RhStream h, u64 author) { h.word(author); return h.finish(); }

// State after entry k = DefaultHasher over the k + 1 first (proposer, index, time): the length first, so no two states share a prefix
LBFT_HD Sip13 rh_state_begin(u32 entries) { Sip13 h; h.init(); h.word(entries); return h; }
LBFT_HD void rh_state_entry(Sip13& h, u32 author, u32 cmd, u32 time_word) { h.word(author); h.word(cmd); h.word(rh_time(time_word)); }

// vote_committed_state (record_store.rs:237-255): three contiguous rounds commit the grandparent's state
LBFT_HD bool rh_has_cs(u32 prev, u32 pp, u32 round, u32 prev_round, u32 pp_round) {
  return prev && pp && round == prev_round + 1 && prev_round == pp_round + 1;
}
// Word w of a block's voters is field B_VOTERS (w == 0) or an extension word behind the record (mw = mask words of the network)
LBFT_HD u32 rh_voter_field(u32 w, u32 mw) { return w == 0 ? (u32)B_VOTERS : (u32)B_WORDS + 3 * (mw - 1) + w - 1; }
// ... of which the bits of authors below n count
LBFT_HD u32 rh_author_bits(u32 w, u32 n) { return n >= 32 * (w + 1) ? 0xffffffffu : n > 32 * w ? (1u << (n - 32 * w)) - 1u : 0u; }
// A block id is an index into the pool when it lies in 1 .. nblocks
LBFT_HD bool rh_valid_id(u32 b, u32 nblocks) { return b - 1u < nblocks; }

// The segment of lanes that walks one instance: the smallest power of two >= n, at least 4 and at most 64 (networks above 64 nodes
// take their nodes and voters in two rounds).
LBFT_HD u32 rh_width(u32 n) {
  u32 w = 4;
  while (w < n && w < 64) w <<= 1;
  return w;
}

}  // namespace lbft
#endif  // LBFT_RECORD_HASH_RULES_H
