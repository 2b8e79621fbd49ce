// record_hash_rules_host.cpp -- TEST INFRASTRUCTURE (tests/test_record_hash_rules_host.py compiles it with g++): the word-wise record
// hashing of csrc/lbft_record_hash_rules.h (what lbft_k_rh_chain runs) next to the byte-wise hashing of lbft_core.h (SipBytes,
// record_hash_block / record_hash_vote, and a QuorumCertificate_ written as SimT::committed_record_hashes writes it).  Every function
// returns both: out[0] word-wise, out[1] byte-wise.
#include "../librabft_simulator_amd/csrc/lbft_record_hash_rules.h"

using namespace lbft;

extern "C" {

void rhr_epoch_id(uint64_t e, uint64_t* out) {
  out[0] = rh_epoch_id(e);
  out[1] = record_hash_epoch_id(e);
}

void rhr_block(uint64_t proposer, uint64_t index, uint32_t time_word, uint64_t prev_qc_hash, uint64_t round, uint64_t author, uint64_t* out) {
  out[0] = rh_block(proposer, index, time_word, prev_qc_hash, round, author);
  out[1] = record_hash_block(proposer, index, (i64)(i32)time_word, prev_qc_hash, round, author);
}

void rhr_vote(uint64_t epoch, uint64_t round, uint64_t block_hash, uint64_t state, int has_cs, uint64_t cs, uint64_t author, uint64_t* out) {
  out[0] = rh_vote(epoch, round, block_hash, state, has_cs != 0, cs, author);
  out[1] = record_hash_vote(epoch, round, block_hash, state, has_cs != 0, cs, author);
}

// voters: mask words (bit a % 32 of word a / 32 = author a voted); out[2] = the number of votes
void rhr_qc(uint64_t epoch, uint64_t round, uint64_t block_hash, uint64_t state, int has_cs, uint64_t cs, const uint32_t* voters, uint32_t words,
            uint64_t author, uint64_t* out) {
  const bool some = has_cs != 0;
  u32 votes = 0;
  for (u32 w = 0; w < words; w++) votes += (u32)__builtin_popcount(voters[w]);
  // word-wise, as the kernel: the votes' shared prefix once, then one word and the finish per author
  const RhStream vs = rh_vote_begin(epoch, round, block_hash, state, some, cs);
  RhStream q = rh_qc_begin(epoch, round, block_hash, state, some, cs, votes);
  for (u32 w = 0; w < words; w++)
    for (u32 m = voters[w]; m; m &= m - 1) {
      const u64 a = 32 * w + (u32)__builtin_ctz(m);
      rh_qc_vote(q, a, rh_vote_end(vs, a));
    }
  out[0] = rh_qc_end(q, author);
  // byte-wise, as SimT::committed_record_hashes
  SipBytes hq; hq.init();
  const char name[] = "QuorumCertificate_::";
  for (u32 i = 0; i < sizeof(name) - 1; i++) hq.byte((u32)name[i]);
  hq.u64le(epoch); hq.u64le(round); hq.u64le(block_hash); hq.u64le(state); hq.option(some, cs);
  hq.uleb(votes);
  for (u32 w = 0; w < words; w++)
    for (u32 m = voters[w]; m; m &= m - 1) {
      const u64 a = 32 * w + (u32)__builtin_ctz(m);
      hq.u64le(a); hq.u64le(a); hq.u64le(record_hash_vote(epoch, round, block_hash, state, some, cs, a));
    }
  hq.u64le(author);
  out[1] = hq.finish();
  out[2] = votes;
}

// the State after the last of `entries` (author, cmd, time word) triples
void rhr_state(const uint32_t* triples, uint32_t entries, uint64_t* out) {
  Sip13 a = rh_state_begin(entries), b;
  b.init(); b.word(entries);
  for (u32 k = 0; k < entries; k++) {
    rh_state_entry(a, triples[3 * k], triples[3 * k + 1], triples[3 * k + 2]);
    b.word(triples[3 * k]); b.word(triples[3 * k + 1]); b.word((u64)(i64)(i32)triples[3 * k + 2]);
  }
  out[0] = a.finish();
  out[1] = b.finish();
}

// a stream of arbitrary pieces: kinds[k] = 0 byte, 1 word, 2 option none, 3 option some, 4 uleb; values[k]
void rhr_stream(const uint8_t* kinds, const uint64_t* values, uint32_t pieces, uint64_t* out) {
  RhStream a; a.init();
  SipBytes b; b.init();
  for (u32 k = 0; k < pieces; k++) {
    const u64 v = values[k];
    switch (kinds[k]) {
      case 0: a.byte((u32)v); b.byte((u32)v); break;
      case 1: a.word(v); b.u64le(v); break;
      case 2: a.option(false, v); b.option(false, v); break;
      case 3: a.option(true, v); b.option(true, v); break;
      default: a.uleb((u32)(v & 0x3fffu)); b.uleb(v & 0x3fffu); break;
    }
  }
  out[0] = a.finish();
  out[1] = b.finish();
}

uint32_t rhr_width(uint32_t n) { return rh_width(n); }
uint32_t rhr_author_bits(uint32_t w, uint32_t n) { return rh_author_bits(w, n); }
uint32_t rhr_voter_field(uint32_t w, uint32_t mw) { return rh_voter_field(w, mw); }

}  // extern "C"
