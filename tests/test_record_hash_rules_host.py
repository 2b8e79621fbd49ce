"""The word-wise record hashing of csrc/lbft_record_hash_rules.h (what lbft_k_rh_chain runs), compiled for the host
(tests/record_hash_rules_host.cpp), against the byte-wise hashing of lbft_core.h that lbft_batch_committed_record_hashes uses and against
a SipHash-1-3 over the BCS bytes written here in Python: Block_, Vote_, QuorumCertificate_ and EpochId on random fields, both
committed_state cases, 0 to 128 votes (128: the two-byte ULEB) with 128-bit voter masks, the State, and the stream writer on random
sequences of bytes, words, options and lengths (every byte phase)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from support import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
VOTE_COUNTS = (0, 1, 3, 63, 64, 65, 127, 128)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = build_shim(tmp_path_factory.mktemp("rh_rules"), "record_hash_rules_host.cpp", "librh_rules.so", "-ffp-contract=off", "-w")
    u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
    L.rhr_epoch_id.argtypes = [u64, vp]
    L.rhr_block.argtypes = [u64, u64, u32, u64, u64, u64, vp]
    L.rhr_vote.argtypes = [u64, u64, u64, u64, C.c_int, u64, u64, vp]
    L.rhr_qc.argtypes = [u64, u64, u64, u64, C.c_int, u64, vp, u32, u64, vp]
    L.rhr_state.argtypes = [vp, u32, vp]
    L.rhr_stream.argtypes = [vp, vp, u32, vp]
    for f in (L.rhr_width, L.rhr_author_bits, L.rhr_voter_field):
        f.restype = u32
    return L


def siphash13(data):
    """SipHash-1-3, keys (0, 0): Rust's DefaultHasher."""
    v = [0x736f6d6570736575, 0x646f72616e646f6d, 0x6c7967656e657261, 0x7465646279746573]

    def rotl(x, b):
        return ((x << b) | (x >> (64 - b))) & M64

    def rnd():
        v[0] = (v[0] + v[1]) & M64; v[1] = rotl(v[1], 13); v[1] ^= v[0]; v[0] = rotl(v[0], 32)
        v[2] = (v[2] + v[3]) & M64; v[3] = rotl(v[3], 16); v[3] ^= v[2]
        v[0] = (v[0] + v[3]) & M64; v[3] = rotl(v[3], 21); v[3] ^= v[0]
        v[2] = (v[2] + v[1]) & M64; v[1] = rotl(v[1], 17); v[1] ^= v[2]; v[2] = rotl(v[2], 32)
    tail = len(data) % 8
    for o in range(0, len(data) - tail, 8):
        m, = struct.unpack_from("<Q", data, o)
        v[3] ^= m; rnd(); v[0] ^= m
    b = ((len(data) & 0xff) << 56) | int.from_bytes(data[len(data) - tail:], "little")
    v[3] ^= b; rnd(); v[0] ^= b
    v[2] ^= 0xff
    rnd(); rnd(); rnd()
    return v[0] ^ v[1] ^ v[2] ^ v[3]


def u64le(x):
    return struct.pack("<Q", x & M64)


def option(some, x):
    return b"\x01" + u64le(x) if some else b"\x00"


def uleb(x):
    out = b""
    while x >= 0x80:
        out += bytes([(x & 0x7f) | 0x80])
        x >>= 7
    return out + bytes([x])


def pair(n=2):
    return np.zeros(n, dtype=np.uint64)


def rnd64(rng):
    return int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))


def test_block_vote_epoch_and_state_equal_the_byte_wise_hashes(shim):
    rng = np.random.default_rng(20261019)
    out = pair()
    for trial in range(300):
        proposer, index, prev, rnd_, author, epoch, bh, state, cs = (rnd64(rng) for _ in range(9))
        tw = int(rng.integers(0, 1 << 32)) if trial % 3 else int(rng.choice([0, 1, 0x7fffffff, 0x80000000, 0xffffffff]))
        signed = tw - (1 << 32) if tw >= 1 << 31 else tw  # the time enters as (u64)(i64)(i32)
        shim.rhr_block(proposer, index, tw, prev, rnd_, author, out.ctypes.data)
        assert out[0] == out[1] == siphash13(b"Block_::" + u64le(proposer) + u64le(index) + u64le(signed) + u64le(prev) + u64le(rnd_) + u64le(author))
        for some in (0, 1):
            shim.rhr_vote(epoch, rnd_, bh, state, some, cs, author, out.ctypes.data)
            assert out[0] == out[1] == siphash13(b"Vote_::" + u64le(epoch) + u64le(rnd_) + u64le(bh) + u64le(state) + option(some, cs) + u64le(author))
        shim.rhr_epoch_id(epoch, out.ctypes.data)
        assert out[0] == out[1] == siphash13(b"EpochId::" + u64le(epoch))
        entries = int(rng.integers(0, 70))
        triples = rng.integers(0, 1 << 32, size=3 * entries, dtype=np.uint64).astype(np.uint32)
        shim.rhr_state(triples.ctypes.data, entries, out.ctypes.data)
        words = [entries] + [int(x) if k % 3 != 2 or x < 1 << 31 else int(x) - (1 << 32) for k, x in enumerate(triples)]
        assert out[0] == out[1] == siphash13(b"".join(u64le(w) for w in words))


@pytest.mark.parametrize("votes", VOTE_COUNTS)
def test_quorum_certificates_equal_the_byte_wise_hash(shim, votes):
    rng = np.random.default_rng(1000 + votes)
    out = pair(3)
    for trial in range(12):
        epoch, rnd_, bh, state, cs, author = (rnd64(rng) for _ in range(6))
        voters = np.sort(rng.choice(128, size=votes, replace=False))
        mask = np.zeros(4, dtype=np.uint32)
        for a in voters:
            mask[a // 32] |= np.uint32(1 << (a % 32))
        for some in (0, 1):
            shim.rhr_qc(epoch, rnd_, bh, state, some, cs, mask.ctypes.data, 4, author, out.ctypes.data)
            body = b"QuorumCertificate_::" + u64le(epoch) + u64le(rnd_) + u64le(bh) + u64le(state) + option(some, cs) + uleb(votes)
            for a in voters:
                vote = siphash13(b"Vote_::" + u64le(epoch) + u64le(rnd_) + u64le(bh) + u64le(state) + option(some, cs) + u64le(int(a)))
                body += u64le(int(a)) + u64le(int(a)) + u64le(vote)
            body += u64le(author)
            assert len(uleb(votes)) == (2 if votes >= 128 else 1)
            assert out[2] == votes and out[0] == out[1] == siphash13(body), (votes, trial, some)


def test_stream_writer_equals_the_byte_writer_in_every_phase(shim):
    rng = np.random.default_rng(7)
    out = pair()
    phases = set()
    for trial in range(400):
        pieces = int(rng.integers(0, 40))
        kinds = rng.integers(0, 5, size=pieces).astype(np.uint8)
        values = np.array([rnd64(rng) for _ in range(pieces)], dtype=np.uint64)
        shim.rhr_stream(kinds.ctypes.data, values.ctypes.data, pieces, out.ctypes.data)
        assert out[0] == out[1], (trial, kinds.tolist())
        data = b""
        for k, v in zip(kinds, values):
            v = int(v)
            if k == 1:
                phases.add(len(data) % 8)
            data += {0: bytes([v & 0xff]), 1: u64le(v), 2: b"\x00", 3: b"\x01" + u64le(v)}.get(int(k), uleb(v & 0x3fff))
        assert out[0] == siphash13(data)
    assert phases == set(range(8))  # a word was appended with 0 .. 7 bytes held


def test_segment_width_author_bits_and_voter_fields(shim):
    assert [shim.rhr_width(n) for n in (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 40, 64, 65, 100, 128)] == \
        [4, 4, 4, 4, 8, 8, 8, 16, 16, 32, 32, 64, 64, 64, 64, 64, 64]
    for n in (1, 3, 4, 31, 32, 33, 40, 64, 65, 100, 127, 128):
        bits = sum(bin(shim.rhr_author_bits(w, n)).count("1") for w in range(4))
        assert bits == n and all(shim.rhr_author_bits(w, n) == ((1 << max(0, min(32, n - 32 * w))) - 1) for w in range(4)), n
    # B_VOTERS, then the fourth run of extension words behind the record (csrc/lbft_core.h: KNOWN, QC, PEND, VOTERS)
    core = open(os.path.join(ROOT, "librabft_simulator_amd", "csrc", "lbft_core.h")).read()
    assert "k == 0 ? (u32)B_VOTERS : B_WORDS + 3 * (MW() - 1) + k - 1" in core
    v0 = shim.rhr_voter_field(0, 1)
    assert [shim.rhr_voter_field(0, mw) for mw in (1, 2, 4)] == [v0] * 3
    assert [shim.rhr_voter_field(w, 4) - v0 for w in (1, 2, 3)] == [1 + 9, 1 + 10, 1 + 11]
    assert shim.rhr_voter_field(1, 2) - v0 == 1 + 3
