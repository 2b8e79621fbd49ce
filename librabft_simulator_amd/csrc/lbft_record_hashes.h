// lbft_record_hashes.h -- the interface between liblbft_hip.so and liblbft_record_hashes.so (the kernel of
// lbft_batch_chain_record_hashes).  As the other side libraries, it is a code object of its own so that the machine code of
// liblbft_hip.so stays exactly what it was; liblbft_hip.so opens it on first use (dlopen beside itself) and calls the launcher on the
// batch's stream.
#ifndef LBFT_RECORD_HASHES_H
#define LBFT_RECORD_HASHES_H

#include <hip/hip_runtime.h>

#include "../../include/lbft.h"
#include "lbft_core.h"

#define LBFT_RECORD_HASHES_LIB "liblbft_record_hashes.so"
// The device-side copy of `out` is taken in chunks of instances that stay below this many bytes
#define LBFT_RH_TEMP_BYTES (256ull << 20)

extern "C" {
// The record hashes of the committed chains of instances first .. first + count - 1 (lbft_record_hash_rules.h, include/lbft.h):
// out[(inst - first) * cap + k] for k < min(length, cap) (NULL: none), heads[inst], node_prefix[inst * p->n + node] (NULL: none).
// The caller zeroes all three: the kernel writes nothing for an instance with a fault word or an empty chain beyond its prefix
// counts, and nothing past a chain's end.
typedef hipError_t (*lbft_rh_chain_fn)(const lbft::Params* p, const lbft::u32* state, lbft::u32 first, lbft::u32 count, lbft_record_hash* out,
                                       lbft::u32 cap, lbft_chain_head* heads, lbft::u32* node_prefix, hipStream_t stream);
}

#endif  // LBFT_RECORD_HASHES_H
