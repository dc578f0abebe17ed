// pf_bloom.cpp — host calls over pf_xxh64.h: pf_xxh64 and pf_bloom_check, for callers that probe the
// split-block Bloom filters of a file (pf_file_chunk_bloom locates them) without a context or a GPU.
// The same header is the kernel's hash and block arithmetic (pf_enc_bloom.hip). No GPU calls.
#include "pf_xxh64.h"
#include "pfloor.h"

extern "C" {

uint64_t pf_xxh64(const void* p, size_t n, uint64_t seed) {
    if (!p) n = 0;
    return pf::xxh64(static_cast<const uint8_t*>(p), n, seed);
}

int pf_bloom_check(const uint8_t* bitset, size_t n_bytes, uint64_t hash) {
    if (!bitset || !pf::bloom_size_ok(n_bytes)) return PF_ERR_INVALID_ARG;
    const uint8_t* blk = bitset + size_t(pf::bloom_block(hash, uint32_t(n_bytes / 32))) * 32;
    for (int i = 0; i < 8; i++)
        if (!(pf::xxh_read32(blk + 4 * i) & pf::bloom_mask(hash, i))) return 0;
    return 1;
}

}  // extern "C"
