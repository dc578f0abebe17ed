// pf_xxh64.h — XXH64 (xxHash, 64-bit) and the split-block Bloom filter arithmetic of parquet-format
// (BloomFilter.md), shared by the device kernel (pf_enc_bloom.hip) and the host calls (pf_bloom.cpp:
// pf_xxh64, pf_bloom_check). One text for both sides: plain C++ on unsigned integers, loads through
// memcpy (any alignment, little-endian on both), no intrinsics, so the CPU test of the host calls is a
// test of the kernel's arithmetic. Internal.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PF_XXH_FN __host__ __device__ inline
#else
#define PF_XXH_FN inline
#endif

namespace pf {

constexpr uint64_t XXH_P1 = 0x9E3779B185EBCA87ull, XXH_P2 = 0xC2B2AE3D27D4EB4Full, XXH_P3 = 0x165667B19E3779F9ull,
                   XXH_P4 = 0x85EBCA77C2B2AE63ull, XXH_P5 = 0x27D4EB2F165667C5ull;

PF_XXH_FN uint64_t xxh_rotl(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
PF_XXH_FN uint64_t xxh_round(uint64_t acc, uint64_t in) { return xxh_rotl(acc + in * XXH_P2, 31) * XXH_P1; }
PF_XXH_FN uint64_t xxh_merge(uint64_t h, uint64_t v) { return (h ^ xxh_round(0, v)) * XXH_P1 + XXH_P4; }
PF_XXH_FN uint64_t xxh_avalanche(uint64_t h) {
    h ^= h >> 33; h *= XXH_P2;
    h ^= h >> 29; h *= XXH_P3;
    return h ^ (h >> 32);
}
PF_XXH_FN uint64_t xxh_read64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
PF_XXH_FN uint32_t xxh_read32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

// The closed forms of a 4- and an 8-byte input (the PLAIN bytes of INT32 / FLOAT and INT64 / DOUBLE): the
// general function's 4-byte and 8-byte tail step alone.
PF_XXH_FN uint64_t xxh64_u32(uint32_t k, uint64_t seed) {
    uint64_t h = seed + XXH_P5 + 4;
    h ^= uint64_t(k) * XXH_P1;
    return xxh_avalanche(xxh_rotl(h, 23) * XXH_P2 + XXH_P3);
}
PF_XXH_FN uint64_t xxh64_u64(uint64_t k, uint64_t seed) {
    uint64_t h = seed + XXH_P5 + 8;
    h ^= xxh_round(0, k);
    return xxh_avalanche(xxh_rotl(h, 27) * XXH_P1 + XXH_P4);
}

// XXH64 of n bytes at p (any alignment).
PF_XXH_FN uint64_t xxh64(const uint8_t* p, size_t n, uint64_t seed) {
    const uint8_t* const end = p + n;
    uint64_t h;
    if (n >= 32) {
        uint64_t v1 = seed + XXH_P1 + XXH_P2, v2 = seed + XXH_P2, v3 = seed, v4 = seed - XXH_P1;
        do {
            v1 = xxh_round(v1, xxh_read64(p));
            v2 = xxh_round(v2, xxh_read64(p + 8));
            v3 = xxh_round(v3, xxh_read64(p + 16));
            v4 = xxh_round(v4, xxh_read64(p + 24));
            p += 32;
        } while (size_t(end - p) >= 32);
        h = xxh_rotl(v1, 1) + xxh_rotl(v2, 7) + xxh_rotl(v3, 12) + xxh_rotl(v4, 18);
        h = xxh_merge(h, v1);
        h = xxh_merge(h, v2);
        h = xxh_merge(h, v3);
        h = xxh_merge(h, v4);
    } else {
        h = seed + XXH_P5;
    }
    h += uint64_t(n);
    while (size_t(end - p) >= 8) {
        h ^= xxh_round(0, xxh_read64(p));
        h = xxh_rotl(h, 27) * XXH_P1 + XXH_P4;
        p += 8;
    }
    if (size_t(end - p) >= 4) {
        h ^= uint64_t(xxh_read32(p)) * XXH_P1;
        h = xxh_rotl(h, 23) * XXH_P2 + XXH_P3;
        p += 4;
    }
    while (p < end) {
        h ^= uint64_t(*p++) * XXH_P5;
        h = xxh_rotl(h, 11) * XXH_P1;
    }
    return xxh_avalanche(h);
}

// ---- split-block Bloom filter: blocks of eight uint32 words, one bit per word and hash ----
constexpr uint32_t BLOOM_MIN_BYTES = 32, BLOOM_MAX_BYTES = 128u << 20;

PF_XXH_FN bool bloom_size_ok(uint64_t bytes) {
    return bytes >= BLOOM_MIN_BYTES && bytes <= BLOOM_MAX_BYTES && (bytes & (bytes - 1)) == 0;
}
// first word of the hash's block
PF_XXH_FN uint32_t bloom_block(uint64_t h, uint32_t n_blocks) { return uint32_t(((h >> 32) * uint64_t(n_blocks)) >> 32); }
// the bit the hash sets in word i of its block
PF_XXH_FN uint32_t bloom_mask(uint64_t h, int i) {
    constexpr uint32_t SALT[8] = {0x47b6137bu, 0x44974d91u, 0x8824ad5bu, 0xa2b7289du, 0x705495c7u, 0x2df1424bu, 0x9efc4947u, 0x5c6bfb31u};
    return 1u << ((uint32_t(h) * SALT[i]) >> 27);
}

}  // namespace pf
