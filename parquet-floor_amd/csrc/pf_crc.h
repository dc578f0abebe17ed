// pf_crc.h — CRC-32 arithmetic (reflected polynomial 0xEDB88320, as zlib / java.util.zip.CRC32) shared by
// the read side (pf_scan.hip: k_page_crc verifies PageHeader.crc), the write side (pf_enc_crc.hip: k_enc_crc
// computes the pieces of a page) and the host fold of those pieces (pf_enc_plan.cpp). Internal.
//
// A raw CRC (zero init, no final xor) is linear in the data: raw(A ‖ B) = raw(A) * x^(8 |B|) + raw(B) mod P,
// so the pieces of a page are reduced independently and folded in order.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PF_CRC_FN __host__ __device__ inline
#else
#define PF_CRC_FN inline
#endif

namespace pf {

constexpr uint32_t CRC_POLY = 0xedb88320u;

// a * b mod P in the reflected representation (x^0 = bit 31).
PF_CRC_FN uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

// x^(8n) mod P from x2n[k] = x^(2^k) mod P.
PF_CRC_FN uint32_t crc_x8n(uint64_t n, const uint32_t* x2n) {
    uint32_t p = 1u << 31;
    unsigned k = 3;
    while (n) {
        if (n & 1) p = crc_mulmod(x2n[k & 31], p);
        n >>= 1;
        k++;
    }
    return p;
}

// x2n[k] = x^(2^k) mod P, k < 32 (the powers repeat with period 32 beyond that: x^(2^32 - 1) = 1).
PF_CRC_FN void crc_x2n_table(uint32_t* x2n) {
    uint32_t p = 1u << 30;   // x^1
    x2n[0] = p;
    for (int k = 1; k < 32; k++) x2n[k] = p = crc_mulmod(p, p);
}

// ---- host fold (plain C++) ----
struct CrcPowers {
    uint32_t x2n[32];
    CrcPowers() { crc_x2n_table(x2n); }
};
inline const uint32_t* crc_x2n_host() {
    static const CrcPowers t;
    return t.x2n;
}

// Raw CRC of a ‖ b from raw(a), raw(b) and x^(8 |b|) mod P (k_enc_crc hands that power back with every
// piece, so the fold of a piece is one multiplication).
inline uint32_t crc_combine_pow(uint32_t raw_a, uint32_t raw_b, uint32_t x8len_b) { return crc_mulmod(x8len_b, raw_a) ^ raw_b; }

// Raw CRC of a ‖ b from raw(a), raw(b) and |b|.
inline uint32_t crc_combine(uint32_t raw_a, uint32_t raw_b, uint64_t len_b) {
    return crc_combine_pow(raw_a, raw_b, crc_x8n(len_b, crc_x2n_host()));
}

struct CrcTable {
    uint32_t t[256];
    CrcTable() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
            t[i] = c;
        }
    }
};

// Raw CRC of `n` bytes appended to data whose raw CRC is `raw` (a byte at a time: the host only feeds the
// bytes it generates itself -- a length varint, a run header, the levels of a column without a validity array).
inline uint32_t crc_raw_bytes(uint32_t raw, const uint8_t* p, size_t n) {
    static const CrcTable tab;
    for (size_t i = 0; i < n; i++) raw = tab.t[(raw ^ p[i]) & 0xffu] ^ (raw >> 8);
    return raw;
}

// Standard CRC32 of `len` bytes from their raw CRC:
// raw(data, init ~0) ^ ~0 = raw(data, 0) ^ (~0 * x^(8 len)) ^ ~0.
inline uint32_t crc_finish(uint32_t raw, uint64_t len) {
    return raw ^ crc_mulmod(crc_x8n(len, crc_x2n_host()), 0xffffffffu) ^ 0xffffffffu;
}

}  // namespace pf
