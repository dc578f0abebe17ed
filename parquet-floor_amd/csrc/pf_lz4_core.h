// pf_lz4_core.h — LZ4 block format (parquet-format codec LZ4_RAW) decode core shared by the host
// model and the GPU kernel (pf_lz4.hip). Plain C++: no HIP call, no allocation, no global table.
//
// What is here: the walk over one sequence -- token, length extensions, offset -- with every
// decision that can refuse a stream. What is not here: who copies the bytes. The host model below
// (decompress_host) executes the sequences one by one; the kernel executes them in batches with
// the whole workgroup and reads the stream through an LDS window (the Reader).
//
// The rules (tests/lz4_blocks.py holds them as a Python model):
//  * a sequence is a token, literal-length extension bytes, the literals, a 2-byte little-endian
//    offset, match-length extension bytes. Literal length = high nibble, 15: add the following
//    bytes until one is not 255. Match length = low nibble + 4, extended the same way;
//  * length sums are 64-bit; a literal length past the remaining input or output, or a match length
//    past the remaining output, is refused at the byte that takes it there;
//  * the stream ends exactly after the literals of its last sequence, whose low nibble is ignored
//    (as liblz4 does). Input used up anywhere else -- before a token, in an extension, the literals
//    or the offset, right after a match -- is refused; so is the empty input. `00` is the empty output;
//  * an offset is in [1, bytes produced so far]. Offset 0 is refused (liblz4 1.9.3 accepts it and
//    copies unspecified bytes);
//  * the output is exactly `size` bytes, never a write at or past dst + size, never a read at or
//    past src + n;
//  * the encoder-side end-of-block restrictions (last 5 bytes literals, last match 12 bytes before
//    the end) are not enforced: liblz4 refuses some such streams, this core accepts them.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "pf_internal.h"

namespace pf {
namespace lz4 {

constexpr uint32_t LZ4_BATCH = 256;     // sequences per LDS batch of k_lz4
constexpr uint32_t LZ4_WINDOW = 8192;   // bytes of the input window k_lz4 stages in LDS
enum : int { L_OK = 0, L_CORRUPT = -2 };

// One sequence: ll literals at input position lit, then ml bytes from off bytes back.
// last: the stream ends after the literals (ml = off = 0).
struct Seq {
    uint32_t lit, ll, ml, off, last;
};

// The plain reader: byte i of the stream.
struct PtrReader {
    const uint8_t* p;
    PF_HD uint32_t operator()(uint32_t i) const { return p[i]; }
};

// The sequence at ip of a stream of n <= 2^30 bytes, with op of the size <= 2^30 output bytes
// produced. false: refused. ip moves past the sequence; every byte read lies below n. On the last
// sequence the output is checked to be exactly size bytes.
template <class Reader>
PF_HD inline bool next_seq(const Reader& rd, uint32_t n, uint32_t size, uint32_t& ip, uint32_t op, Seq& s) {
    if (ip >= n) return false;
    const uint32_t tok = rd(ip++);
    const uint64_t room = uint64_t(size - op);
    uint64_t ll = tok >> 4;
    if (ll == 15) {
        for (;;) {
            if (ip >= n) return false;
            const uint32_t b = rd(ip++);
            ll += b;
            if (ll > uint64_t(n - ip) || ll > room) return false;
            if (b != 255) break;
        }
    }
    if (ll > uint64_t(n - ip) || ll > room) return false;
    s.lit = ip;
    s.ll = uint32_t(ll);
    s.ml = s.off = 0;
    ip += uint32_t(ll);
    s.last = ip == n;
    if (s.last) return ll == room;
    if (n - ip < 2) return false;
    const uint32_t off = rd(ip) | (rd(ip + 1) << 8);
    ip += 2;
    if (off == 0 || uint64_t(off) > uint64_t(op) + ll) return false;
    uint64_t ml = (tok & 15u) + 4u;
    if ((tok & 15u) == 15u) {
        for (;;) {
            if (ip >= n) return false;
            const uint32_t b = rd(ip++);
            ml += b;
            if (ml > room - ll) return false;
            if (b != 255) break;
        }
    }
    if (ml > room - ll) return false;
    s.ml = uint32_t(ml);
    s.off = off;
    return true;
}

// The serial host model: L_OK when src[0 .. n) is one block that produces exactly size bytes.
inline int decompress_host(const uint8_t* src, size_t n, uint8_t* dst, size_t size) {
    if (n > (size_t(1) << 30) || size > (size_t(1) << 30)) return L_CORRUPT;
    const PtrReader rd{src};
    uint32_t ip = 0, op = 0;
    for (;;) {
        Seq s;
        if (!next_seq(rd, uint32_t(n), uint32_t(size), ip, op, s)) return L_CORRUPT;
        for (uint32_t j = 0; j < s.ll; j++) dst[op + j] = src[s.lit + j];
        op += s.ll;
        if (s.last) return L_OK;
        for (uint32_t j = 0; j < s.ml; j++) dst[op + j] = dst[op - s.off + j];
        op += s.ml;
    }
}

}  // namespace lz4
}  // namespace pf
