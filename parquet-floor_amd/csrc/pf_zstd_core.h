// pf_zstd_core.h — Zstandard (RFC 8878) decode core shared by the host model and the GPU kernel
// (pf_zstd.hip). Plain C++: no HIP call, no allocation, no global table (the predefined
// distributions and the code baselines are arithmetic), so every function compiles for both sides.
//
// What is here: frame / block / literals / sequences headers, the backward bit reader, the FSE
// table build from normalised counts, the Huffman table from direct or FSE-compressed weights,
// Huffman stream decode, the sequence decoder with the repeat-offset rules, and every bounds and
// limit check. What is not here: who copies the bytes. The host model below (decompress_host)
// executes sequences serially; the kernel executes them in batches with the whole workgroup.
//
// Rules beyond RFC 8878 that follow libzstd's one-shot decoder (pinned by tests/test_zstd_core.py):
// a compressed block with Huffman literals needs >= 5 bytes, four streams need >= 6 literals and
// >= 10 stream bytes, a window above 2^31 is refused, four Huffman streams of >= 8 bytes each need
// not be used up exactly (huf_stream), the content checksum is consumed and not verified (page
// integrity is the page CRC of pf_scan_pages).
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "pf_internal.h"

namespace pf {
namespace zstd {

constexpr uint32_t Z_BLOCK_MAX = 128u << 10;   // Block_Maximum_Size
constexpr int Z_LL_LOG = 9, Z_OF_LOG = 8, Z_ML_LOG = 9, Z_HUF_LOG = 11, Z_WT_LOG = 6;
constexpr int Z_LL_MAX = 35, Z_OF_MAX = 31, Z_ML_MAX = 52;
constexpr int Z_WINDOW_LOG_MAX = 31;
enum : int { Z_OK = 0, Z_CORRUPT = -2 };

// One FSE decode cell. base: the code's baseline (LL / ML / OF tables), unused for weights.
struct Ent {
    uint16_t next;
    uint8_t nb, sym;
    uint32_t base;
};
struct HufEnt {
    uint8_t sym, nb;
};

// Entropy state of one frame (LDS on the GPU, 16.3 KiB) with the scratch its table builds need.
// The Huffman side (huf .. start) and the sequence side (ll .. snext) are built by different threads.
struct Tables {
    Ent ll[1 << Z_LL_LOG], of[1 << Z_OF_LOG], ml[1 << Z_ML_LOG];
    HufEnt huf[1 << Z_HUF_LOG];
    Ent wt[1 << Z_WT_LOG];
    int16_t hnorm[256];
    uint16_t hnext[256];
    int16_t snorm[64];
    uint16_t snext[64];
    uint8_t weights[256];
    uint32_t rank[16], start[16];
    uint32_t rep[3];
    uint8_t ll_log, of_log, ml_log, huf_log, fse_ok, huf_ok;
    uint8_t huf_pairs;   // libzstd would read this table two symbols a lookup (huf_pairs_for)
};

PF_HD inline uint32_t hibit(uint32_t v) { return 31u - uint32_t(__builtin_clz(v)); }   // v > 0

// n <= 32 bits at bit position pos of the little-endian bit array p[0 .. len); bits outside read 0.
PF_HD inline uint32_t bits_at(const uint8_t* p, uint32_t len, int64_t pos, uint32_t n) {
    if (n == 0 || pos + int64_t(n) <= 0) return 0;
    const int64_t s = pos < 0 ? 0 : pos;
    const uint64_t b0 = uint64_t(s) >> 3;
    uint64_t v = 0;
    for (uint32_t k = 0; k < 5; k++)
        if (b0 + k < len) v |= uint64_t(p[b0 + k]) << (8 * k);
    v >>= (s & 7);
    v &= (uint64_t(1) << uint32_t(pos + n - s)) - 1;
    return uint32_t(pos < 0 ? v << uint32_t(-pos) : v);
}

// Backward bit reader: bits are taken from the top of the stream down. c holds 64 bits of the
// stream of which the low `have` (56..63 after a refill) lie below pos. pos < 0: the stream was
// overrun (the missing bits read as 0); callers test it where the format says so.
struct BitR {
    const uint8_t* p;
    uint32_t len;
    uint32_t lo;    // readable bytes below p (Huffman streams that follow other streams), else 0
    int32_t have;
    int64_t pos;
    uint64_t c;
};
PF_HD inline void br_refill(BitR& b) {
    const int64_t B = (b.pos - 56) >> 3;   // floor: first byte of the window, may be negative
    uint64_t c = 0;
    if (B >= 0 && uint64_t(B) + 8 <= b.len) {
        __builtin_memcpy(&c, b.p + B, 8);
    } else {
        for (int k = 0; k < 8; k++) {
            const int64_t i = B + k;
            if (i >= -int64_t(b.lo) && i < int64_t(b.len)) c |= uint64_t(b.p[i]) << (8 * k);
        }
    }
    b.c = c;
    b.have = int32_t(b.pos - 8 * B);
}
PF_HD inline bool br_init(BitR& b, const uint8_t* p, uint32_t len, uint32_t lo = 0) {
    if (len < 1 || p[len - 1] == 0) return false;   // no end mark
    b.p = p;
    b.len = len;
    b.lo = lo;
    b.pos = int64_t(len - 1) * 8 + hibit(p[len - 1]);
    br_refill(b);
    return true;
}
PF_HD inline uint32_t br_peek(BitR& b, uint32_t n) {   // n <= 32
    if (b.have < int32_t(n)) br_refill(b);
    return n ? uint32_t((b.c >> uint32_t(b.have - int32_t(n))) & ((uint64_t(1) << n) - 1)) : 0u;
}
PF_HD inline void br_skip(BitR& b, uint32_t n) { b.have -= int32_t(n); b.pos -= n; }
PF_HD inline uint32_t br_read(BitR& b, uint32_t n) {
    const uint32_t v = br_peek(b, n);
    br_skip(b, n);
    return v;
}

// ---- code baselines and predefined distributions ----
PF_HD inline uint32_t ll_bits(uint32_t c) { return c < 16 ? 0 : c < 20 ? 1 : c < 22 ? 2 : c < 24 ? 3 : c == 24 ? 4 : c - 19; }
PF_HD inline uint32_t ml_bits(uint32_t c) { return c < 32 ? 0 : c < 36 ? 1 : c < 38 ? 2 : c < 40 ? 3 : c < 42 ? 4 : c == 42 ? 5 : c - 36; }
PF_HD inline uint32_t ll_base(uint32_t c) {
    if (c < 16) return c;
    uint32_t b = 16;
    for (uint32_t k = 16; k < c; k++) b += 1u << ll_bits(k);
    return b;
}
PF_HD inline uint32_t ml_base(uint32_t c) {
    if (c < 32) return c + 3;
    uint32_t b = 35;
    for (uint32_t k = 32; k < c; k++) b += 1u << ml_bits(k);
    return b;
}
PF_HD inline int ll_default(int s) { return s == 0 ? 4 : s == 1 ? 3 : s < 13 ? 2 : s < 16 ? 1 : s < 25 ? 2 : s == 25 ? 3 : s == 26 ? 2 : s < 32 ? 1 : -1; }
PF_HD inline int ml_default(int s) { return s == 0 ? 1 : s == 1 ? 4 : s == 2 ? 3 : s < 9 ? 2 : s < 46 ? 1 : -1; }
PF_HD inline int of_default(int s) { return s < 6 ? 1 : s < 9 ? 2 : s < 24 ? 1 : -1; }

enum : int { K_WT = 0, K_LL = 1, K_OF = 2, K_ML = 3 };
PF_HD inline uint32_t code_base(int kind, uint32_t s) {
    return kind == K_LL ? ll_base(s) : kind == K_ML ? ml_base(s) : kind == K_OF ? (1u << s) : 0u;
}

// ---- FSE ----
// Normalised counts of an FSE table description (forward bit stream). nsym: symbols described.
PF_HD inline bool fse_read_ncount(const uint8_t* p, uint32_t n, int max_log, int max_sym, int16_t* norm, int& log,
                                  int& nsym, uint32_t& used) {
    if (n < 1) return false;
    int64_t pos = 4;
    log = 5 + int(bits_at(p, n, 0, 4));
    if (log > max_log) return false;
    int remaining = 1 << log, s = 0;
    while (remaining > 0 && s <= max_sym) {
        const uint32_t nb = hibit(uint32_t(remaining) + 1) + 1;
        uint32_t val = bits_at(p, n, pos, nb);
        pos += nb;
        const uint32_t lower = (1u << (nb - 1)) - 1, thr = (1u << nb) - 1 - (uint32_t(remaining) + 1);
        if ((val & lower) < thr) { pos -= 1; val &= lower; }
        else if (val > lower) val -= thr;
        const int proba = int(val) - 1;
        remaining -= proba < 0 ? 1 : proba;
        norm[s++] = int16_t(proba);
        if (proba == 0) {
            for (;;) {
                const uint32_t rep = bits_at(p, n, pos, 2);
                pos += 2;
                for (uint32_t r = 0; r < rep; r++) {
                    if (s > max_sym) return false;
                    norm[s++] = 0;
                }
                if (rep != 3) break;
            }
        }
    }
    if (remaining != 0) return false;
    nsym = s;
    used = uint32_t((pos + 7) >> 3);
    return used <= n;
}

// Decode table of 1 << log cells from normalised counts that sum to 1 << log (-1 counts as 1).
PF_HD inline bool fse_build(const int16_t* norm, int nsym, int log, Ent* t, uint16_t* next, int kind) {
    const uint32_t size = 1u << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    uint32_t high = size;
    for (int s = 0; s < nsym; s++) {
        if (norm[s] == -1) { t[--high].sym = uint8_t(s); next[s] = 1; }
        else next[s] = uint16_t(norm[s]);
    }
    uint32_t pos = 0;
    for (int s = 0; s < nsym; s++)
        for (int i = 0; i < norm[s]; i++) {
            t[pos].sym = uint8_t(s);
            do pos = (pos + step) & mask; while (pos >= high);
        }
    if (pos != 0) return false;
    for (uint32_t u = 0; u < size; u++) {
        const uint32_t s = t[u].sym, ns = next[s]++;
        const uint32_t nb = uint32_t(log) - hibit(ns);
        t[u].nb = uint8_t(nb);
        t[u].next = uint16_t((ns << nb) - size);
        t[u].base = code_base(kind, s);
    }
    return true;
}

// ---- Huffman ----
// Tree description at p[0 .. n) -> T.huf / T.huf_log. used: its bytes.
PF_HD inline bool huf_read(const uint8_t* p, uint32_t n, Tables& T, uint32_t& used) {
    if (n < 1) return false;
    const uint32_t hb = p[0];
    uint8_t* w = T.weights;
    uint32_t nw = 0;
    if (hb >= 128) {   // direct: 4 bits per weight
        nw = hb - 127;
        const uint32_t nbytes = (nw + 1) / 2;
        if (1 + nbytes > n) return false;
        for (uint32_t i = 0; i < nw; i++) w[i] = (i & 1) ? (p[1 + i / 2] & 15) : (p[1 + i / 2] >> 4);
        used = 1 + nbytes;
    } else {           // FSE-compressed, two interleaved states
        if (1 + hb > n) return false;
        int log = 0, nsym = 0;
        uint32_t u = 0;
        if (!fse_read_ncount(p + 1, hb, Z_WT_LOG, 255, T.hnorm, log, nsym, u)) return false;
        if (!fse_build(T.hnorm, nsym, log, T.wt, T.hnext, K_WT)) return false;
        BitR b;
        if (!br_init(b, p + 1 + u, hb - u)) return false;
        uint32_t s1 = br_read(b, uint32_t(log)), s2 = br_read(b, uint32_t(log));
        for (;;) {
            if (nw > 253) return false;
            w[nw++] = T.wt[s1].sym;
            s1 = T.wt[s1].next + br_read(b, T.wt[s1].nb);
            if (b.pos < 0) { w[nw++] = T.wt[s2].sym; break; }
            if (nw > 253) return false;
            w[nw++] = T.wt[s2].sym;
            s2 = T.wt[s2].next + br_read(b, T.wt[s2].nb);
            if (b.pos < 0) { w[nw++] = T.wt[s1].sym; break; }
        }
        used = 1 + hb;
    }
    uint32_t total = 0;
    for (int k = 0; k < 16; k++) T.rank[k] = 0;
    for (uint32_t i = 0; i < nw; i++) {
        if (w[i] > Z_HUF_LOG + 1) return false;
        T.rank[w[i]]++;
        total += (1u << w[i]) >> 1;
    }
    if (total == 0) return false;
    const uint32_t log = hibit(total) + 1;
    if (log > uint32_t(Z_HUF_LOG)) return false;
    const uint32_t rest = (1u << log) - total;
    if (rest & (rest - 1)) return false;   // the last weight completes a power of two
    const uint32_t last = hibit(rest) + 1;
    w[nw++] = uint8_t(last);
    T.rank[last]++;
    if (T.rank[1] < 2 || (T.rank[1] & 1)) return false;
    uint32_t acc = 0;
    for (uint32_t k = 1; k <= log; k++) { T.start[k] = acc; acc += T.rank[k] << (k - 1); }
    for (uint32_t s = 0; s < nw; s++) {
        const uint32_t k = w[s];
        if (!k) continue;
        const uint32_t cells = 1u << (k - 1), at = T.start[k];
        for (uint32_t q = 0; q < cells; q++) T.huf[at + q] = HufEnt{uint8_t(s), uint8_t(log + 1 - k)};
        T.start[k] = at + cells;
    }
    T.huf_log = uint8_t(log);
    return true;
}

// Which of its two decoders libzstd builds for a Huffman table, from the sizes of the literals
// section that brings the table (its HUF_selectDecoder: a cost per table and per 256 symbols for
// the one-symbol and the two-symbol decoder, by compressed / regenerated size in sixteenths). It
// matters only to a stream that runs out (huf_stream).
PF_HD inline bool huf_pairs_for(uint32_t regen, uint32_t csize) {
    const uint32_t q = csize >= regen ? 15u : csize * 16u / regen, d256 = regen >> 8;
    const uint32_t t1 = q < 2 ? 0 : q == 2 ? 150 : q == 3 ? 170 : q == 4 ? 177 : q == 5 ? 197 : q == 6 ? 221 : q == 7 ? 256 : q == 8 ? 359
                      : q == 9 ? 582 : q == 10 ? 688 : q == 11 ? 825 : q == 12 ? 976 : q == 13 ? 1180 : q == 14 ? 1377 : 1412;
    const uint32_t s1 = q < 2 ? 0 : q == 2 ? 216 : q == 3 ? 205 : q == 4 ? 199 : q == 5 ? 194 : q == 6 ? 192 : q == 7 ? 189 : q == 8 ? 188
                      : q == 9 ? 187 : q == 10 ? 187 : q == 11 ? 186 : q == 12 ? 185 : q == 13 ? 186 : 185;
    const uint32_t t2 = q < 2 ? 1 : q == 2 ? 381 : q == 3 ? 514 : q == 4 ? 539 : q == 5 ? 644 : q == 6 ? 735 : q == 7 ? 881 : q == 8 ? 1167
                      : q == 9 ? 1570 : q == 10 ? 1712 : q == 11 ? 1965 : q == 12 ? 2131 : q == 13 ? 2070 : q == 14 ? 1731 : 1695;
    const uint32_t s2 = q < 2 ? 1 : q == 2 ? 119 : q == 3 ? 112 : q == 4 ? 110 : q == 5 ? 107 : q == 6 ? 107 : q == 7 ? 106 : q == 8 ? 109
                      : q == 9 ? 114 : q == 10 ? 122 : q == 11 ? 136 : q == 12 ? 150 : q == 13 ? 175 : 202;
    const uint32_t one = t1 + s1 * d256, two = t2 + s2 * d256;
    return two + (two >> 5) < one;
}

// One Huffman stream of `count` symbols. strict: the stream must then be exactly used up. Not strict
// (four streams of >= 8 bytes each, where libzstd's decoder makes no such check): bits left over are
// ignored, and a stream that runs out goes on into the `lo` bytes that lie before it, then zeros.
// pairs: two symbols whose codes fit one 11-bit lookup are taken together, as libzstd's two-symbol
// decoder does; it differs from one at a time only where a stream runs out inside such a pair.
PF_HD inline bool huf_stream(const HufEnt* t, uint32_t log, const uint8_t* p, uint32_t len, uint32_t lo, bool strict, bool pairs,
                             uint8_t* out, uint32_t count) {
    BitR b;
    if (strict) {
        if (!br_init(b, p, len)) return false;
    } else {   // (libzstd takes a last byte of 0 as eight data bits there)
        b.p = p; b.len = len; b.lo = lo;
        b.pos = int64_t(len - 1) * 8 + (p[len - 1] ? hibit(p[len - 1]) : 8);
        br_refill(b);
    }
    const int64_t floor_pos = -8 * int64_t(lo);
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t w = br_peek(b, Z_HUF_LOG);
        const HufEnt e = t[w >> (uint32_t(Z_HUF_LOG) - log)];
        uint32_t nb = e.nb;
        out[i] = e.sym;
        if (pairs && !strict && i + 1 < count) {
            const HufEnt e2 = t[((w << nb) & ((1u << Z_HUF_LOG) - 1)) >> (uint32_t(Z_HUF_LOG) - log)];
            if (nb + e2.nb <= uint32_t(Z_HUF_LOG)) {
                out[++i] = e2.sym;
                nb += e2.nb;
            }
        }
        br_skip(b, nb);
        if (strict && b.pos < 0) return false;
        if (!strict && b.pos <= floor_pos) { b.pos += 64; br_refill(b); }   // its last 64-bit window, again
    }
    return !strict || b.pos == 0;
}

// ---- frame and block headers ----
struct FrameHdr {
    uint32_t hdr;          // bytes to step over: the header, or the whole skippable frame
    uint32_t block_max;    // min(window, 128 KiB): the most a compressed block may hold
    uint64_t fcs;
    uint8_t has_fcs, checksum, skippable;
};
PF_HD inline uint32_t le32(const uint8_t* p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24; }
PF_HD inline bool frame_header(const uint8_t* p, uint64_t n, FrameHdr& h) {
    h = FrameHdr{};
    if (n < 4) return false;
    const uint32_t magic = le32(p);
    if ((magic & 0xfffffff0u) == 0x184d2a50u) {
        if (n < 8) return false;
        const uint64_t sz = le32(p + 4);
        if (sz > n - 8) return false;
        h.skippable = 1;
        h.hdr = uint32_t(8 + sz);
        return true;
    }
    if (magic != 0xfd2fb528u || n < 5) return false;
    const uint32_t d = p[4];
    const uint32_t fcs_flag = d >> 6, single = (d >> 5) & 1, did_flag = d & 3;
    if (d & 8) return false;   // reserved bit
    h.checksum = (d >> 2) & 1;
    const uint32_t did_len = did_flag == 3 ? 4 : did_flag;
    const uint32_t fcs_len = fcs_flag == 0 ? single : (1u << fcs_flag);
    const uint32_t need = 5 + (single ? 0 : 1) + did_len + fcs_len;
    if (n < need) return false;
    uint32_t at = 5;
    uint64_t window = 0;
    if (!single) {
        const uint32_t wd = p[at++], wlog = 10 + (wd >> 3);
        if (wlog > uint32_t(Z_WINDOW_LOG_MAX)) return false;
        window = (uint64_t(1) << wlog) + ((uint64_t(1) << wlog) >> 3) * (wd & 7);
    }
    uint32_t did = 0;
    for (uint32_t k = 0; k < did_len; k++) did |= uint32_t(p[at++]) << (8 * k);
    if (did != 0) return false;   // dictionaries are out of scope
    uint64_t fcs = 0;
    for (uint32_t k = 0; k < fcs_len; k++) fcs |= uint64_t(p[at++]) << (8 * k);
    if (fcs_len == 2) fcs += 256;
    h.has_fcs = fcs_len > 0;
    h.fcs = fcs;
    if (single) window = fcs;
    h.block_max = uint32_t(window < Z_BLOCK_MAX ? window : Z_BLOCK_MAX);
    h.hdr = need;
    return true;
}
PF_HD inline void frame_begin(Tables& T) {
    T.rep[0] = 1; T.rep[1] = 4; T.rep[2] = 8;
    T.fse_ok = 0;
    T.huf_ok = 0;
}

struct BlockHdr {
    uint32_t last, type, size;   // type 0 raw, 1 RLE, 2 compressed; size: the Block_Size field
    uint32_t src;                // bytes of the block in the input
};
// Header of the block at p[0 .. n); out_left: bytes the destination still takes.
PF_HD inline bool block_header(const uint8_t* p, uint64_t n, const FrameHdr& fh, uint64_t out_left, BlockHdr& b) {
    if (n < 3) return false;
    const uint32_t v = uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16;
    b.last = v & 1;
    b.type = (v >> 1) & 3;
    b.size = v >> 3;
    if (b.type == 3 || b.size > Z_BLOCK_MAX) return false;
    b.src = b.type == 1 ? 1 : b.size;
    if (b.src > n - 3) return false;
    if (b.type == 2) return b.size <= fh.block_max && b.size >= 2;
    return b.size <= out_left;
}

// ---- literals section ----
struct LitHdr {
    uint32_t type;      // 0 raw, 1 RLE, 2 Huffman, 3 Huffman with the previous table
    uint32_t regen;     // literals
    uint32_t csize;     // Huffman: tree description + streams
    uint32_t streams;   // 1 or 4
    uint32_t hdr;       // header bytes
    uint32_t total;     // bytes of the whole section
};
// out_cap: the most literals the block may still produce.
PF_HD inline bool lit_header(const uint8_t* p, uint32_t n, uint32_t out_cap, bool huf_ok, LitHdr& h) {
    if (n < 1) return false;
    const uint32_t b0 = p[0], sf = (b0 >> 2) & 3;
    h.type = b0 & 3;
    h.csize = 0;
    h.streams = 1;
    if (h.type < 2) {
        h.hdr = sf == 1 ? 2 : sf == 3 ? 3 : 1;
        if (h.hdr > n) return false;
        h.regen = h.hdr == 1 ? b0 >> 3 : h.hdr == 2 ? (b0 >> 4) | uint32_t(p[1]) << 4 : (b0 >> 4) | uint32_t(p[1]) << 4 | uint32_t(p[2]) << 12;
        h.total = h.hdr + (h.type == 0 ? h.regen : 1);
    } else {
        if (n < 5) return false;
        if (h.type == 3 && !huf_ok) return false;
        h.hdr = sf < 2 ? 3 : sf + 2;
        const uint64_t v = uint64_t(le32(p)) | uint64_t(p[4]) << 32;
        const uint32_t w = sf < 2 ? 10 : sf == 2 ? 14 : 18;
        h.regen = uint32_t(v >> 4) & ((1u << w) - 1);
        h.csize = uint32_t(v >> (4 + w)) & ((1u << w) - 1);
        h.streams = sf == 0 ? 1 : 4;
        if (h.streams == 4 && h.regen < 6) return false;
        h.total = h.hdr + h.csize;
    }
    return h.total <= n && h.regen <= Z_BLOCK_MAX && h.regen <= out_cap;
}

// The 1 or 4 streams of Huffman literals at p[0 .. n) (after the tree description).
struct LitStreams {
    uint32_t off[4], len[4], out[4], cnt[4];
    uint32_t strict;
};
PF_HD inline bool lit_streams(const uint8_t* p, uint32_t n, const LitHdr& h, LitStreams& s) {
    if (h.streams == 1) {
        s.off[0] = 0; s.len[0] = n; s.out[0] = 0; s.cnt[0] = h.regen;
        s.strict = 1;
        return n >= 1;
    }
    if (n < 10) return false;
    const uint32_t l1 = p[0] | uint32_t(p[1]) << 8, l2 = p[2] | uint32_t(p[3]) << 8, l3 = p[4] | uint32_t(p[5]) << 8;
    if (6 + l1 + l2 + l3 > n) return false;
    const uint32_t seg = (h.regen + 3) / 4;
    if (3 * seg > h.regen) return false;
    s.off[0] = 6; s.len[0] = l1;
    s.off[1] = 6 + l1; s.len[1] = l2;
    s.off[2] = 6 + l1 + l2; s.len[2] = l3;
    s.off[3] = 6 + l1 + l2 + l3; s.len[3] = n - s.off[3];
    s.strict = 0;
    for (int k = 0; k < 4; k++) {
        s.out[k] = uint32_t(k) * seg;
        s.cnt[k] = k < 3 ? seg : h.regen - 3 * seg;
        if (s.len[k] < 8) s.strict = 1;
    }
    return true;
}

// ---- sequences section ----
struct SeqHdr {
    uint32_t nseq;
    uint32_t bits_off;   // where the bitstream starts within the section
};
PF_HD inline bool seq_table(int mode, const uint8_t* p, uint32_t n, uint32_t& at, int kind, Tables& T) {
    Ent* t = kind == K_LL ? T.ll : kind == K_OF ? T.of : T.ml;
    uint8_t& tlog = kind == K_LL ? T.ll_log : kind == K_OF ? T.of_log : T.ml_log;
    const int max_sym = kind == K_LL ? Z_LL_MAX : kind == K_OF ? Z_OF_MAX : Z_ML_MAX;
    const int max_log = kind == K_LL ? Z_LL_LOG : kind == K_OF ? Z_OF_LOG : Z_ML_LOG;
    if (mode == 3) return T.fse_ok != 0;   // repeat: the table of the last block that had sequences
    if (mode == 1) {
        if (at >= n || p[at] > max_sym) return false;
        t[0] = Ent{0, 0, p[at], code_base(kind, p[at])};
        tlog = 0;
        at++;
        return true;
    }
    int log = 0, nsym = 0;
    if (mode == 0) {
        nsym = max_sym + 1;
        if (kind == K_OF) nsym = 29;
        log = kind == K_OF ? 5 : 6;
        for (int s = 0; s < nsym; s++) T.snorm[s] = int16_t(kind == K_LL ? ll_default(s) : kind == K_OF ? of_default(s) : ml_default(s));
    } else {
        uint32_t u = 0;
        if (at >= n || !fse_read_ncount(p + at, n - at, max_log, max_sym, T.snorm, log, nsym, u)) return false;
        at += u;
    }
    if (!fse_build(T.snorm, nsym, log, t, T.snext, kind)) return false;
    tlog = uint8_t(log);
    return true;
}
// Section header and the three tables. nseq == 0: the section is its header alone.
PF_HD inline bool seq_header(const uint8_t* p, uint32_t n, Tables& T, SeqHdr& h) {
    if (n < 1) return false;
    uint32_t at = 1, ns = p[0];
    if (ns >= 128) {
        if (ns == 255) {
            if (n < 3) return false;
            ns = (p[1] | uint32_t(p[2]) << 8) + 0x7f00;
            at = 3;
        } else {
            if (n < 2) return false;
            ns = ((ns - 128) << 8) + p[1];
            at = 2;
        }
    }
    h.nseq = ns;
    h.bits_off = at;
    if (ns == 0) return at == n;
    if (at >= n) return false;
    const uint32_t modes = p[at++];
    if (modes & 3) return false;   // reserved bits
    if (!seq_table(int(modes >> 6), p, n, at, K_LL, T)) return false;
    if (!seq_table(int(modes >> 4) & 3, p, n, at, K_OF, T)) return false;
    if (!seq_table(int(modes >> 2) & 3, p, n, at, K_ML, T)) return false;
    T.fse_ok = 1;
    h.bits_off = at;
    return at < n;
}

struct SeqDec {
    BitR b;
    uint32_t sl, so, sm;
};
struct Seq {
    uint32_t ll, ml, off;
};
PF_HD inline bool seq_init(SeqDec& d, const Tables& T, const uint8_t* p, uint32_t len) {
    if (!br_init(d.b, p, len)) return false;
    d.sl = br_read(d.b, T.ll_log);
    d.so = br_read(d.b, T.of_log);
    d.sm = br_read(d.b, T.ml_log);
    return true;
}
// The next sequence; updates T.rep. last: no state update follows, and the stream must be used up.
PF_HD inline bool seq_next(SeqDec& d, Tables& T, bool last, Seq& s) {
    const Ent le = T.ll[d.sl], oe = T.of[d.so], me = T.ml[d.sm];
    const uint32_t ov = oe.base + br_read(d.b, oe.sym);
    s.ml = me.base + br_read(d.b, ml_bits(me.sym));
    s.ll = le.base + br_read(d.b, ll_bits(le.sym));
    uint32_t* rep = T.rep;
    if (ov > 3) {
        s.off = ov - 3;
        rep[2] = rep[1]; rep[1] = rep[0]; rep[0] = s.off;
    } else {
        const uint32_t idx = ov - 1 + (s.ll == 0 ? 1 : 0);
        if (idx == 0) {
            s.off = rep[0];
        } else {
            s.off = idx == 3 ? rep[0] - 1 : rep[idx];
            if (s.off == 0) return false;
            if (idx >= 2) rep[2] = rep[1];
            rep[1] = rep[0];
            rep[0] = s.off;
        }
    }
    if (last) return d.b.pos == 0;
    d.sl = le.next + br_read(d.b, le.nb);
    d.sm = me.next + br_read(d.b, me.nb);
    d.so = oe.next + br_read(d.b, oe.nb);
    return true;
}
// May this sequence run? lit_left: literals not yet used; block_out: bytes the block has produced;
// frame_out: bytes the frame had produced before the block; out_left: room left in the destination.
PF_HD inline bool seq_check(const Seq& s, uint32_t lit_left, uint32_t block_out, uint64_t frame_out, uint64_t out_left) {
    if (s.ll > lit_left) return false;
    const uint64_t n = uint64_t(s.ll) + s.ml;
    if (n > out_left || block_out + n > Z_BLOCK_MAX) return false;
    return s.off <= frame_out + block_out + s.ll;
}
PF_HD inline bool tail_check(uint32_t lit_left, uint32_t block_out, uint64_t out_left) {
    return lit_left <= out_left && uint64_t(block_out) + lit_left <= Z_BLOCK_MAX;
}

#ifndef __HIP_DEVICE_COMPILE__
// ---- the host model: one serial decoder over the core ----
// lit: Z_BLOCK_MAX bytes of work area. Decodes every frame of src into dst[0 .. cap).
inline int decompress_host(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, Tables& T, uint8_t* lit) {
    size_t ip = 0, op = 0;
    while (ip < n) {
        FrameHdr fh;
        if (!frame_header(src + ip, n - ip, fh)) return Z_CORRUPT;
        ip += fh.hdr;
        if (fh.skippable) continue;
        frame_begin(T);
        const size_t f0 = op;
        for (;;) {
            BlockHdr bh;
            if (!block_header(src + ip, n - ip, fh, cap - op, bh)) return Z_CORRUPT;
            ip += 3;
            const uint8_t* p = src + ip;
            if (bh.type == 0) {
                for (uint32_t i = 0; i < bh.size; i++) dst[op + i] = p[i];
                op += bh.size;
            } else if (bh.type == 1) {
                for (uint32_t i = 0; i < bh.size; i++) dst[op + i] = p[0];
                op += bh.size;
            } else {
                const uint64_t left = cap - op;
                LitHdr lh;
                if (!lit_header(p, bh.size, uint32_t(left < Z_BLOCK_MAX ? left : Z_BLOCK_MAX), T.huf_ok, lh)) return Z_CORRUPT;
                const uint8_t* lits = p + lh.hdr;   // raw
                if (lh.type >= 2) {
                    uint32_t used = 0;
                    if (lh.type == 2) {
                        if (!huf_read(p + lh.hdr, lh.csize, T, used)) return Z_CORRUPT;
                        T.huf_ok = 1;
                        T.huf_pairs = huf_pairs_for(lh.regen, lh.csize);
                    }
                    LitStreams ls;
                    if (!lit_streams(p + lh.hdr + used, lh.csize - used, lh, ls)) return Z_CORRUPT;
                    for (uint32_t k = 0; k < lh.streams; k++)
                        if (!huf_stream(T.huf, T.huf_log, p + lh.hdr + used + ls.off[k], ls.len[k], ls.off[k], ls.strict != 0, T.huf_pairs != 0,
                                        lit + ls.out[k], ls.cnt[k]))
                            return Z_CORRUPT;
                    lits = lit;
                }
                const uint8_t* sp = p + lh.total;
                const uint32_t sn = bh.size - lh.total;
                SeqHdr sh;
                if (!seq_header(sp, sn, T, sh)) return Z_CORRUPT;
                uint32_t lp = 0, bo = 0;
                if (sh.nseq) {
                    SeqDec d;
                    if (!seq_init(d, T, sp + sh.bits_off, sn - sh.bits_off)) return Z_CORRUPT;
                    for (uint32_t i = 0; i < sh.nseq; i++) {
                        Seq s;
                        if (!seq_next(d, T, i + 1 == sh.nseq, s)) return Z_CORRUPT;
                        if (!seq_check(s, lh.regen - lp, bo, op - f0, left - bo)) return Z_CORRUPT;
                        uint8_t* o = dst + op + bo;
                        for (uint32_t j = 0; j < s.ll; j++) o[j] = lh.type == 1 ? lits[0] : lits[lp + j];
                        o += s.ll;
                        for (uint32_t j = 0; j < s.ml; j++) o[j] = o[int64_t(j) - int64_t(s.off)];
                        lp += s.ll;
                        bo += s.ll + s.ml;
                    }
                }
                const uint32_t tail = lh.regen - lp;
                if (!tail_check(tail, bo, left - bo)) return Z_CORRUPT;
                for (uint32_t j = 0; j < tail; j++) dst[op + bo + j] = lh.type == 1 ? lits[0] : lits[lp + j];
                op += bo + tail;
            }
            ip += bh.src;
            if (bh.last) break;
        }
        if (fh.has_fcs && uint64_t(op - f0) != fh.fcs) return Z_CORRUPT;
        if (fh.checksum) {
            if (n - ip < 4) return Z_CORRUPT;
            ip += 4;   // consumed, not verified
        }
    }
    *out_len = op;
    return Z_OK;
}
#endif

}  // namespace zstd
}  // namespace pf
