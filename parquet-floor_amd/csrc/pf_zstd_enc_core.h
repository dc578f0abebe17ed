// pf_zstd_enc_core.h — Zstandard (RFC 8878) encode core shared by the host model (compress_host) and
// the GPU kernel (pf_zstd_enc.hip). Plain C++ over pf_zstd_core.h: the predefined distributions and the
// code baselines are the decode core's arithmetic, and the encoding tables are read off the decode
// tables fse_build makes, so encoder and decoder cannot disagree about a cell.
//
// One job (<= ZE_BLOCK bytes) becomes one block: RLE when all bytes are equal, else a compressed
// block, else (not strictly smaller) raw. A compressed block is
//   literals   raw | RLE | Huffman (1 stream up to 1023 literals, 4 above), lengths <= 11, Kraft sum 1,
//              the tree as direct 4-bit weights or FSE-compressed weights, whichever is shorter;
//   sequences  the three predefined tables, real offsets (value = offset + 3) and repeat offset 1
//              (value 1) once the job has written a real offset of its own (repeat offsets outlive a
//              block, and a job does not know what the blocks before it left there).
//
// Who runs what: functions with (lane, nl) arguments split their work over nl lanes and write disjoint
// cells or order-independent ORs / adds (or32 / add32: LDS atomics on the device), so the kernel calls
// them with (lane, 64) between barriers and the host model with (0, 1). Everything else is serial: one
// lane on the device, the same code on the host. The match finder alone is written twice, with the
// wave's ballots in the kernel and restated lane by lane in find_matches_host.
#pragma once
#include "pf_zstd_core.h"

namespace pf {
namespace zstd {

constexpr uint32_t ZE_BLOCK = 8192;               // bytes of one job = one block (ZC_BLOCK, pf_encode.h)
constexpr uint32_t ZE_HBITS = 12;                 // match table: last position (+1) of a 4-byte prefix hash
// A sequence costs about 21 bits under the predefined tables, a Huffman literal about 5: matches of 4 bytes
// are left to the literals (sizes at 4, 5 and 6 in DESIGN 4.31).
constexpr uint32_t ZE_MIN_MATCH = 5;
constexpr uint32_t ZE_SEQ_MAX = ZE_BLOCK / ZE_MIN_MATCH + 1;   // matches do not overlap
constexpr uint32_t ZE_HUF_MAX = 11;               // longest Huffman code
constexpr uint32_t ZE_LANES = 64;
constexpr uint32_t ZE_NONE = 0xffffffffu;
static_assert(ZE_MIN_MATCH >= 4 && ZE_BLOCK <= Z_BLOCK_MAX && ZE_BLOCK <= 65535, "positions and lengths are kept in 16 bits");

PF_HD inline void or32(uint32_t* p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicOr(p, v);
#else
    *p |= v;
#endif
}
PF_HD inline void add32(uint32_t* p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

// One FSE encoding table: the cells of symbol s in index order are cell[cum[s] .. cum[s] + cnt[s]); the
// r-th of them is the decoder's state with ns = cnt[s] + r (fse_build).
struct EncFse {
    uint8_t cell[64];
    uint8_t cnt[56], cum[56];
    uint32_t log;
};
// Scratch of one table build (the decode table it is read off).
struct __attribute__((may_alias)) EncFseScratch {
    Ent t[64];
    uint16_t next[56];
    int16_t norm[56];
};

PF_HD inline bool fse_enc_build(const int16_t* norm, int nsym, int log, EncFse& e, EncFseScratch& s) {
    if (!fse_build(norm, nsym, log, s.t, s.next, K_WT)) return false;
    uint32_t acc = 0;
    for (int k = 0; k < nsym; k++) {
        const uint32_t c = norm[k] < 0 ? 1u : uint32_t(norm[k]);
        e.cnt[k] = uint8_t(c);
        e.cum[k] = uint8_t(acc);
        acc += c;
    }
    const uint32_t size = 1u << log;
    for (uint32_t u = 0; u < size; u++) {
        const uint32_t k = s.t[u].sym, ns = (uint32_t(s.t[u].next) + size) >> s.t[u].nb;
        e.cell[e.cum[k] + ns - e.cnt[k]] = uint8_t(u);
    }
    e.log = uint32_t(log);
    return true;
}
PF_HD inline bool fse_enc_predefined(int kind, EncFse& e, EncFseScratch& s) {
    const int nsym = kind == K_LL ? Z_LL_MAX + 1 : kind == K_OF ? 29 : Z_ML_MAX + 1;
    for (int k = 0; k < nsym; k++) s.norm[k] = int16_t(kind == K_LL ? ll_default(k) : kind == K_OF ? of_default(k) : ml_default(k));
    return fse_enc_build(s.norm, nsym, kind == K_OF ? 5 : 6, e, s);
}
// The state a stream ends in (the decoder's first): the symbol's cell that takes the most bits.
PF_HD inline uint32_t fse_enc_init(const EncFse& e, uint32_t sym) { return e.cell[e.cum[sym]]; }
// The decoder is in state `cs` after symbol `sym`: the cell it was in before, and the bits it read.
PF_HD inline uint32_t fse_enc_step(const EncFse& e, uint32_t sym, uint32_t cs, uint32_t& bits, uint32_t& nb) {
    const uint32_t size = 1u << e.log, c = e.cnt[sym], x = cs + size;
    nb = e.log - hibit(c);
    if ((x >> nb) < c) nb--;
    bits = x & ((1u << nb) - 1u);
    return e.cell[e.cum[sym] + (x >> nb) - c];
}

// Forward bit writer (low bits first) into p[0 .. cap); a backward stream is the same bits closed with
// the end mark. ovf: bytes past cap were dropped.
struct BitW {
    uint8_t* p;
    uint32_t cap, at, n;
    uint64_t acc;
    bool ovf;
};
PF_HD inline void bw_init(BitW& b, uint8_t* p, uint32_t cap) { b.p = p; b.cap = cap; b.at = 0; b.n = 0; b.acc = 0; b.ovf = false; }
PF_HD inline void bw_add(BitW& b, uint32_t v, uint32_t k) {   // k <= 32, v < 2^k
    b.acc |= uint64_t(v) << b.n;
    b.n += k;
    while (b.n >= 8) {
        if (b.at < b.cap) b.p[b.at] = uint8_t(b.acc); else b.ovf = true;
        b.at++;
        b.acc >>= 8;
        b.n -= 8;
    }
}
PF_HD inline void bw_flush(BitW& b) {
    if (b.n) bw_add(b, 0, 8 - b.n);
}
PF_HD inline void bw_close(BitW& b) {   // the end mark: the highest set bit of the last byte
    bw_add(b, 1, 1);
    bw_flush(b);
}

// ---- sequence codes: the inverse of ll_base / ml_base ----
PF_HD inline uint32_t ll_code(uint32_t v, uint32_t& base) {
    if (v < 16) { base = v; return v; }
    uint32_t c = 16, b = 16;
    while (b + (1u << ll_bits(c)) <= v) { b += 1u << ll_bits(c); c++; }
    base = b;
    return c;
}
PF_HD inline uint32_t ml_code(uint32_t v, uint32_t& base) {   // v >= 3
    if (v < 35) { base = v; return v - 3; }
    uint32_t c = 32, b = 35;
    while (b + (1u << ml_bits(c)) <= v) { b += 1u << ml_bits(c); c++; }
    base = b;
    return c;
}

// ---- the work area of one job (LDS on the device) ----
struct __attribute__((may_alias)) HufWork {
    uint32_t hist[256];
    uint16_t node[256];        // weights of the internal nodes
    uint16_t parent[512];      // then the depths
    uint16_t code[256];
    uint8_t order[256];        // present symbols by (count, symbol)
    uint8_t clen[256];
    uint8_t weights[256];
    uint8_t tree[132];         // the tree description
    uint16_t lanebits[4 * ZE_LANES];   // bits of a lane's symbols, per stream
    uint32_t ndist, maxsym, maxlen, tree_len, tree_fse;
    EncFse fwt;
    EncFseScratch fs;          // the weights' table build
};
struct LitPlan {
    uint32_t type;             // 0 raw, 1 RLE, 2 Huffman
    uint32_t streams, hdr, total;
    uint32_t cnt[4], bits[4], bytes[4];
    uint32_t bit0[4];          // Huffman: where a stream's bits start in the block
};
// Areas that are dead after a phase are used again: the job's bytes give way to the assembled block, the
// match table to the sequences section (its first ZE_BLOCK bytes: a longer one means a raw block anyway)
// and the Huffman work (the rest), and the literals' area holds the scratch of the three predefined
// tables' builds before the first literal is written.
struct EncWork {
    uint32_t amem[(ZE_BLOCK + 16) / 4];   // the job's bytes (+ 16 zeros); later the assembled block
    uint32_t tab[1u << ZE_HBITS];         // the match table; later the sequences section and the Huffman work
    uint32_t litmem[ZE_BLOCK / 4];        // the literals
    uint16_t sll[ZE_SEQ_MAX], sml[ZE_SEQ_MAX], sof[ZE_SEQ_MAX];
    EncFse fll, fof, fml;
    LitPlan lp;
    uint32_t nseq, nlit, seq_bytes, reps, btype, bsize;
    uint32_t seq_lane[ZE_LANES];   // bits of a lane's sequences
    uint32_t seq_fin[3];           // the states the stream opens with: LL, OF, ML
    uint32_t seq_at, seq_bits;     // bytes of the section's head; bits of all sequences
};
static_assert(3 * ZE_SEQ_MAX <= ZE_BLOCK, "the sequences' code bytes lie in the job's dead bytes");
constexpr uint32_t ZE_SEQ_CAP = ZE_BLOCK;   // bytes of the sequences section's area
static_assert(ZE_SEQ_CAP + sizeof(HufWork) <= (4u << ZE_HBITS), "the Huffman work lies behind the sequences section");
static_assert(3 * sizeof(EncFseScratch) <= ZE_BLOCK, "the predefined tables' scratch lies in the literals' area");
PF_HD inline uint8_t* ew_buf(EncWork& W) { return reinterpret_cast<uint8_t*>(W.amem); }
PF_HD inline uint8_t* ew_seq(EncWork& W) { return reinterpret_cast<uint8_t*>(W.tab); }
PF_HD inline uint8_t* ew_lit(EncWork& W) { return reinterpret_cast<uint8_t*>(W.litmem); }
PF_HD inline HufWork& ew_huf(EncWork& W) { return *reinterpret_cast<HufWork*>(W.tab + ZE_SEQ_CAP / 4); }
PF_HD inline EncFseScratch& ew_fs(EncWork& W, int k) { return reinterpret_cast<EncFseScratch*>(W.litmem)[k]; }

PF_HD inline uint32_t ze_hash(uint32_t v) { return (v * 0x1e35a7bdu) >> (32 - ZE_HBITS); }
PF_HD inline uint32_t ze_ld32(const uint8_t* b, uint32_t p) {
    return uint32_t(b[p]) | uint32_t(b[p + 1]) << 8 | uint32_t(b[p + 2]) << 16 | uint32_t(b[p + 3]) << 24;
}

// ---- Huffman ----
// Histogram of the literals (hist zeroed before).
PF_HD inline void huf_hist(EncWork& W, uint32_t lane, uint32_t nl) {
    for (uint32_t i = lane; i < W.nlit; i += nl) add32(&ew_huf(W).hist[ew_lit(W)[i]], 1u);
}
// Rank sort of the present symbols by (count, symbol); ndist (zeroed before) counts them.
PF_HD inline void huf_sort(EncWork& W, uint32_t lane, uint32_t nl) {
    HufWork& h = ew_huf(W);
    for (uint32_t s = lane; s < 256; s += nl) {
        const uint32_t c = h.hist[s];
        if (!c) continue;
        uint32_t r = 0;
        for (uint32_t t = 0; t < 256; t++) {
            const uint32_t ct = h.hist[t];
            r += (ct != 0 && (ct < c || (ct == c && t < s))) ? 1u : 0u;
        }
        h.order[r] = uint8_t(s);
        add32(&h.ndist, 1u);
    }
}

// FSE-compressed weights of h.weights[0 .. nw) into dst[0 .. 128): the header byte and the description.
// 0: not possible (one distinct weight, or 128 bytes and more).
PF_HD inline uint32_t huf_weights_fse(EncWork& W, uint32_t nw, uint8_t* dst) {
    HufWork& h = ew_huf(W);
    EncFseScratch& s = h.fs;
    uint32_t cnt[13];
    for (int k = 0; k < 13; k++) cnt[k] = 0;
    for (uint32_t i = 0; i < nw; i++) cnt[h.weights[i]]++;
    int maxw = 0, big = 0;
    for (int k = 0; k < 13; k++) {
        if (cnt[k]) maxw = k;
        if (cnt[k] > cnt[big]) big = k;
    }
    if (nw < 2 || cnt[big] == nw) return 0;
    // normalised counts, sum 64, every present weight >= 1
    const int log = Z_WT_LOG, size = 1 << log;
    int sum = 0;
    for (int k = 0; k <= maxw; k++) {
        int v = cnt[k] ? int(cnt[k] * uint32_t(size) / nw) : 0;
        if (cnt[k] && v < 1) v = 1;
        s.norm[k] = int16_t(v);
        sum += v;
    }
    while (sum > size) {
        int at = 0;
        for (int k = 1; k <= maxw; k++)
            if (s.norm[k] > s.norm[at]) at = k;
        s.norm[at]--;
        sum--;
    }
    s.norm[big] = int16_t(s.norm[big] + (size - sum));
    if (!fse_enc_build(s.norm, maxw + 1, log, h.fwt, s)) return 0;
    // the table description (fse_read_ncount's mirror)
    BitW b;
    bw_init(b, dst + 1, 127);
    bw_add(b, uint32_t(log - 5), 4);
    int remaining = size, k = 0;
    while (remaining > 0) {
        const uint32_t nb = hibit(uint32_t(remaining) + 1) + 1;
        const uint32_t lower = (1u << (nb - 1)) - 1, thr = (1u << nb) - 1 - (uint32_t(remaining) + 1);
        const uint32_t val = uint32_t(s.norm[k]) + 1;
        if (val < thr) bw_add(b, val, nb - 1);
        else bw_add(b, val > lower ? val + thr : val, nb);
        remaining -= s.norm[k];
        const bool zero = s.norm[k] == 0;
        k++;
        if (zero) {   // how many more zeros follow, two bits at a time
            int run = 0;
            while (k + run <= maxw && s.norm[k + run] == 0) run++;
            k += run;
            while (run >= 3) { bw_add(b, 3, 2); run -= 3; }
            bw_add(b, uint32_t(run), 2);
        }
    }
    bw_flush(b);
    if (b.ovf) return 0;
    const uint32_t nc = b.at;
    // two interleaved states: the decoder takes even weights from the first, odd ones from the second,
    // and the last two come out of the states the stream opens with
    BitW w;
    bw_init(w, dst + 1 + nc, 127 - nc);
    uint32_t st[2];
    st[(nw - 1) & 1] = fse_enc_init(h.fwt, h.weights[nw - 1]);
    st[(nw - 2) & 1] = fse_enc_init(h.fwt, h.weights[nw - 2]);
    for (uint32_t i = nw - 2; i-- > 0;) {
        uint32_t bits, nb;
        st[i & 1] = fse_enc_step(h.fwt, h.weights[i], st[i & 1], bits, nb);
        bw_add(w, bits, nb);
    }
    bw_add(w, st[1], uint32_t(log));
    bw_add(w, st[0], uint32_t(log));
    bw_close(w);
    if (w.ovf || nc + w.at > 127) return 0;
    dst[0] = uint8_t(nc + w.at);
    return 1 + nc + w.at;
}

// Code lengths (<= 11, Kraft sum exactly 1), codes, weights and the tree description for h.hist,
// after huf_sort. tree_len == 0: no description is possible and the literals stay raw.
PF_HD inline void huf_build(EncWork& W) {
    HufWork& h = ew_huf(W);
    const uint32_t n = h.ndist;
    h.tree_len = 0;
    h.tree_fse = 0;
    if (n < 2) return;
    // the standard build over the sorted leaves: two queues, a leaf before a node of equal weight
    uint32_t li = 0, ni = 0;
    for (uint32_t j = 0; j + 1 < n; j++) {
        uint32_t wsum = 0;
        for (int k = 0; k < 2; k++) {
            if (li < n && (ni >= j || h.hist[h.order[li]] <= h.node[ni])) {
                wsum += h.hist[h.order[li]];
                h.parent[li++] = uint16_t(n + j);
            } else {
                wsum += h.node[ni];
                h.parent[n + ni++] = uint16_t(n + j);
            }
        }
        h.node[j] = uint16_t(wsum);   // <= ZE_BLOCK
    }
    h.parent[2 * n - 2] = 0;   // the root's depth; a parent's index is above its children's
    for (uint32_t i = 2 * n - 2; i-- > 0;) h.parent[i] = uint16_t(h.parent[h.parent[i]] + 1);
    for (uint32_t s = 0; s < 256; s++) h.clen[s] = 0;
    // limit to 11 bits and repair the Kraft sum (units of 2^-11): lengthen the rarest of the longest
    // codes below 11 until it is <= 1, then shorten the most frequent code that fits until it is 1
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t l = h.parent[i] > ZE_HUF_MAX ? ZE_HUF_MAX : h.parent[i];
        h.clen[h.order[i]] = uint8_t(l);
        kraft += 1u << (ZE_HUF_MAX - l);
    }
    const uint32_t one = 1u << ZE_HUF_MAX;
    while (kraft > one) {
        uint32_t best = ZE_NONE, bl = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t l = h.clen[h.order[i]];
            if (l < ZE_HUF_MAX && l > bl) { bl = l; best = i; }
        }
        h.clen[h.order[best]] = uint8_t(bl + 1);
        kraft -= 1u << (ZE_HUF_MAX - bl - 1);
    }
    while (kraft < one) {
        for (uint32_t i = n; i-- > 0;) {
            const uint32_t l = h.clen[h.order[i]];
            if (l > 1 && (1u << (ZE_HUF_MAX - l)) <= one - kraft) {
                h.clen[h.order[i]] = uint8_t(l - 1);
                kraft += 1u << (ZE_HUF_MAX - l);
                break;
            }
        }
    }
    // weights, and the codes as huf_read lays its table out: by weight, then by symbol
    uint32_t maxlen = 0, maxsym = 0, rank[ZE_HUF_MAX + 2], next[ZE_HUF_MAX + 2];
    for (uint32_t s = 0; s < 256; s++)
        if (h.clen[s]) { maxsym = s; if (h.clen[s] > maxlen) maxlen = h.clen[s]; }
    for (uint32_t k = 0; k <= ZE_HUF_MAX + 1; k++) rank[k] = 0;
    for (uint32_t s = 0; s <= maxsym; s++) {
        const uint32_t w = h.clen[s] ? maxlen + 1 - h.clen[s] : 0;
        h.weights[s] = uint8_t(w);
        rank[w]++;
    }
    uint32_t acc = 0;
    for (uint32_t k = 1; k <= maxlen; k++) { next[k] = acc >> (k - 1); acc += rank[k] << (k - 1); }
    for (uint32_t s = 0; s <= maxsym; s++)
        if (h.weights[s]) h.code[s] = uint16_t(next[h.weights[s]]++);
    h.maxlen = maxlen;
    h.maxsym = maxsym;
    // the description lists the weights below the last present symbol
    const uint32_t nw = maxsym;
    const uint32_t direct = nw <= 128 ? 1 + (nw + 1) / 2 : ZE_NONE;
    const uint32_t fse = huf_weights_fse(W, nw, h.tree);
    if (fse && fse < direct) {
        h.tree_len = fse;
        h.tree_fse = 1;
    } else if (direct != ZE_NONE) {
        h.tree[0] = uint8_t(127 + nw);
        for (uint32_t i = 0; i < (nw + 1) / 2; i++)
            h.tree[1 + i] = uint8_t(h.weights[2 * i] << 4 | (2 * i + 1 < nw ? h.weights[2 * i + 1] : 0));
        h.tree_len = direct;
    }
}

// The streams' symbol counts (before the bits are summed).
PF_HD inline void lit_streams_plan(EncWork& W) {
    LitPlan& p = W.lp;
    p.streams = W.nlit > 1023 ? 4 : 1;
    const uint32_t seg = (W.nlit + 3) / 4;
    for (uint32_t k = 0; k < 4; k++) p.cnt[k] = p.streams == 1 ? (k == 0 ? W.nlit : 0) : (k < 3 ? seg : W.nlit - 3 * seg);
}
// A lane's symbols of stream k: [i0, i1) within the literals.
PF_HD inline void huf_lane_range(const EncWork& W, uint32_t k, uint32_t lane, uint32_t nl, uint32_t& i0, uint32_t& i1) {
    const uint32_t s0 = W.lp.streams == 1 ? 0 : k * ((W.nlit + 3) / 4), cnt = W.lp.cnt[k], per = (cnt + nl - 1) / nl;
    const uint32_t a = lane * per < cnt ? lane * per : cnt, b = a + per < cnt ? a + per : cnt;
    i0 = s0 + a;
    i1 = s0 + b;
}
// Bits of every lane's symbols -> h.lanebits[k * ZE_LANES + lane].
PF_HD inline void huf_count_bits(EncWork& W, uint32_t lane, uint32_t nl) {
    for (uint32_t k = 0; k < W.lp.streams; k++) {
        uint32_t i0, i1, sum = 0;
        huf_lane_range(W, k, lane, nl, i0, i1);
        for (uint32_t i = i0; i < i1; i++) sum += ew_huf(W).clen[ew_lit(W)[i]];
        ew_huf(W).lanebits[k * ZE_LANES + lane] = sum;
    }
}
// A lane's codes of every stream, ORed into the block at out32 (zeroed before); bit0[k]: the stream's
// first bit. The last symbol lies lowest, because the decoder reads from the top down.
PF_HD inline void huf_put(EncWork& W, uint32_t* out32, const uint32_t* bit0, uint32_t lane, uint32_t nl) {
    for (uint32_t k = 0; k < W.lp.streams; k++) {
        uint32_t i0, i1;
        huf_lane_range(W, k, lane, nl, i0, i1);
        uint32_t pos = bit0[k];
        for (uint32_t l = lane + 1; l < nl; l++) pos += ew_huf(W).lanebits[k * ZE_LANES + l];
        for (uint32_t i = i1; i-- > i0;) {
            const uint32_t s = ew_lit(W)[i], nb = ew_huf(W).clen[s];
            const uint64_t v = uint64_t(ew_huf(W).code[s]) << (pos & 31);
            or32(&out32[pos >> 5], uint32_t(v));
            if (v >> 32) or32(&out32[(pos >> 5) + 1], uint32_t(v >> 32));
            pos += nb;
        }
        if (lane == 0) or32(&out32[(bit0[k] + W.lp.bits[k]) >> 5], 1u << ((bit0[k] + W.lp.bits[k]) & 31));   // the end mark
    }
}

PF_HD inline uint32_t lit_raw_hdr(uint32_t n) { return n < 32 ? 1 : n < 4096 ? 2 : 3; }
// The cheapest of raw, RLE and Huffman, sizes only (after huf_build and huf_count_bits).
PF_HD inline void lit_plan(EncWork& W, uint32_t nl) {
    LitPlan& p = W.lp;
    const uint32_t n = W.nlit, rh = lit_raw_hdr(n);
    p.type = 0;
    p.hdr = rh;
    p.total = rh + n;
    if (ew_huf(W).ndist == 1 && rh + 1 < p.total) {
        p.type = 1;
        p.total = rh + 1;
    }
    if (ew_huf(W).ndist < 2 || ew_huf(W).tree_len == 0) return;
    uint32_t cs = ew_huf(W).tree_len + (p.streams == 4 ? 6 : 0);
    for (uint32_t k = 0; k < p.streams; k++) {
        uint32_t b = 0;
        for (uint32_t l = 0; l < nl; l++) b += ew_huf(W).lanebits[k * ZE_LANES + l];
        p.bits[k] = b;
        p.bytes[k] = b / 8 + 1;
        cs += p.bytes[k];
    }
    const uint32_t big = n > cs ? n : cs;
    const uint32_t hh = p.streams == 1 ? 3 : big < 16384 ? 4 : 5;
    if (p.streams == 1 && big > 1023) return;
    if (p.streams == 4 && (p.bytes[0] > 65535 || p.bytes[1] > 65535 || p.bytes[2] > 65535 || big >= (1u << 18))) return;
    if (hh + cs < p.total) {
        p.type = 2;
        p.hdr = hh;
        p.total = hh + cs;
    }
}
// Header, tree description and jump table of the literals section at o; bit0[k]: where stream k's bits
// start, counted from `base` (o's offset in the block). Raw and RLE literals: the header alone.
PF_HD inline void lit_write_head(EncWork& W, uint8_t* o, uint32_t base, uint32_t* bit0) {
    const LitPlan& p = W.lp;
    const uint32_t n = W.nlit;
    if (p.type < 2) {
        const uint32_t v = p.hdr == 1 ? (n << 3 | p.type) : (n << 4 | (p.hdr == 2 ? 4u : 12u) | p.type);
        for (uint32_t k = 0; k < p.hdr; k++) o[k] = uint8_t(v >> (8 * k));
        if (p.type == 1) o[p.hdr] = ew_lit(W)[0];
        return;
    }
    const uint32_t cs = p.total - p.hdr, wbits = p.hdr == 3 ? 10 : p.hdr == 4 ? 14 : 18;
    const uint32_t sf = p.streams == 1 ? 0 : p.hdr == 3 ? 1 : p.hdr == 4 ? 2 : 3;
    const uint64_t v = 2u | sf << 2 | uint64_t(n) << 4 | uint64_t(cs) << (4 + wbits);
    for (uint32_t k = 0; k < p.hdr; k++) o[k] = uint8_t(v >> (8 * k));
    uint32_t at = p.hdr;
    for (uint32_t k = 0; k < ew_huf(W).tree_len; k++) o[at++] = ew_huf(W).tree[k];
    if (p.streams == 4)
        for (uint32_t k = 0; k < 3; k++) { o[at++] = uint8_t(p.bytes[k]); o[at++] = uint8_t(p.bytes[k] >> 8); }
    for (uint32_t k = 0; k < p.streams; k++) { bit0[k] = (base + at) * 8; at += p.bytes[k]; }
}

// ---- sequences ----
// (One lane, serial: kept as the kernel's A/B variant PF_ZE_SERIAL_SEQ; the model and the kernel use the split form
// below.) The section for sll / sml / sof[0 .. nseq) into dst[0 .. cap): the count, the modes byte (all
// predefined) and the bitstream, written from the last sequence to the first in the mirror of
// seq_init / seq_next. Returns its bytes, ZE_NONE when they do not fit. reps: repeat codes used.
PF_HD inline uint32_t seq_encode(EncWork& W, uint8_t* dst, uint32_t cap) {
    const uint32_t n = W.nseq;
    W.reps = 0;
    if (cap < 4) return ZE_NONE;
    if (n == 0) { dst[0] = 0; return 1; }
    uint32_t at = 0;
    if (n < 128) dst[at++] = uint8_t(n);
    else if (n < 0x7f00) { dst[at++] = uint8_t((n >> 8) + 128); dst[at++] = uint8_t(n); }
    else { dst[at++] = 255; dst[at++] = uint8_t(n - 0x7f00); dst[at++] = uint8_t((n - 0x7f00) >> 8); }
    dst[at++] = 0;   // Symbol_Compression_Modes: LL, OF, ML predefined
    BitW b;
    bw_init(b, dst + at, cap - at);
    uint32_t sl = 0, so = 0, sm = 0;
    for (uint32_t i = n; i-- > 0;) {
        const uint32_t ll = W.sll[i], ml = W.sml[i], off = W.sof[i];
        // repeat offset 1: the job's last offset, once it has one; only with literals in front
        const bool rep = i > 0 && off == W.sof[i - 1] && ll > 0;
        const uint32_t ov = rep ? 1u : off + 3;
        W.reps += rep ? 1u : 0u;
        uint32_t lb, mb;
        const uint32_t lc = ll_code(ll, lb), mc = ml_code(ml, mb), oc = hibit(ov);
        if (i + 1 == n) {
            sl = fse_enc_init(W.fll, lc);
            so = fse_enc_init(W.fof, oc);
            sm = fse_enc_init(W.fml, mc);
        } else {   // the decoder updates LL, ML, OF after this sequence's extra bits
            uint32_t bits, nb;
            so = fse_enc_step(W.fof, oc, so, bits, nb);
            bw_add(b, bits, nb);
            sm = fse_enc_step(W.fml, mc, sm, bits, nb);
            bw_add(b, bits, nb);
            sl = fse_enc_step(W.fll, lc, sl, bits, nb);
            bw_add(b, bits, nb);
        }
        bw_add(b, ll - lb, ll_bits(lc));   // read as OF, ML, LL
        bw_add(b, ml - mb, ml_bits(mc));
        bw_add(b, ov - (1u << oc), oc);
    }
    bw_add(b, sm, W.fml.log);   // read first: LL, OF, ML
    bw_add(b, so, W.fof.log);
    bw_add(b, sl, W.fll.log);
    bw_close(b);
    if (b.ovf) return ZE_NONE;
    return at + b.at;
}

// The same section by many lanes. A sequence's fields are fixed by its codes and by the three FSE state
// chains, and each chain depends on nothing but its own codes, so: seq_codes (every lane) stores the
// LL / OF / ML codes as bytes over the job's dead bytes; seq_chain (one lane per chain, the same code over
// three tables) walks its chain from the last sequence to the first and replaces every code by
// 1 << nb | bits, the bits the decoder reads when it leaves that sequence; seq_count sums the bits of a
// lane's run of consecutive sequences; seq_head sizes the section; seq_put ORs every field into place
// (dwords zeroed before). The bytes are seq_encode's.
PF_HD inline uint8_t* seq_cb(EncWork& W, uint32_t k) { return ew_buf(W) + k * ZE_SEQ_MAX; }
PF_HD inline uint32_t seq_ov(const EncWork& W, uint32_t i) {
    return (i > 0 && W.sof[i] == W.sof[i - 1] && W.sll[i] > 0) ? 1u : uint32_t(W.sof[i]) + 3;
}
PF_HD inline void seq_codes(EncWork& W, uint32_t lane, uint32_t nl) {   // W.reps zeroed before
    for (uint32_t i = lane; i < W.nseq; i += nl) {
        uint32_t b;
        const uint32_t ov = seq_ov(W, i);
        seq_cb(W, 0)[i] = uint8_t(ll_code(W.sll[i], b));
        seq_cb(W, 1)[i] = uint8_t(hibit(ov));
        seq_cb(W, 2)[i] = uint8_t(ml_code(W.sml[i], b));
        if (ov == 1) add32(&W.reps, 1u);
    }
}
PF_HD inline void seq_chain(EncWork& W, uint32_t k) {   // k: 0 LL, 1 OF, 2 ML; nseq > 0
    const EncFse& e = k == 0 ? W.fll : k == 1 ? W.fof : W.fml;
    uint8_t* c = seq_cb(W, k);
    const uint32_t n = W.nseq;
    uint32_t st = fse_enc_init(e, c[n - 1]);
    c[n - 1] = 1;
    for (uint32_t i = n - 1; i-- > 0;) {
        uint32_t bits, nb;
        st = fse_enc_step(e, c[i], st, bits, nb);
        c[i] = uint8_t(1u << nb | bits);
    }
    W.seq_fin[k] = st;
}
PF_HD inline void seq_lane_range(const EncWork& W, uint32_t lane, uint32_t nl, uint32_t& i0, uint32_t& i1) {
    const uint32_t n = W.nseq, per = (n + nl - 1) / nl;
    i0 = lane * per < n ? lane * per : n;
    i1 = i0 + per < n ? i0 + per : n;
}
PF_HD inline void seq_count(EncWork& W, uint32_t lane, uint32_t nl) {
    uint32_t i0, i1, sum = 0;
    seq_lane_range(W, lane, nl, i0, i1);
    for (uint32_t i = i0; i < i1; i++) {
        uint32_t b;
        sum += ll_bits(ll_code(W.sll[i], b)) + ml_bits(ml_code(W.sml[i], b)) + hibit(seq_ov(W, i));
        for (uint32_t k = 0; k < 3; k++) sum += hibit(seq_cb(W, k)[i]);
    }
    W.seq_lane[lane] = sum;
}
// Count and modes byte at dst; W.seq_bytes: the section's bytes, ZE_NONE when they pass cap.
PF_HD inline void seq_head(EncWork& W, uint8_t* dst, uint32_t cap, uint32_t nl) {
    const uint32_t n = W.nseq;
    if (n == 0) { dst[0] = 0; W.seq_bytes = 1; W.seq_at = 1; W.seq_bits = 0; return; }
    uint32_t at = 0, bits = 0;
    if (n < 128) dst[at++] = uint8_t(n);
    else if (n < 0x7f00) { dst[at++] = uint8_t((n >> 8) + 128); dst[at++] = uint8_t(n); }
    else { dst[at++] = 255; dst[at++] = uint8_t(n - 0x7f00); dst[at++] = uint8_t((n - 0x7f00) >> 8); }
    dst[at++] = 0;   // Symbol_Compression_Modes: LL, OF, ML predefined
    for (uint32_t l = 0; l < nl; l++) bits += W.seq_lane[l];
    W.seq_at = at;
    W.seq_bits = bits;
    const uint32_t bytes = at + (bits + W.fll.log + W.fof.log + W.fml.log) / 8 + 1;
    W.seq_bytes = bytes + 8 <= cap ? bytes : ZE_NONE;   // (8: the dwords a field may straddle)
}
PF_HD inline void seq_or(uint32_t* out32, uint32_t& pos, uint32_t v, uint32_t nb) {
    const uint64_t x = uint64_t(v) << (pos & 31);
    if (uint32_t(x)) or32(&out32[pos >> 5], uint32_t(x));
    if (x >> 32) or32(&out32[(pos >> 5) + 1], uint32_t(x >> 32));
    pos += nb;
}
PF_HD inline void seq_put(EncWork& W, uint32_t* out32, uint32_t lane, uint32_t nl) {
    const uint32_t n = W.nseq;
    if (n == 0 || W.seq_bytes == ZE_NONE) return;
    uint32_t i0, i1, pos = W.seq_at * 8;
    seq_lane_range(W, lane, nl, i0, i1);
    for (uint32_t l = lane + 1; l < nl; l++) pos += W.seq_lane[l];
    for (uint32_t i = i1; i-- > i0;) {
        for (int k = 1; k <= 3; k++) {   // the state bits as the decoder reads them last: OF, ML, LL
            const uint32_t m = seq_cb(W, k == 3 ? 0 : uint32_t(k))[i], nb = hibit(m);
            seq_or(out32, pos, m - (1u << nb), nb);
        }
        uint32_t lb, mb;
        const uint32_t ov = seq_ov(W, i), lc = ll_code(W.sll[i], lb), mc = ml_code(W.sml[i], mb), oc = hibit(ov);
        seq_or(out32, pos, W.sll[i] - lb, ll_bits(lc));
        seq_or(out32, pos, W.sml[i] - mb, ml_bits(mc));
        seq_or(out32, pos, ov - (1u << oc), oc);
    }
    if (lane == 0) {   // the states the decoder starts from (read LL, OF, ML) and the end mark, at the top
        pos = W.seq_at * 8 + W.seq_bits;
        seq_or(out32, pos, W.seq_fin[2], W.fml.log);
        seq_or(out32, pos, W.seq_fin[1], W.fof.log);
        seq_or(out32, pos, W.seq_fin[0], W.fll.log);
        seq_or(out32, pos, 1, 1);
    }
}

// Block type and Block_Size from the sections' sizes: compressed only when strictly smaller.
PF_HD inline void block_plan(EncWork& W, uint32_t len, bool all_equal) {
    if (all_equal) { W.btype = 1; W.bsize = len; return; }
    const uint32_t cs = W.seq_bytes == ZE_NONE ? ZE_NONE : W.lp.total + W.seq_bytes;
    if (cs < len) { W.btype = 2; W.bsize = cs; }
    else { W.btype = 0; W.bsize = len; }
}
PF_HD inline void block_header_put(uint8_t* o, uint32_t last, uint32_t type, uint32_t size) {
    const uint32_t v = (last & 1u) | type << 1 | size << 3;
    o[0] = uint8_t(v); o[1] = uint8_t(v >> 8); o[2] = uint8_t(v >> 16);
}
// Bytes a block of this plan takes after its 3-byte header.
PF_HD inline uint32_t block_payload(uint32_t type, uint32_t size) { return type == 1 ? 1u : size; }

// ---- the frame header (host) ----
// Magic, a descriptor with Single_Segment set and the content size in its shortest form. o: 9 bytes.
inline uint32_t frame_header_put(uint64_t n, uint8_t* o) {
    const uint32_t flag = n < 256 ? 0 : n < 65536 + 256 ? 1 : 2;
    o[0] = 0x28; o[1] = 0xb5; o[2] = 0x2f; o[3] = 0xfd;
    o[4] = uint8_t(flag << 6 | 1u << 5);
    if (flag == 0) { o[5] = uint8_t(n); return 6; }
    if (flag == 1) { o[5] = uint8_t(n - 256); o[6] = uint8_t((n - 256) >> 8); return 7; }
    for (int k = 0; k < 4; k++) o[5 + k] = uint8_t(n >> (8 * k));
    return 9;
}
constexpr uint8_t ZE_EMPTY_BLOCK[3] = {1, 0, 0};   // the last, raw, empty block of a frame of 0 bytes

#ifndef __HIP_DEVICE_COMPILE__
// ---- the host model ----
struct EncStats {
    uint64_t rep_codes, blocks_raw, blocks_rle, blocks_compressed, lit_raw, lit_rle, lit_huf, weights_fse, sequences;
};

// The wave's match finder, lane by lane: 64 positions a step, each looked up against the table as it
// was before the step; the first matching lane starts a match, later matching lanes past its end
// follow in the same step (a match that stays below ZE_MIN_MATCH is passed over); the positions passed
// are hashed in (the highest position of a hash wins, as the kernel's atomic max decides).
inline void find_matches_host(EncWork& W, uint32_t len) {
    const uint8_t* buf = ew_buf(W);
    for (uint32_t i = 0; i < (1u << ZE_HBITS); i++) W.tab[i] = 0;
    uint32_t ip = 0, lit = 0;
    W.nseq = 0;
    W.nlit = 0;
    while (ip + 4 <= len) {
        uint32_t c[ZE_LANES], h[ZE_LANES];
        uint64_t mask = 0;
        for (uint32_t lane = 0; lane < ZE_LANES; lane++) {
            const uint32_t q = ip + lane;
            const bool valid = q + 4 <= len;
            const uint32_t v = valid ? ze_ld32(buf, q) : 0u;
            h[lane] = ze_hash(v);
            c[lane] = valid ? W.tab[h[lane]] : 0u;
            if (valid && c[lane] != 0 && ze_ld32(buf, c[lane] - 1) == v) mask |= uint64_t(1) << lane;
        }
        uint32_t e = ip + ZE_LANES;
        if (mask) {
            uint64_t mk = mask;
            e = ip;
            while (mk) {
                const uint32_t f = uint32_t(__builtin_ctzll(mk)), qf = ip + f, cand = c[f] - 1;
                uint32_t L = 4;
                while (qf + L < len && buf[qf + L] == buf[cand + L]) L++;
                if (L < ZE_MIN_MATCH) { mk &= mk - 1; continue; }
                for (uint32_t j = lit; j < qf; j++) ew_lit(W)[W.nlit++] = buf[j];
                W.sll[W.nseq] = uint16_t(qf - lit);
                W.sml[W.nseq] = uint16_t(L);
                W.sof[W.nseq] = uint16_t(qf - cand);
                W.nseq++;
                e = qf + L;
                lit = e;
                mk = e - ip >= 64 ? 0ull : (mk & ~((1ull << (e - ip)) - 1ull));
            }
            if (e == ip) e = ip + ZE_LANES;   // every match of the step was too short
        }
        for (uint32_t lane = 0; lane < ZE_LANES; lane++) {
            const uint32_t q = ip + lane;
            if (q + 4 <= len && q < e) W.tab[h[lane]] = q + 1;
        }
        ip = e;
    }
    for (uint32_t j = lit; j < len; j++) ew_lit(W)[W.nlit++] = buf[j];
}

// The block of a job whose sequences and literals stand in W (the block assembler): sizes first, then
// the cheapest form, header included, at dst, which takes 3 + len bytes. src: the job's bytes.
inline uint32_t assemble_host(EncWork& W, const uint8_t* src, uint32_t len, bool last, bool all_equal, uint8_t* dst, EncStats* st) {
    W.seq_bytes = ZE_NONE;
    if (!all_equal) {
        for (uint32_t s = 0; s < 256; s++) ew_huf(W).hist[s] = 0;
        ew_huf(W).ndist = 0;
        huf_hist(W, 0, 1);
        huf_sort(W, 0, 1);
        huf_build(W);
        lit_streams_plan(W);
        huf_count_bits(W, 0, 1);
        lit_plan(W, 1);
        W.reps = 0;
        for (uint32_t i = 0; i < ZE_SEQ_CAP / 4; i++) W.tab[i] = 0;
        seq_codes(W, 0, 1);
        for (uint32_t k = 0; k < 3 && W.nseq; k++) seq_chain(W, k);
        seq_count(W, 0, 1);
        seq_head(W, ew_seq(W), ZE_SEQ_CAP, 1);
        seq_put(W, W.tab, 0, 1);
    }
    block_plan(W, len, all_equal);
    block_header_put(dst, last ? 1u : 0u, W.btype, W.bsize);
    if (W.btype == 1) {
        dst[3] = src[0];
    } else if (W.btype == 0) {
        for (uint32_t i = 0; i < len; i++) dst[3 + i] = src[i];
    } else {   // assembled in the work area (the job's bytes are not needed any more), as the kernel does
        uint32_t* out32 = W.amem;
        uint8_t* out = ew_buf(W);
        for (uint32_t i = 0; i < (ZE_BLOCK + 16) / 4; i++) out32[i] = 0;
        lit_write_head(W, out, 0, W.lp.bit0);
        if (W.lp.type == 2) huf_put(W, out32, W.lp.bit0, 0, 1);
        else if (W.lp.type == 0) for (uint32_t i = 0; i < W.nlit; i++) out[W.lp.hdr + i] = ew_lit(W)[i];
        for (uint32_t i = 0; i < W.seq_bytes; i++) out[W.lp.total + i] = ew_seq(W)[i];
        for (uint32_t i = 0; i < W.bsize; i++) dst[3 + i] = out[i];
    }
    if (st) {
        st->blocks_raw += W.btype == 0;
        st->blocks_rle += W.btype == 1;
        st->blocks_compressed += W.btype == 2;
        if (W.btype == 2) {
            st->lit_raw += W.lp.type == 0;
            st->lit_rle += W.lp.type == 1;
            st->lit_huf += W.lp.type == 2;
            st->weights_fse += W.lp.type == 2 && ew_huf(W).tree_fse;
            st->rep_codes += W.reps;
            st->sequences += W.nseq;
        }
    }
    return 3 + block_payload(W.btype, W.bsize);
}

// One job: src[0 .. len) -> the whole block (header included) at dst, which takes 3 + len bytes.
inline uint32_t compress_job_host(EncWork& W, const uint8_t* src, uint32_t len, bool last, uint8_t* dst, EncStats* st) {
    uint8_t* buf = ew_buf(W);
    for (uint32_t i = 0; i < len + 16; i++) buf[i] = i < len ? src[i] : 0;
    bool all_equal = true;
    for (uint32_t i = 1; i < len; i++) all_equal = all_equal && src[i] == src[0];
    if (!all_equal) {
        fse_enc_predefined(K_LL, W.fll, ew_fs(W, 0));
        fse_enc_predefined(K_OF, W.fof, ew_fs(W, 1));
        fse_enc_predefined(K_ML, W.fml, ew_fs(W, 2));
        find_matches_host(W, len);
    }
    return assemble_host(W, src, len, last, all_equal, dst, st);
}

// The frame of src[0 .. n): what pf_zstd_compress returns, byte for byte. Z_CORRUPT: dst is too small
// (*out_len is still the size needed).
inline int compress_host(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, EncWork& W, EncStats* st = nullptr) {
    uint8_t hdr[9], blk[3 + ZE_BLOCK];
    size_t op = 0;
    bool fits = true;
    auto put = [&](const uint8_t* p, size_t k) {
        if (op + k <= cap) { for (size_t i = 0; i < k; i++) dst[op + i] = p[i]; } else fits = false;
        op += k;
    };
    put(hdr, frame_header_put(n, hdr));
    if (n == 0) put(ZE_EMPTY_BLOCK, 3);
    for (size_t o = 0; o < n; o += ZE_BLOCK) {
        const uint32_t len = uint32_t(n - o < ZE_BLOCK ? n - o : ZE_BLOCK);
        put(blk, compress_job_host(W, src + o, len, o + len == n, blk, st));
    }
    *out_len = op;
    return fits ? Z_OK : Z_CORRUPT;
}
#endif

}  // namespace zstd
}  // namespace pf
