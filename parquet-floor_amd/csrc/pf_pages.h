// pf_pages.h — device code shared by the page-decode units (pf_ba.hip, the pf_flat*.hip units
// through pf_flat.h, pf_decode.hip, pf_snappy_head.hip). The build has no relocatable device code, so every function here is
// compiled again in each unit that calls it; nothing in this header defines a kernel or a
// __device__ variable.
//
//   page_sections      where a data page's rep / def / values sections lie (parquet-mr
//                      ColumnReaderImpl.readPageV1 / readPageV2)
//   decode_level_tile  a tile of def / rep levels (RunLengthBitPackingHybridDecoder, and the
//                      deprecated BIT_PACKED ByteBitPackingValuesReader)
//   wave_walk_runs     run headers of a hybrid stream into a run table, one wave; run_find /
//                      run_value read it back; all_present is the one-lane "no nulls" test
//   ld_*_any, gld_*    unaligned loads as aligned dwords + v_alignbyte
//   copy_value / zero_value / flush_bits  value slots and validity bitmap words
#pragma once
#include <hip/hip_runtime.h>

#include "pf_device.h"

namespace pf {

constexpr int NT = 256;   // threads of a page-decode workgroup

#ifndef PF_TILE
#define PF_TILE 512   // k_count / k_decode level tiles: 512 beat 1024 in 6 of 6 runs (~0.7 %), 2048 3 % slower
#endif
constexpr int TILE = PF_TILE;
constexpr int EPT = TILE / NT;   // entries per thread per tile (4 consecutive)

// ---- page section layout ------------------------------------------------------------------
struct Sections {
    const uint8_t* rep; uint64_t rep_n;
    const uint8_t* def; uint64_t def_n;
    const uint8_t* val; uint64_t val_n;
    int rep_rle, def_rle;    // 1 = RLE hybrid, 0 = BIT_PACKED (v1 deprecated)
};

// v1: [rep][def][values], each RLE level section prefixed by its 4-byte LE length;
//     BIT_PACKED levels take ceil(n*bw/8) bytes, no prefix.
// v2: levels in pg.lvl (rep_len + def_len bytes, no prefixes), values in pg.body.
__device__ inline bool page_sections(const DevPage& pg, const DevChunk& ck, Sections& s) {
    s.rep = s.def = nullptr; s.rep_n = s.def_n = 0; s.rep_rle = s.def_rle = 1;
    if (pg.flags & PG_V2) {
        s.rep = pg.lvl; s.rep_n = pg.rep_len;
        s.def = pg.lvl + pg.rep_len; s.def_n = pg.def_len;
        s.val = pg.body; s.val_n = pg.body_len;
        if (ck.max_rep == 0) s.rep_n = 0;
        if (ck.max_def == 0) s.def_n = 0;
        return true;
    }
    uint64_t pos = 0, n = pg.body_len;
    const uint8_t* b = pg.body;
    for (int which = 0; which < 2; which++) {
        int maxl = which == 0 ? ck.max_rep : ck.max_def;
        if (maxl == 0) continue;
        int enc = which == 0 ? pg.rep_enc : pg.def_enc;
        const uint8_t* p; uint64_t len;
        if (enc == 3) {
            if (pos + 4 > n) return false;
            len = ld32le(b, pos, n);
            pos += 4;
            if (len > n - pos) return false;
            p = b + pos;
        } else if (enc == 4) {
            len = (uint64_t(pg.num_values) * bit_width(maxl) + 7) / 8;
            if (len > n - pos) return false;
            p = b + pos;
        } else {
            return false;
        }
        pos += len;
        if (which == 0) { s.rep = p; s.rep_n = len; s.rep_rle = enc == 3; }
        else { s.def = p; s.def_n = len; s.def_rle = enc == 3; }
    }
    s.val = b + pos; s.val_n = n - pos;
    return true;
}

// ---- tile-wise level decoding ---------------------------------------------------------------
struct LevelLds {
    Piece prep[TILE];
    Piece pdef[TILE];
    uint8_t rep[TILE];
    uint8_t def[TILE];
    RleState srep, sdef;
    int nprep, npdef;
    uint32_t count;
    int err;
};

// BIT_PACKED (deprecated, big-endian bit order: ByteBitPackingValuesReader BE) level at index i
__device__ __forceinline__ uint32_t bitpacked_be(const uint8_t* p, uint64_t n, uint64_t i, int bw) {
    uint32_t v = 0;
    for (int b = 0; b < bw; b++) {
        uint64_t bit = i * bw + b;
        v = (v << 1) | ((ld8(p, bit >> 3, n) >> (7 - (bit & 7))) & 1);
    }
    return v;
}

// Decode the levels of entries [e0, e0 + want) into L.rep / L.def; returns count (== want) or
// sets L.err. Must be called by all threads (blockDim.x >= 128).
__device__ inline uint32_t decode_level_tile(LevelLds& L, const Sections& s, const DevChunk& ck,
                                             uint64_t e0, uint32_t want) {
    const int bwr = bit_width(ck.max_rep), bwd = bit_width(ck.max_def);
    // the two walks run concurrently on lanes of different waves
    if (threadIdx.x == 0) {
        L.nprep = 0;
        if (ck.max_rep > 0 && s.rep_rle) {
            uint32_t got = rle_walk(L.srep, s.rep, s.rep_n, bwr, want, L.prep, TILE, L.nprep);
            if (got != want || L.srep.err) L.err = 1;
        }
    } else if (threadIdx.x == 64) {
        L.npdef = 0;
        if (ck.max_def > 0 && s.def_rle) {
            uint32_t got = rle_walk(L.sdef, s.def, s.def_n, bwd, want, L.pdef, TILE, L.npdef);
            if (got != want || L.sdef.err) L.err = 1;
        }
    }
    __syncthreads();
    if (L.err) return 0;
    if (ck.max_rep > 0) {
        if (s.rep_rle) rle_expand<uint8_t>(L.prep, L.nprep, s.rep, s.rep_n, bwr, L.rep);
        else for (uint32_t i = threadIdx.x; i < want; i += NT) L.rep[i] = uint8_t(bitpacked_be(s.rep, s.rep_n, e0 + i, bwr));
    } else {
        for (uint32_t i = threadIdx.x; i < want; i += NT) L.rep[i] = 0;
    }
    if (ck.max_def > 0) {
        if (s.def_rle) rle_expand<uint8_t>(L.pdef, L.npdef, s.def, s.def_n, bwd, L.def);
        else for (uint32_t i = threadIdx.x; i < want; i += NT) L.def[i] = uint8_t(bitpacked_be(s.def, s.def_n, e0 + i, bwd));
    } else {
        for (uint32_t i = threadIdx.x; i < want; i += NT) L.def[i] = 0;
    }
    __syncthreads();
    // levels above their maximum are corrupt
    int bad = 0;
    for (uint32_t i = threadIdx.x; i < want; i += NT)
        bad |= (L.rep[i] > ck.max_rep) | (L.def[i] > ck.max_def);
    if (__syncthreads_or(bad)) { if (threadIdx.x == 0) L.err = 1; __syncthreads(); return 0; }
    return want;
}

// ---- values helpers ------------------------------------------------------------------------
// BYTE_ARRAY data pages: chars of the entries before each block of FBLK entries (the flat kernels split
// pages into blocks), written by the count kernels for dictionary pages (block_chars, pf_page_tables.h).
__device__ __forceinline__ uint64_t* flat_block_chars(const DevPage& pg) {
    if (!pg.aux) return nullptr;
    return block_chars(pg.aux, pg.aux_cap);
}
__device__ __forceinline__ bool is_dict_enc(int e) { return e == 2 || e == 8; }

// Copy one value of width w from `src` to `dst` (dst is aligned to w for w in {1,4,8}).
__device__ __forceinline__ void copy_value(uint8_t* dst, const uint8_t* src, int w) {
    if (w == 4) { uint32_t v = uint32_t(src[0]) | uint32_t(src[1]) << 8 | uint32_t(src[2]) << 16 | uint32_t(src[3]) << 24; *reinterpret_cast<uint32_t*>(dst) = v; }
    else if (w == 8) {
        uint64_t v = 0;
        #pragma unroll
        for (int k = 0; k < 8; k++) v |= uint64_t(src[k]) << (8 * k);
        *reinterpret_cast<uint64_t*>(dst) = v;
    } else {
        for (int k = 0; k < w; k++) dst[k] = src[k];
    }
}

__device__ __forceinline__ void zero_value(uint8_t* dst, int w) {
    if (w == 4) *reinterpret_cast<uint32_t*>(dst) = 0;
    else if (w == 8) *reinterpret_cast<uint64_t*>(dst) = 0;
    else for (int k = 0; k < w; k++) dst[k] = 0;
}

// Flush a bit array covering bits [b0, b0+nbits) (bit b0 stored at LDS bit (b0 & 31)) to words of
// `out` (bitmap, LSB-first). Edge words use atomicOr (neighbouring pages share them; the output
// bitmap is zeroed before the launch), inner words are plain stores.
__device__ inline void flush_bits(const uint32_t* bits, uint64_t b0, uint32_t nbits, uint8_t* out_bytes) {
    if (nbits == 0) return;
    uint32_t* out = reinterpret_cast<uint32_t*>(out_bytes);
    uint64_t w0 = b0 >> 5, w1 = (b0 + nbits - 1) >> 5;
    for (uint64_t w = w0 + threadIdx.x; w <= w1; w += blockDim.x) {
        uint32_t v = bits[w - w0];
        if (w == w0 || w == w1) { if (v) atomicOr(out + w, v); }
        else out[w] = v;
    }
}

// ---- run tables of RLE/bit-packed hybrid streams ------------------------------------------------
struct Run {
    uint32_t first;    // index of the first value the run covers (entries for levels)
    uint32_t count;
    uint32_t data;     // RLE value, or absolute bit offset of the run's packed values
    uint32_t packed;
};

// The run walk's contract (wave_walk_runs below): walk RLE/bit-packed hybrid run headers of p[0..n)
// (parquet-mr RunLengthBitPackingHybridDecoder) from the walker state (pos = next header, first =
// index of its first value) until `limit` values are covered. Runs that end at or before `lo` are
// skipped, the others are stored. Returns 0 covered (covered = limit), 1 stream ended or corrupt
// first, 2 table full (covered = end of the last stored run; the state points after it).
struct RunWalk {
    uint64_t pos;
    uint32_t first;
};

// ---- wave-parallel run discovery (north_star K2: run boundaries found by wavefront scans) ------
//
// The run headers of an RLE/bit-packed hybrid stream form a chain (each header's position follows
// from the previous run's length), and writers emit long stretches of identical headers: Arrow and
// parquet-mr cut bit-packed runs at 512 values (header 0x81 0x01), so a page of random dictionary
// ids or levels is ~40 runs with one byte stride. One round: every lane decodes the header at
// pos (the chain position, exact), then lane i decodes the header at pos + i * stride and votes
// whether it repeats lane 0's; the ballot's first failing lane ends the accepted prefix, and a
// prefix scan of the (equal) run lengths gives every accepted run's first value. A stretch of k
// equal runs costs one round instead of k dependent header loads; mixed runs still advance by
// one run per round. Called by all 64 lanes of one wave with wave-uniform arguments.
struct WaveRun {
    uint64_t pos;        // header position (uniform)
    uint32_t first;      // first value of the run at pos (uniform)
};
constexpr int WAVE_SERIAL_RUNS = 8;   // after a prediction fails at lane 1: this many runs without predicting

template <class Src>
__device__ __forceinline__ bool hdr_decode(const Src& B, uint64_t n, uint64_t p, int bw, uint64_t& h, uint32_t& hl,
                                           uint32_t& val) {
    h = 0;
    hl = 0;
    val = 0;
    #pragma unroll
    for (int k = 0; k < 5; k++) {
        if (p + uint64_t(k) >= n) return false;
        const uint32_t c = B(p + uint64_t(k));
        h |= uint64_t(c & 0x7fu) << (7 * k);
        if (!(c & 0x80u)) { hl = uint32_t(k) + 1u; break; }
    }
    if (hl == 0) return false;   // headers above 2^35 are not runs of a page
    if (!(h & 1)) {
        const uint32_t nbv = uint32_t(bw + 7) >> 3;
        if (p + hl + nbv > n) return false;
        for (uint32_t b = 0; b < nbv; b++) val |= uint32_t(B(p + hl + b)) << (8 * b);
    }
    return true;
}

// One discovery round from st (uniform). Returns the accepted runs k (lanes < k hold run `r`,
// with its count clipped at `limit`), 0 when the header at st.pos is an empty run (skipped), -1
// when the stream ends or is corrupt there. st advances past the accepted runs.
// spec = false: only the run at st.pos (no prediction; used after a round the prediction failed at
// lane 1, so streams of mixed runs cost one header decode per run instead of 64).
template <class Src>
__device__ int wave_run_round(const Src& B, uint64_t n, int bw, uint32_t limit, WaveRun& st, Run& r, bool& trunc,
                              bool spec = true) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t h0;
    uint32_t hl0, v0;
    if (!hdr_decode(B, n, st.pos, bw, h0, hl0, v0)) return -1;
    const bool packed = h0 & 1;
    const uint64_t cnt0 = packed ? (h0 >> 1) * 8 : (h0 >> 1);
    const uint64_t pay0 = packed ? (h0 >> 1) * uint64_t(bw) : uint64_t(uint32_t(bw + 7) >> 3);
    if (cnt0 == 0) {
        st.pos += hl0 + (packed ? 0 : pay0);
        return 0;
    }
    const uint64_t stride = uint64_t(hl0) + pay0;
    // lane i: the i-th run from st.pos, if the headers repeat
    const uint64_t p = st.pos + uint64_t(lane) * stride;
    bool ok = true;
    uint32_t v = v0;
    if (lane > 0) {
        uint64_t h;
        uint32_t hl;
        ok = spec && hdr_decode(B, n, p, bw, h, hl, v) && h == h0 && hl == hl0 && (!packed || p + hl + pay0 <= n);
    }
    const uint64_t fail = __ballot(!ok);
    uint32_t k = fail ? uint32_t(__ffsll((unsigned long long)fail) - 1) : 64u;
    // runs needed to reach `limit` (the last one clipped)
    const uint64_t left = uint64_t(limit - st.first);
    const uint64_t need = (left + cnt0 - 1) / cnt0;
    if (uint64_t(k) > need) k = uint32_t(need);
    const uint64_t f = uint64_t(st.first) + uint64_t(lane) * cnt0;
    r.first = uint32_t(f);
    r.count = uint32_t(min<uint64_t>(cnt0, f < limit ? uint64_t(limit) - f : 0));
    r.packed = packed ? 1u : 0u;
    r.data = packed ? uint32_t((p + hl0) * 8) : v;
    // a truncated final bit-packed run (lane 0 only: the others required the whole payload)
    uint64_t adv = uint64_t(k) * stride;
    trunc = packed && st.pos + stride > n;
    if (trunc) adv = n - st.pos;
    st.pos += adv;
    st.first = uint32_t(min<uint64_t>(uint64_t(st.first) + uint64_t(k) * cnt0, uint64_t(limit)));
    return int(k);
}

// The run walk by a whole wave from state st0 (runs / nruns / covered / the final state are written
// by lane 0 or by the lanes holding the runs). All 64 lanes call it. The start state is
// a value, not shared memory: one lane's store to LDS is not ordered before the other lanes' loads
// without a barrier.
[[maybe_unused]] static __device__ int wave_walk_runs(const uint8_t* p, uint64_t n, int bw, uint32_t lo, uint32_t limit, Run* runs, int cap,
                              int& nruns_out, uint32_t& covered_out, RunWalk& stw, RunWalk st0) {
    const uint32_t lane = threadIdx.x & 63u;
    const auto B = [p](uint64_t i) { return uint32_t(p[i]); };
    WaveRun st{st0.pos, st0.first};
    int nr = 0, ret = 0;
    uint32_t covered = st.first;
    int serial = 0;   // runs left to take one at a time after a failed prediction
    while (st.first < limit) {
        Run r;
        const uint64_t pos0 = st.pos;
        const uint32_t f0 = st.first;
        bool trunc;
        const int k = wave_run_round(B, n, bw, limit, st, r, trunc, serial == 0);
        if (k < 0) { ret = 1; break; }
        if (k == 0) continue;
        serial = serial > 0 ? serial - 1 : (k == 1 && st.first < limit ? WAVE_SERIAL_RUNS : 0);
        // stored: runs ending after lo (a prefix of the round's runs ends at or before lo)
        const bool keep = lane < uint32_t(k) && r.first + r.count > lo;
        const uint64_t km = __ballot(keep);
        const int nk = __popcll(km);
        const int rank = __popcll(km & ((1ull << lane) - 1ull));
        if (nr + nk > cap) {   // table full: store what fits, stop after the last stored run
            const int room = cap - nr;
            if (keep && rank < room) runs[nr + rank] = r;
            // the round's runs up to the last stored one: lanes [0, first kept lane + room)
            const uint32_t upto = uint32_t(__ffsll((unsigned long long)km) - 1) + uint32_t(room);
            const uint64_t stride = (st.pos - pos0) / uint64_t(k);
            st.pos = pos0 + uint64_t(upto) * stride;
            st.first = f0 + (upto ? __shfl(r.first + r.count, int(upto) - 1, 64) - f0 : 0u);
            covered = st.first;
            nr = cap;
            ret = 2;
            break;
        }
        if (keep) runs[nr + rank] = r;
        nr += nk;
        covered = st.first;
    }
    if (lane == 0) {
        nruns_out = nr;
        covered_out = covered;
        stw.pos = st.pos;
        stw.first = st.first;
    }
    return ret;
}

// Definition levels of p[0..n): 1 if every one of the `ne` levels is max_def (RLE runs only),
// 0 otherwise (or corrupt: the single-workgroup path reports it).
[[maybe_unused]] static __device__ int all_present(const uint8_t* p, uint64_t n, int bw, uint32_t ne, uint32_t max_def) {
    uint64_t pos = 0;
    uint32_t covered = 0;
    while (covered < ne) {
        uint64_t h;
        if (!uvarint(p, n, pos, h)) return 0;
        if (h & 1) return 0;
        const int nbv = (bw + 7) >> 3;
        if (pos + nbv > n) return 0;
        uint32_t v = 0;
        for (int b = 0; b < nbv; b++) v |= uint32_t(p[pos + b]) << (8 * b);
        pos += nbv;
        if ((h >> 1) == 0) continue;
        if (v != max_def) return 0;
        covered += uint32_t(min<uint64_t>(h >> 1, uint64_t(ne - covered)));
    }
    return 1;
}

// Unaligned loads from global memory as aligned dwords + v_alignbyte (the dwords covering
// [p, p + 4 or 8) plus up to 3 following bytes must be readable).
__device__ __forceinline__ uint32_t ld_u32_any(const uint8_t* p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
    const uint32_t sh = uint32_t(a & 3u);
    if (!sh) return q[0];
    return __builtin_amdgcn_alignbyte(q[1], q[0], sh);   // byte shift
}
__device__ __forceinline__ uint64_t ld_u64_any(const uint8_t* p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
    const uint32_t sh = uint32_t(a & 3u);
    const uint32_t d0 = q[0], d1 = q[1];
    if (!sh) return uint64_t(d0) | (uint64_t(d1) << 32);
    const uint32_t d2 = q[2];
    return uint64_t(__builtin_amdgcn_alignbyte(d1, d0, sh)) | (uint64_t(__builtin_amdgcn_alignbyte(d2, d1, sh)) << 32);
}
__device__ __forceinline__ uint64_t ld64_bytes(const uint8_t* p) {
    uint64_t v = 0;
    #pragma unroll
    for (int k = 0; k < 8; k++) v |= uint64_t(p[k]) << (8 * k);
    return v;
}
// LSB-first bit field of width w <= 32 starting at bit `sh` (< 8) of p (12 bytes readable from p).
// Branch-free unaligned loads from global memory for callers that guarantee the extra readable
// bytes: all dwords are loaded unconditionally (no per-lane branch on the alignment, so a thread's
// loads of several values stay in flight together) and joined with v_alignbyte (shift 0 = dword).
__device__ __forceinline__ uint32_t gld_u32_8(const uint8_t* p) {   // p + 8 readable
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const PF_GLOBAL uint32_t* q = (const PF_GLOBAL uint32_t*)(a & ~uintptr_t(3));
    return __builtin_amdgcn_alignbyte(q[1], q[0], uint32_t(a & 3u));
}
__device__ __forceinline__ uint64_t gld_u64_12(const uint8_t* p) {   // p + 12 readable
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const PF_GLOBAL uint32_t* q = (const PF_GLOBAL uint32_t*)(a & ~uintptr_t(3));
    const uint32_t sh = uint32_t(a & 3u), d0 = q[0], d1 = q[1], d2 = q[2];
    return uint64_t(__builtin_amdgcn_alignbyte(d1, d0, sh)) | (uint64_t(__builtin_amdgcn_alignbyte(d2, d1, sh)) << 32);
}
__device__ __forceinline__ uint32_t bits_fast(const uint8_t* p, uint32_t sh, int w) {   // p + 12 readable
    const uint64_t v = gld_u64_12(p) >> sh;
    return uint32_t(v & (w == 32 ? 0xffffffffull : ((1ull << w) - 1ull)));
}

// Index of the run holding value i (runs sorted by `first`, runs[0].first == 0).
// Last of rows [0, nr) whose first(row) <= key (row 0 when none is): the run tables' binary search,
// in the caller's index type I.
template <class I, class F>
__device__ __forceinline__ I last_row_le(I nr, uint32_t key, F first) {
    I lo = 0, hi = nr;
    while (hi - lo > 1) {
        const I mid = (lo + hi) >> 1;
        if (first(mid) <= key) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int run_find(const Run* runs, int nr, uint32_t i) {
    return last_row_le(nr, i, [runs](int r) { return runs[r].first; });
}
// Row i of a page's id run table (k_runs) as a Run; nr, cov: the table's nruns and covered
__device__ __forceinline__ Run id_run(const IdRunTab* T, uint32_t i, uint32_t nr, uint32_t cov) {
    const uint32_t f = T->fp(i);
    const uint32_t nf = i + 1 < nr ? T->first(i + 1) : cov;
    Run r;
    r.first = f & 0x7fffffffu;
    r.count = nf - r.first;
    r.data = T->data(i);
    r.packed = f >> 31;
    return r;
}

__device__ __forceinline__ uint32_t run_value(const Run& r, const uint8_t* p, uint64_t n, uint32_t i, int bw) {
    return r.packed ? bits_le(p, n, uint64_t(r.data) + uint64_t(i - r.first) * uint64_t(bw), bw) : r.data;
}

}  // namespace pf
