// pf_decode.hip — K2..K7, the general path: data pages of any shape, tile after tile, on gfx950.
//
// Replaces the per-value work parquet-mr 1.12.2 does behind ColumnReader (called from
// src/main/java/blue/strategic/parquet/ParquetReader.java:141-168 and :196-203):
//   K2 RLE/bit-packed hybrid expansion of def/rep levels and dictionary ids
//      (RunLengthBitPackingHybridDecoder, DictionaryValuesReader)
//   K3 dictionary gather (PlainValuesDictionary.decodeToX behind getX(), :151-161)
//   K4 PLAIN decode (Integer/Long/Float/Double/Boolean/Binary/FixedLen PlainValuesReader)
//   K5 DELTA_BINARY_PACKED (DeltaBinaryPackingValuesReader[ForLong]) — pf_delta.hip
//   K6 null scatter: def == maxDef test of ParquetReader.java:146 -> validity + slot positions
//   K7 repetition levels -> list offsets (ParquetReader.java:200's rep stream)
// Flat columns take the faster kernels of the pf_flat*.hip units where those apply, PLAIN BYTE_ARRAY length
// chains are walked by pf_ba.hip; every page they leave is decoded here.
//
// Kernels (256 threads, entries in tiles of TILE, unless noted):
//   k_count       a small grid striding over the data pages of BYTE_ARRAY / nested chunks: slots,
//                 values, rows, chars (+ per-value positions or dictionary ids in the page's aux buffer)
//   k_scan        per chunk, one wave: exclusive scans of the page counts -> output bases
//   k_decode      a small grid striding over the data pages still undecoded: levels -> validity /
//                 list offsets / levels; values -> slots (decode_page)
//   k_nest_lvl, k_count_seg, k_nest_scan, k_nest_ids, k_nest_chars, k_decode_seg
//                 nested pages cut into segments, each decoded by decode_page from checkpoints
#include <hip/hip_runtime.h>

#include "pf_launch.h"
#include "pf_pages.h"

namespace pf {

// ---- k_count ---------------------------------------------------------------------------------
struct CountLds {
    LevelLds L;
    Piece pval[TILE];
    uint32_t ids[TILE];
    uint32_t scan_tmp[NT / 64];
    RleState sval;
    int npval, verr;
    unsigned long long chars_acc;
};

__device__ void count_page(const DevChunk* __restrict__ chunks, DevPage* pages, int pi, DevChunkResult* res, BaJob* bajobs,
                           CountLds& C) {
    LevelLds& L = C.L;
    Piece* pval = C.pval;
    uint32_t* ids = C.ids;
    uint32_t* scan_tmp = C.scan_tmp;
    RleState& sval = C.sval;
    int& npval = C.npval;
    int& verr = C.verr;
    unsigned long long& chars_acc = C.chars_acc;
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    if (res[pg.chunk].status != 0) return;   // an earlier stage failed this chunk
    if (pg.counted == 1 || pg.seg_ok == 1) return;   // counted by k_count_flat / k_count_seg
    Sections s;
    const bool ok = page_sections(pg, ck, s);
    if (threadIdx.x == 0) {
        rle_init(L.srep); rle_init(L.sdef); rle_init(sval);
        L.err = ok ? 0 : 1; verr = 0; chars_acc = 0;
        sval.pos = 1;    // dictionary ids: skip the bit-width byte
    }
    __syncthreads();
    if (L.err) { if (threadIdx.x == 0) set_status(res, pg.chunk, ST_CORRUPT, pi); return; }

    const bool dict = is_dict_enc(pg.encoding);
    const bool binary = ck.ptype == 6;
    const int id_bw = (dict && s.val_n > 0) ? int(s.val[0]) : 0;
    uint64_t slots = 0, vals = 0, rows = 0;
    uint64_t* blk_chars = flat_block_chars(pg);
    for (uint64_t e0 = 0; e0 < uint64_t(pg.num_values); e0 += TILE) {
        uint32_t want = uint32_t(min<uint64_t>(TILE, uint64_t(pg.num_values) - e0));
        if (binary && dict && blk_chars && e0 % FBLK == 0 && threadIdx.x == 0) blk_chars[e0 / FBLK] = chars_acc;
        decode_level_tile(L, s, ck, e0, want);
        if (L.err) break;
        uint32_t ns = 0, nv = 0, nr = 0;
        for (uint32_t i = threadIdx.x; i < want; i += NT) {
            int d = L.def[i];
            ns += (ck.max_rep == 0 || d >= ck.repeated_def);
            nv += (d == ck.max_def);
            nr += (L.rep[i] == 0);
        }
        uint32_t t;
        block_excl_scan<NT>(ns, scan_tmp, t); slots += t;
        block_excl_scan<NT>(nr, scan_tmp, t); rows += t;
        block_excl_scan<NT>(nv, scan_tmp, t);
        // dictionary ids of this tile's present values: decode, keep in aux, sum lengths
        if (binary && dict && t > 0) {
            if (threadIdx.x == 0) {
                if (id_bw > 32 || !ck.dict_len) verr = 1;
                else {
                    uint32_t got = rle_walk(sval, s.val, s.val_n, id_bw, t, pval, TILE, npval);
                    if (got != t || sval.err) verr = 1;
                }
            }
            __syncthreads();
            if (verr) break;
            rle_expand<uint32_t>(pval, npval, s.val, s.val_n, id_bw, ids);
            __syncthreads();
            uint64_t acc = 0;
            int bad = 0;
            for (uint32_t i = threadIdx.x; i < t; i += NT) {
                uint32_t id = ids[i];
                if (int64_t(id) >= ck.dict_n) { bad = 1; continue; }
                acc += ck.dict_len[id];
                pg.aux[vals + i] = id;
            }
            if (__syncthreads_or(bad)) { if (threadIdx.x == 0) verr = 1; __syncthreads(); break; }
            atomicAdd(&chars_acc, (unsigned long long)acc);
        }
        vals += t;
        __syncthreads();
    }
    if (L.err || verr) { if (threadIdx.x == 0) set_status(res, pg.chunk, ST_CORRUPT, pi); return; }
    if (binary && (pg.encoding == 6 || pg.encoding == 7) && pg.dx) {
        // DELTA_LENGTH_BYTE_ARRAY / DELTA_BYTE_ARRAY: lengths decoded by k_dlen (pf_delta.hip)
        if (threadIdx.x == 0) {
            if (int64_t(vals) > pg.dx_total || int64_t(vals) > pg.dx_bad) verr = 1;
            else chars_acc = dx_cpos(pg.dx)[vals];
        }
        __syncthreads();
        if (verr) { if (threadIdx.x == 0) set_status(res, pg.chunk, ST_CORRUPT, pi); return; }
    } else if (binary && !dict) {
        if (pg.encoding != 0 || pg.ba_job < 0) {
            if (threadIdx.x == 0) set_status(res, pg.chunk, ST_ENCODING, pi);
            return;
        }
        if (threadIdx.x == 0) {   // the value chain is walked by the k_ba_* kernels
            BaJob& J = bajobs[pg.ba_job];
            J.p = s.val;
            J.n = uint32_t(min<uint64_t>(s.val_n, J.n_cap));
            J.count = int64_t(vals);
            J.state = vals > 0 ? BA_OK : BA_SKIP;
            chars_acc = 0;
        }
        __syncthreads();
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        pg.n_slots = int64_t(slots);
        pg.n_values = int64_t(vals);
        pg.n_rows = int64_t(rows);
        pg.n_chars = int64_t(chars_acc);
    }
}

// Grid-stride over the BYTE_ARRAY / nested pages with a small grid: nearly every page is counted by
// k_count_flat or k_count_seg and skipped here, and a block per page (22 KiB of LDS each) waited for
// CUs held by the other streams' kernels (13-96 us per no-op launch in the r04 kernel trace).
// Grid-stride over a batch's page list for kernels most of whose pages are already done: a block
// tests NT of its pages at once (one round of loads instead of a few dependent loads per page in
// series) and runs `body` only on those `need` accepts, in turn (page order does not matter: each
// page writes its own outputs).
template <typename Need, typename Body>
__device__ __forceinline__ void stride_pages(const int* page_list, int n, Need need, Body body) {
    __shared__ int s_idx[NT];
    __shared__ int s_cnt;
    for (int c0 = 0; int(blockIdx.x) + c0 * int(gridDim.x) < n; c0 += NT) {
        const int i = int(blockIdx.x) + (c0 + int(threadIdx.x)) * int(gridDim.x);
        const int pi = i < n ? page_list[i] : -1;
        const bool w = pi >= 0 && need(pi);
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        if (w) s_idx[atomicAdd(&s_cnt, 1)] = pi;
        __syncthreads();
        const int m = s_cnt;
        for (int k = 0; k < m; k++) {
            body(s_idx[k]);
            __syncthreads();
        }
        __syncthreads();   // (everyone has read s_cnt before the next round resets it)
    }
}

__global__ __launch_bounds__(NT) void k_count(const DevChunk* __restrict__ chunks, DevPage* pages,
                                              const int* page_list, int n, DevChunkResult* res, BaJob* bajobs) {
    __shared__ CountLds C;
    // (count_page's own early exits, tested for a block's pages at once)
    stride_pages(page_list, n,
                 [&](int pi) { const DevPage& pg = pages[pi]; return (res[pg.chunk].status == 0) & (pg.counted != 1) & (pg.seg_ok != 1); },
                 [&](int pi) { count_page(chunks, pages, pi, res, bajobs, C); });
}

// ---- k_scan (one wave per chunk) ------------------------------------------------------------
__global__ __launch_bounds__(64) void k_scan(DevChunk* chunks, DevPage* pages, const int* chunk_list,
                                             DevChunkResult* res, uint8_t* chars_arena, uint64_t arena_cap,
                                             unsigned long long* arena_used) {
    const int c = chunk_list[blockIdx.x];
    DevChunk& ck = chunks[c];
    const int lane = threadIdx.x;
    // page prefixes: 64 pages' counts loaded at once, wave scans (a serial loop put its loads in series)
    const int np = ck.n_pages, fp = ck.first_page;
    int64_t s = 0, v = 0, r = 0, ch = 0;
    for (int i0 = 0; i0 < np; i0 += 64) {
        const int i = i0 + lane;
        int64_t a[4] = {0, 0, 0, 0};
        if (i < np) { const DevPage& pg = pages[fp + i]; a[0] = pg.n_slots; a[1] = pg.n_values; a[2] = pg.n_rows; a[3] = pg.n_chars; }
        int64_t x[4] = {a[0], a[1], a[2], a[3]};
        #pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            #pragma unroll
            for (int q = 0; q < 4; q++) {
                const int64_t y = __shfl_up(x[q], d, 64);
                if (lane >= d) x[q] += y;
            }
        }
        if (i < np) {
            DevPage& pg = pages[fp + i];
            pg.slot_start = s + x[0] - a[0]; pg.value_start = v + x[1] - a[1];
            pg.row_start = r + x[2] - a[2]; pg.char_start = ch + x[3] - a[3];
        }
        s += __shfl(x[0], 63, 64); v += __shfl(x[1], 63, 64); r += __shfl(x[2], 63, 64); ch += __shfl(x[3], 63, 64);
    }
    if (lane != 0) return;
    res[c].num_slots = s; res[c].num_values = v; res[c].num_rows = r; res[c].num_chars = ch;
    if (ck.ptype == 6) {
        if (ch > int64_t(0x7fffffff)) { set_status(res, c, ST_CAPACITY, -1); ck.chars = nullptr; }
        else {
            unsigned long long need = (unsigned long long)((ch + 255) & ~int64_t(255));
            unsigned long long at = atomicAdd(arena_used, need);
            if (at + need > arena_cap) { set_status(res, c, ST_CAPACITY, -1); ck.chars = nullptr; }
            else ck.chars = chars_arena + at;
        }
        if (ck.offsets) ck.offsets[0] = 0;
    }
    if (ck.max_rep == 1 && ck.list_offsets) ck.list_offsets[r] = int32_t(s);
}

// Segment path (k_nest_*): the bytes of hybrid stream p[0, n) one segment reads, from the state at
// its first entry (a) to the next segment's (b: the header after the run holding the next segment's
// first entry; null or a sentinel = the stream's end), staged in LDS buffer buf of cap bytes. On
// success p / n become the LDS copy (stream byte lo + i at p[i]; bytes past the staged range read as
// zero but the segment's walk never needs them) and lo is returned: the caller rebases its walk
// state with rle_rebase. Returns 0 and leaves p / n alone when the range does not fit. All threads call.
__device__ __forceinline__ uint64_t stage_seg(uint32_t* buf, uint32_t cap, const uint8_t*& p, uint64_t& n,
                                              const RleState& a, const RleState* b) {
    if (a.err || n == 0 || n > 0xffffffffull) return 0;
    const uint64_t lo = (a.run_packed && a.run_left > 0) ? (a.run_bit >> 3) : a.pos;
    uint64_t hi = (b && !b->err) ? b->pos : n;
    if (lo >= n) return 0;
    hi = min<uint64_t>(n, hi + 16);
    if (hi <= lo || hi - lo + 48 > cap) return 0;
    const uint32_t off = stage_bytes(buf, p, n, uint32_t(lo), uint32_t(hi));
    __syncthreads();
    p = reinterpret_cast<const uint8_t*>(buf) + off;
    n = hi - lo;
    return lo;
}
__device__ __forceinline__ void rle_rebase(RleState& s, uint64_t lo) {
    if (lo == 0) return;
    s.pos -= lo;
    if (s.run_packed && s.run_left > 0) s.run_bit -= 8 * lo;
}

// ---- k_decode ----------------------------------------------------------------------------------
struct DecodeLds {
    LevelLds L;
    Piece pval[TILE];
    uint32_t ids[TILE];
    uint32_t vbits[TILE / 32 + 2];   // validity bits of the tile's slots (relative to aligned base)
    uint32_t lbits[TILE / 32 + 2];   // list validity bits (rows)
    uint32_t scan_tmp[NT / 64];
    RleState sval;
    int npval, verr;
};

// One segment of a nested page (k_decode_seg): its entries, where its slots / rows / chars / values
// start within the page and the rep, def and value stream states at its first entry.
struct DecodeRange {
    uint64_t e_b, e_e;
    uint64_t slot_base, row_base, char_base, vidx;
    const RleState* st;   // [3], segment-strided (st[k * nseg])
    const RleState* nx;   // the next segment's, or null
    int nseg;
    uint32_t* buf[3];     // LDS for the segment's rep / def / dictionary-id bytes (stage_seg)
};
#ifndef PF_SEG_LVL_CAP
#define PF_SEG_LVL_CAP 4096
#endif
// LDS for one segment's level / dictionary-id bytes (a segment whose bytes do not fit reads them from HBM)
constexpr uint32_t SEG_LVL_CAP = PF_SEG_LVL_CAP, SEG_VAL_CAP = 2 * PF_SEG_LVL_CAP;

__device__ __forceinline__ void decode_page(const DevChunk* __restrict__ chunks, DevPage* pages, const int pi, DevChunkResult* res,
                            DecodeLds& S, const DecodeRange* R = nullptr) {
    LevelLds& L = S.L;
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    if (pg.done != 0 || res[pg.chunk].status != 0) return;   // k_flat[_fixed] took it / an earlier stage failed this chunk
    if (!R && pg.seg_ok == 1) return;                         // k_decode_seg's
    Sections s;
    const bool ok = page_sections(pg, ck, s);
    if (tid == 0) {
        if (R) { L.srep = R->st[0]; L.sdef = R->st[R->nseg]; S.sval = R->st[2 * R->nseg]; }
        else { rle_init(L.srep); rle_init(L.sdef); rle_init(S.sval); }
        L.err = ok ? 0 : 1; S.verr = 0;
    }
    __syncthreads();
    if (L.err) { if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi); return; }

    const int enc = pg.encoding;
    const bool binary = ck.ptype == 6;
    const bool dict = is_dict_enc(enc);
    const bool boolean = ck.ptype == 0;
    const int w = ck.width;
    const bool counted = ck.needs_count != 0;
    // FIXED_LEN_BYTE_ARRAY in DELTA_BYTE_ARRAY: this pass writes validity and null slots and leaves each
    // present value's slot in aux; k_dba_chars then builds the values in value order at their slots
    const bool flba_dba = enc == 7 && ck.ptype == 7;
    // value-stream setup
    int id_bw = 0;
    if (dict) {
        id_bw = s.val_n > 0 ? int(s.val[0]) : 0;
        if (tid == 0 && !R) S.sval.pos = 1;
    } else if (boolean && enc == 3) {
        // RLE booleans: 4-byte length prefix, then a bit-width-1 hybrid stream
        if (tid == 0 && !R) S.sval.pos = 0;
    }
    const uint8_t* rle_bool_p = nullptr; uint64_t rle_bool_n = 0;
    if (boolean && enc == 3) {
        uint32_t ln = s.val_n >= 4 ? ld32le(s.val, 0, s.val_n) : 0;
        if (s.val_n < 4 || ln > s.val_n - 4) { if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi); return; }
        rle_bool_p = s.val + 4; rle_bool_n = ln;
    }
    // encoding / type support check (PLAIN, dictionary, RLE bool, DELTA_BINARY_PACKED ints, BSS)
    bool supported = false;
    if (enc == 0) supported = true;
    else if (dict) supported = !boolean && (binary ? ck.dict_pos != nullptr : ck.dict_data != nullptr);
    else if (enc == 3) supported = boolean;
    else if (enc == 5) supported = (ck.ptype == 1 || ck.ptype == 2) && pg.aux != nullptr;
    else if (enc == 9) supported = (ck.ptype == 4 || ck.ptype == 5);
    else if (enc == 6 || enc == 7) supported = (binary || (flba_dba && pg.aux != nullptr)) && pg.dx != nullptr;   // k_dlen lengths
    if (!supported) { if (tid == 0) set_status(res, pg.chunk, dict ? ST_CORRUPT : ST_ENCODING, pi); return; }
    if (dict && id_bw > 32) { if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi); return; }
    if (binary && !ck.chars) return;   // capacity error already recorded by k_scan
    if (R) {   // the segment's stream bytes in LDS: the walks below read one run header per dependent load
        const int n3 = R->nseg;
        const uint64_t lr = stage_seg(R->buf[0], SEG_LVL_CAP, s.rep, s.rep_n, R->st[0], R->nx ? &R->nx[0] : nullptr);
        const uint64_t ld = ck.max_def > 0 ? stage_seg(R->buf[1], SEG_LVL_CAP, s.def, s.def_n, R->st[n3], R->nx ? &R->nx[n3] : nullptr) : 0;
        const uint64_t lv = (dict && !binary) ? stage_seg(R->buf[2], SEG_VAL_CAP, s.val, s.val_n, R->st[2 * n3], R->nx ? &R->nx[2 * n3] : nullptr) : 0;
        if (tid == 0) { rle_rebase(L.srep, lr); rle_rebase(L.sdef, ld); rle_rebase(S.sval, lv); }
        __syncthreads();
    }

    // bases
    uint64_t slot_base = counted ? uint64_t(pg.slot_start) : uint64_t(pg.entry_start);
    uint64_t row_base = counted ? uint64_t(pg.row_start) : uint64_t(pg.entry_start);
    uint64_t char_base = counted ? uint64_t(pg.char_start) : 0;
    uint64_t vidx = 0;   // page-relative index of the next present value
    const uint64_t bss_total = (enc == 9 && w > 0) ? s.val_n / uint64_t(w) : 0;
    uint64_t e_b = 0, e_e = uint64_t(pg.num_values);
    if (R) {
        e_b = R->e_b; e_e = R->e_e;
        slot_base += R->slot_base; row_base += R->row_base; char_base += R->char_base; vidx = R->vidx;
    }

    for (uint64_t e0 = e_b; e0 < e_e; e0 += TILE) {
        uint32_t want = uint32_t(min<uint64_t>(TILE, e_e - e0));
        decode_level_tile(L, s, ck, e0, want);
        if (L.err) break;
        // per-thread: EPT consecutive entries
        const uint32_t eb = uint32_t(tid) * EPT;
        uint32_t fs = 0, fv = 0, fr = 0;   // bit flags per local entry
        #pragma unroll
        for (int k = 0; k < EPT; k++) {
            uint32_t e = eb + k;
            if (e < want) {
                int d = L.def[e];
                fs |= uint32_t(ck.max_rep == 0 || d >= ck.repeated_def) << k;
                fv |= uint32_t(d == ck.max_def) << k;
                fr |= uint32_t(L.rep[e] == 0) << k;
            }
        }
        uint32_t ts, tv, tr;
        uint32_t so = block_excl_scan<NT>(__popc(fs), S.scan_tmp, ts);
        uint32_t vo = block_excl_scan<NT>(__popc(fv), S.scan_tmp, tv);
        uint32_t ro = block_excl_scan<NT>(__popc(fr), S.scan_tmp, tr);

        // dictionary ids / RLE booleans for this tile's present values
        if ((dict || (boolean && enc == 3)) && tv > 0) {
            if (tid == 0) {
                const uint8_t* vp = dict ? s.val : rle_bool_p;
                uint64_t vn = dict ? s.val_n : rle_bool_n;
                int bw = dict ? id_bw : 1;
                if (binary && dict) S.npval = 0;   // ids were kept by k_count
                else {
                    uint32_t got = rle_walk(S.sval, vp, vn, bw, tv, S.pval, TILE, S.npval);
                    if (got != tv || S.sval.err) S.verr = 1;
                }
            }
            __syncthreads();
            if (S.verr) break;
            if (binary && dict) {
                for (uint32_t i = tid; i < tv; i += NT) S.ids[i] = pg.aux[vidx + i];
            } else {
                rle_expand<uint32_t>(S.pval, S.npval, dict ? s.val : rle_bool_p, dict ? s.val_n : rle_bool_n,
                                     dict ? id_bw : 1, S.ids);
            }
            __syncthreads();
        }
        // BYTE_ARRAY: per-slot lengths -> char offsets (scan over slots in entry order)
        uint32_t my_len[EPT];
        uint64_t my_src[EPT];
        uint32_t lsum = 0;
        if (binary) {
            uint32_t v = vo;
            #pragma unroll
            for (int k = 0; k < EPT; k++) {
                my_len[k] = 0; my_src[k] = 0;
                if ((fv >> k) & 1) {
                    uint64_t gv = vidx + v;
                    if (dict) {
                        uint32_t id = S.ids[v];
                        if (int64_t(id) < ck.dict_n) { my_src[k] = ck.dict_pos[id]; my_len[k] = ck.dict_len[id]; }
                        else S.verr = 1;
                    } else if (enc == 6 || enc == 7) {   // cpos: chars before value gv (checked by k_count)
                        const uint64_t* cpos = dx_cpos(pg.dx);
                        my_src[k] = uint64_t(pg.dx_data) + cpos[gv];
                        my_len[k] = uint32_t(cpos[gv + 1] - cpos[gv]);
                    } else {
                        uint32_t p = pg.aux[gv];
                        uint32_t l = (p >= 4 && p <= s.val_n) ? ld32le(s.val, p - 4, s.val_n) : 0xffffffffu;
                        if (l <= s.val_n - p) { my_src[k] = p; my_len[k] = l; }
                        else S.verr = 1;
                    }
                    v++;
                }
                lsum += my_len[k];
            }
        }
        uint32_t tchars = 0;
        uint32_t lo = binary ? block_excl_scan<NT>(lsum, S.scan_tmp, tchars) : 0;
        if (binary && (S.verr || char_base + tchars > uint64_t(pg.char_start + pg.n_chars))) {
            S.verr = 1;   // inconsistent with k_count's sizing: never write past this page's chars
            break;
        }

        // validity / list-validity bit staging
        const uint64_t vb0 = slot_base + 0;      // first slot of this tile
        for (uint32_t i = tid; i < TILE / 32 + 2; i += NT) { S.vbits[i] = 0; S.lbits[i] = 0; }
        __syncthreads();

        // per-entry writes
        {
            uint32_t sidx = so, vv = vo, ridx = ro;
            uint64_t cpos = char_base + lo;
            #pragma unroll
            for (int k = 0; k < EPT; k++) {
                uint32_t e = eb + k;
                if (e >= want) break;
                const bool is_slot = (fs >> k) & 1, present = (fv >> k) & 1, rstart = (fr >> k) & 1;
                if (ck.max_rep > 0) {
                    uint64_t ge = uint64_t(pg.entry_start) + e0 + e;
                    if (ck.def_levels) ck.def_levels[ge] = L.def[e];
                    if (ck.rep_levels) ck.rep_levels[ge] = L.rep[e];
                    if (rstart && ck.max_rep == 1) {
                        uint64_t row = row_base + ridx;
                        if (ck.list_offsets) ck.list_offsets[row] = int32_t(slot_base + sidx);
                        if (L.def[e] >= ck.list_null_def) {
                            uint64_t rb = row - (row_base & ~uint64_t(31));
                            atomicOr(&S.lbits[rb >> 5], 1u << (rb & 31));
                        }
                    }
                }
                if (rstart) ridx++;
                if (!is_slot) continue;
                const uint64_t slot = slot_base + sidx;
                if (present && ck.max_def > 0) {
                    uint64_t rb = slot - (vb0 & ~uint64_t(31));
                    atomicOr(&S.vbits[rb >> 5], 1u << (rb & 31));
                }
                if (binary) {
                    if (present) {
                        const uint8_t* src = dict ? ck.dict_data + my_src[k] : s.val + my_src[k];
                        if (enc != 7)   // DELTA_BYTE_ARRAY chars: k_dba_chars (values depend on their predecessor)
                            for (uint32_t j = 0; j < my_len[k]; j++) ck.chars[cpos + j] = src[j];
                        cpos += my_len[k];
                    }
                    ck.offsets[slot + 1] = int32_t(cpos);
                } else if (present) {
                    const uint64_t gv = vidx + vv;
                    uint8_t* dst = ck.values + slot * uint64_t(w);
                    if (dict) {
                        uint32_t id = S.ids[vv];
                        if (int64_t(id) >= ck.dict_n) { S.verr = 1; }
                        else copy_value(dst, ck.dict_data + uint64_t(id) * w, w);
                    } else if (boolean) {
                        uint32_t b = (enc == 3) ? S.ids[vv] : ((ld8(s.val, gv >> 3, s.val_n) >> (gv & 7)) & 1);
                        if (enc == 0 && (gv >> 3) >= s.val_n) S.verr = 1;
                        dst[0] = uint8_t(b);
                    } else if (enc == 0) {
                        if ((gv + 1) * uint64_t(w) > s.val_n) S.verr = 1;
                        else copy_value(dst, s.val + gv * w, w);
                    } else if (enc == 5) {
                        const uint64_t* dv = reinterpret_cast<const uint64_t*>(pg.aux);
                        if (w == 8) *reinterpret_cast<uint64_t*>(dst) = dv[gv];
                        else *reinterpret_cast<uint32_t*>(dst) = uint32_t(dv[gv]);
                    } else if (enc == 9) {
                        if (gv >= bss_total) S.verr = 1;
                        else for (int b = 0; b < w; b++) dst[b] = s.val[uint64_t(b) * bss_total + gv];
                    } else if (flba_dba) {
                        if (gv < uint64_t(pg.aux_cap)) pg.aux[gv] = uint32_t(slot);
                        else S.verr = 1;
                    }
                } else {
                    zero_value(ck.values + slot * uint64_t(w), w);
                }
                if (present) vv++;
                sidx++;
            }
        }
        __syncthreads();
        if (S.verr) break;
        if (ck.max_def > 0 && ck.validity) flush_bits(S.vbits, vb0, ts, ck.validity);
        if (ck.max_rep == 1 && ck.list_validity) flush_bits(S.lbits, row_base, tr, ck.list_validity);
        slot_base += ts;
        row_base += tr;
        char_base += tchars;
        vidx += tv;
        __syncthreads();
    }
    if (L.err || S.verr) { if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi); return; }
    if (flba_dba) {   // the page's present values against k_dlen's streams and checks (as count_page does for BYTE_ARRAY)
        if (int64_t(vidx) > pg.dx_total || int64_t(vidx) > pg.dx_bad) { if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi); return; }
        if (tid == 0) pg.n_values = int64_t(vidx);   // k_dba_chars' value count (flat pages are not counted)
    }
    if (!counted && tid == 0) atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values),
                                        (unsigned long long)vidx);
}

// Pages the flat kernels did not take (nested, DELTA_LENGTH / DELTA_BYTE_ARRAY, RLE booleans, BSS,
// anything they rejected). Grid-stride over the batch's page list with a grid sized by the host to
// the pages that will need it (listed first): most blocks find their pages done, and a launch of
// one large-LDS block per page would wait for CUs that other streams' kernels hold.
__global__ __launch_bounds__(NT) void k_decode(const DevChunk* __restrict__ chunks, DevPage* pages,
                                               const int* page_list, int n, DevChunkResult* res) {
    __shared__ DecodeLds S;
    // (decode_page's own early exits, tested for a block's pages at once)
    stride_pages(page_list, n,
                 [&](int pi) { const DevPage& pg = pages[pi]; return (pg.done == 0) & (pg.seg_ok != 1) & (res[pg.chunk].status == 0); },
                 [&](int pi) { decode_page(chunks, pages, pi, res, S); });
}

// ---- nested pages in segments (k_nest_*) --------------------------------------------------------
// A nested page's levels are walked run by run from its first entry, so k_count / k_decode take it in
// ONE workgroup tile after tile: a 520K-entry page (one per chunk in config 5) runs ~1000 tiles in
// series on one CU. Here the page is cut into segments of seg_len entries, each decoded by its own
// workgroup from checkpoints of the three hybrid streams (rep, def, dictionary ids):
//   k_nest_lvl   (page x {rep, def} x 8 KiB window): every window position decoded as a run header,
//                pointer jumping to the window exits, a single-pass hand-over between windows, and
//                the state at every segment start;
//   k_count_seg  (page x segment): slots / values / rows of the segment's levels;
//   k_nest_scan  (page, one wave): their prefixes over the page, the page totals (k_scan), and the
//                dictionary-id stream's state at each segment's first value;
//   k_nest_ids   (page x segment, BYTE_ARRAY dictionary): ids kept for k_decode_seg, chars;
//   k_nest_chars (page, one wave): the segments' chars prefix, the page's chars;
//   k_decode_seg (page x segment): decode_page over the segment.
// Checkpoint states are exactly rle_walk's state after the segment's first t values (mid-run when t
// falls inside a run), so each segment's decode is the serial walk's, from t on.
constexpr uint32_t NW_BYTES = 8192;   // nest_walk's LDS window over a stream (k_nest_scan)
static_assert(sizeof(RleState) == NEST_CK_BYTES, "checkpoint size (host plans the segment tables)");

__device__ __forceinline__ RleState* nest_ck(const DevPage& pg, int k) {
    return reinterpret_cast<RleState*>(pg.seg) + size_t(k) * size_t(pg.nseg);
}
__device__ __forceinline__ SegRec* nest_rec(const DevPage& pg) {
    return reinterpret_cast<SegRec*>(pg.seg + 3ull * NEST_CK_BYTES * uint64_t(pg.nseg));
}
__device__ __forceinline__ RleState rle_sentinel() {   // a target the stream never reached: walking from it fails
    RleState s;
    rle_init(s);
    s.pos = ~uint64_t(0);
    s.err = 1;
    return s;
}

// One wave: walk the hybrid stream p[0, n) (bit width bw) from byte pos0 (a run header), and store in
// out[k] the state after target(k) values, k < nt (targets non-decreasing). Targets the stream does
// not reach (it ends, breaks, or holds fewer values) get rle_sentinel(). All lanes walk in step (the
// LDS reads broadcast); lane 0 writes.
template <typename Target>
__device__ void nest_walk(uint32_t* st, const uint8_t* p, uint64_t n, int bw, uint64_t pos0, int nt, Target target,
                          RleState* out) {
    const int lane = threadIdx.x & 63;
    int k = 0;
    uint64_t e = 0, pos = pos0;
    uint64_t wb = ~uint64_t(0);   // stream offset of the window's first byte (st byte woff)
    uint32_t woff = 0;
    const uint8_t* W = reinterpret_cast<const uint8_t*>(st);
    const int nbv = (bw + 7) >> 3;
    uint64_t t = nt > 0 ? target(0) : 0;
    while (k < nt && pos < n) {
        if (wb == ~uint64_t(0) || pos < wb || pos + 16 > wb + NW_BYTES) {
            __syncthreads();
            wb = pos;
            woff = stage_bytes(st, p, n, uint32_t(pos), uint32_t(min<uint64_t>(n, pos + NW_BYTES)));
            __syncthreads();
        }
        // header (uvarint, <= 10 bytes) and an RLE value (<= 4 bytes) lie inside the window
        const uint8_t* q = W + woff + (pos - wb);
        uint64_t h = 0;
        uint32_t hl = 0;
        bool hok = false;
        for (uint32_t sh = 0; sh < 70; sh += 7) {
            if (pos + hl >= n) break;
            const uint32_t c = q[hl++];
            h |= uint64_t(c & 0x7f) << sh;
            if (!(c & 0x80)) { hok = true; break; }
        }
        if (!hok) break;
        const uint64_t a = pos + hl;
        uint64_t cnt, next, bit0 = 0;
        uint32_t val = 0;
        const uint32_t packed = uint32_t(h & 1);
        if (packed) {
            const uint64_t groups = h >> 1;
            cnt = groups * 8;
            bit0 = a * 8;
            const uint64_t nb = groups * uint64_t(bw), avail = n - a;
            next = a + (nb < avail ? nb : avail);
        } else {
            cnt = h >> 1;
            if (a + nbv > n) break;
            for (int b = 0; b < nbv; b++) val |= uint32_t(q[hl + b]) << (8 * b);
            next = a + nbv;
        }
        while (k < nt && t < e + cnt) {
            if (lane == 0) {
                RleState r;
                r.pos = next;
                r.run_left = e + cnt - t;
                r.run_bit = packed ? bit0 + (t - e) * uint64_t(bw) : 0;
                r.run_val = val;
                r.run_packed = int32_t(packed);
                r.err = 0;
                out[k] = r;
            }
            k++;
            if (k < nt) t = target(k);
        }
        e += cnt;
        pos = next;
    }
    for (; k < nt; k++)
        if (lane == 0) out[k] = rle_sentinel();
}

// the page's segment path applies: rep / def sections parse and are RLE hybrid streams
__device__ __forceinline__ bool nest_sections(const DevPage& pg, const DevChunk& ck, Sections& s) {
    return pg.seg != nullptr && ck.max_rep > 0 && page_sections(pg, ck, s) && s.rep_rle && (ck.max_def == 0 || s.def_rle);
}

// One hybrid-stream run header at stream position p (q = its bytes, >= 14 readable): false when p
// holds no run the serial walk (rle_walk) would accept.
struct HybRun {
    uint64_t cnt, next, bit0;
    uint32_t val, packed;
};
__device__ __forceinline__ bool hyb_header(const uint8_t* q, uint64_t p, uint64_t n, int bw, HybRun& r) {
    uint64_t h = 0;
    uint32_t hl = 0;
    bool hok = false;
    for (uint32_t sh = 0; sh < 70; sh += 7) {
        if (p + hl >= n) break;
        const uint32_t c = q[hl++];
        h |= uint64_t(c & 0x7f) << sh;
        if (!(c & 0x80)) { hok = true; break; }
    }
    if (!hok) return false;
    const uint64_t a = p + hl;
    r.packed = uint32_t(h & 1);
    r.val = 0;
    r.bit0 = 0;
    if (r.packed) {
        const uint64_t groups = h >> 1;
        r.cnt = groups * 8;
        r.bit0 = a * 8;
        const uint64_t nb = groups * uint64_t(bw), avail = n - a;
        r.next = a + (nb < avail ? nb : avail);
    } else {
        const int nbv = (bw + 7) >> 3;
        r.cnt = h >> 1;
        if (a + nbv > n) return false;
        for (int b = 0; b < nbv; b++) r.val |= uint32_t(q[hl + b]) << (8 * b);
        r.next = a + nbv;
    }
    return true;
}
__device__ __forceinline__ RleState hyb_state(const HybRun& r, uint64_t e_start, uint64_t t, int bw) {
    RleState x;
    x.pos = r.next;
    x.run_left = e_start + r.cnt - t;
    x.run_bit = r.packed ? r.bit0 + (t - e_start) * uint64_t(bw) : 0;
    x.run_val = r.val;
    x.run_packed = int32_t(r.packed);
    x.err = 0;
    return x;
}

// k_nest_lvl: NL_NT threads per NEST_WIN-byte window of a page's rep or def stream. Run headers can
// only be found by walking from the stream's start, so every byte position of the window is decoded
// as a header at once, and pointer jumping (log2(NEST_WIN) rounds in LDS) gives, for every position,
// where the chain from it leaves the window and the entries it covers on the way (north_star K2: run
// boundaries by parallel scans). The true chain's entry position and count then come from the
// previous window (single-pass hand-over through npub: one lookup per window on the critical path),
// and the window walks its part of the true chain to store the checkpoints inside it (states at
// multiples of seg_len entries) after publishing its exit.
constexpr int NL_NT = 256;
constexpr uint32_t NL_END = 0xFFFFFFu;        // exit field: the chain ends inside the window (no run at its last position)
constexpr uint32_t NL_FAR = 0xFFFFFEu;        // exit field: leaves the window for a position >= w0 + NL_FAR (exact exit by a walk)
constexpr uint64_t NL_CMAX = (1ull << 40) - 1;   // count field saturates (the exact count is then walked)
constexpr uint32_t NL_JNONE = 0xFFFu, NL_JCMAX = 0xFFFFFu;   // J: no exit inside the window; saturated entries
static_assert(NEST_WIN <= 2048, "J packs window-relative exits in 12 bits");
__global__ __launch_bounds__(NL_NT) void k_nest_lvl(const DevChunk* __restrict__ chunks, DevPage* pages, const int* __restrict__ list,
                                                    DevChunkResult* res, uint32_t spin_cap) {
    __shared__ __attribute__((aligned(16))) uint32_t st[(NEST_WIN + 64) / 4];
    __shared__ uint64_t X[NEST_WIN];   // per position: entries to the exit << 24 | exit (window-relative, NL_END, NL_FAR)
    // the same after 5 rounds, packed in 32 bits: jumps over >= 32 runs (or to the exit), for the checkpoint
    // walk; exit in the low 12 bits (NL_JNONE: none inside the window), entries (saturating) above
    __shared__ uint32_t J[NEST_WIN];
    __shared__ uint64_t s_hand[3];
    const int tid = threadIdx.x;
    const int pi = list[blockIdx.z];
    const int which = blockIdx.y;   // 0 = rep, 1 = def
    const uint32_t w = blockIdx.x;
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    Sections s;
    if (res[pg.chunk].status != 0 || !nest_sections(pg, ck, s) || w >= uint32_t(pg.nwin)) return;   // (seg_ok stays 0)
    const int nseg = pg.nseg;
    const uint64_t sl = uint64_t(uint32_t(pg.seg_len));
    RleState* out = nest_ck(pg, which);
    // (max: a window that timed out waiting for its hand-over may already have set 2 = failed)
    if (which == 0 && w == 0 && tid == 0) __hip_atomic_fetch_max(&pg.seg_ok, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (which == 1 && ck.max_def == 0) {
        if (w == 0) for (int k = tid; k < nseg; k += NL_NT) { RleState r; rle_init(r); out[k] = r; }
        return;
    }
    const uint8_t* p = which == 0 ? s.rep : s.def;
    const uint64_t n = which == 0 ? s.rep_n : s.def_n;
    const int bw = bit_width(uint32_t(which == 0 ? ck.max_rep : ck.max_def));
    const uint64_t w0 = uint64_t(w) * NEST_WIN, w1 = w0 + NEST_WIN;
    if (w0 >= n && w > 0) return;                  // past the stream (no one waits on it)
    const bool last = w1 >= n;                     // writes the sentinels of targets the chain never reached
    WinPub* pub = pg.npub + size_t(which) * size_t(pg.nwin);
    // ---- stage the window (+ 16 bytes: a header and an RLE value that start inside it) ----
    const uint32_t woff = stage_bytes(st, p, n, uint32_t(min<uint64_t>(w0, n)), uint32_t(min<uint64_t>(w1 + 16, n)));
    __syncthreads();
    const uint8_t* W = reinterpret_cast<const uint8_t*>(st) + woff;   // W[i] = stream byte w0 + i
    // ---- every position as a header, then pointer jumping to the window's exit ----
    for (uint32_t i = tid; i < NEST_WIN; i += NL_NT) {
        const uint64_t pp = w0 + i;
        HybRun r;
        uint64_t x = NL_END;
        if (pp < n && hyb_header(W + i, pp, n, bw, r)) {
            const uint64_t rel = r.next - w0;
            x = (min<uint64_t>(r.cnt, NL_CMAX) << 24) | (rel < NL_FAR ? rel : uint64_t(NL_FAR));
        }
        X[i] = x;
    }
    __syncthreads();
    for (uint32_t span = 1; span < NEST_WIN; span <<= 1) {
        for (uint32_t i = tid; i < NEST_WIN; i += NL_NT) {
            const uint64_t x = X[i];
            const uint32_t e = uint32_t(x & 0xFFFFFFu);
            if (e < NEST_WIN) {   // (in place: a successor already advanced this round only jumps further)
                const uint64_t y = X[e];
                const uint64_t c = min<uint64_t>((x >> 24) + (y >> 24), NL_CMAX);
                X[i] = (c << 24) | (y & 0xFFFFFFu);
            }
        }
        __syncthreads();
        if (span == 16) {
            for (uint32_t i = tid; i < NEST_WIN; i += NL_NT) {
                const uint64_t x = X[i];
                const uint32_t e = uint32_t(x & 0xFFFFFFu);
                J[i] = (e < NEST_WIN ? e : NL_JNONE) | (uint32_t(min<uint64_t>(x >> 24, NL_JCMAX)) << 12);
            }
        }
    }
    __syncthreads();
    // ---- the true chain's entry from the previous window; exit to the next ----
    if (tid == 0) {
        uint64_t tp = 0, te = 0;
        uint32_t tst = 0;
        bool ok = true;
        // bounded (spin_cap: 2^22; the diagnostics option nest_timeout makes it 0, so every hand-over
        // "times out"): a hand-over that never comes sends the page to the whole-page path (below)
        // instead of hanging
        if (w > 0) ok = winpub_get(pub[w - 1], spin_cap, tp, te, tst);
        s_hand[0] = tp; s_hand[1] = te; s_hand[2] = uint64_t(tst) | (ok ? 0u : 2u);
        uint64_t xp = tp, xe = te;
        uint32_t xst = tst;
        if (ok && tst == 0 && tp < w1) {
            const uint64_t x = X[tp - w0];
            const uint32_t e = uint32_t(x & 0xFFFFFFu);
            const uint64_t c = x >> 24;
            if (e == NL_FAR || c == NL_CMAX) {   // exact exit / count by walking (a run of > 16 MB, or counts near 2^40)
                while (xp < w1) {
                    HybRun r;
                    if (xp >= n || !hyb_header(W + (xp - w0), xp, n, bw, r)) { xst = 1; break; }
                    xe += r.cnt;
                    xp = r.next;
                }
            } else {
                xe = te + c;
                if (e == NL_END) { xst = 1; xp = w1; }   // (where it ended does not matter once it has)
                else xp = w0 + e;
            }
        }
        // a hand-over that never came (a scheduling stall, not the data): the page leaves the segment
        // path and k_count / k_decode decode it whole, as k_dbp_pos does with dbp_ok = 2
        if (!ok) __hip_atomic_fetch_max(&pg.seg_ok, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // a failed hand-over is published as the overflow word, so every later window fails at once
        winpub_put(pub[w], ok ? xp : ~0ull, xe, xst);
    }
    __syncthreads();
    if (s_hand[2] & 2u) return;
    // ---- checkpoints inside the window: one wave walks its part of the true chain ----
    uint64_t tp = s_hand[0], te = s_hand[1];
    uint32_t tst = uint32_t(s_hand[2]);
    if (tid < 64) {   // (all 64 lanes walk in step; lane 0 stores)
        uint64_t k = (te + sl - 1) / sl;   // first target >= te
        if (tst == 0) {
            while (k < uint64_t(nseg) && tp < w1) {
                const uint64_t t = k * sl;
                // jump over runs before the target: >= 32 at a time
                while (true) {
                    const uint32_t x = J[tp - w0];
                    const uint32_t e = x & 0xFFFu, c = x >> 12;
                    if (e >= NEST_WIN || c == NL_JCMAX || te + c > t) break;   // (saturated: the header walk)
                    te += c;
                    tp = w0 + e;
                }
                HybRun r;
                if (tp >= n || !hyb_header(W + (tp - w0), tp, n, bw, r)) { tst = 1; break; }
                if (t < te + r.cnt) {   // the target's run
                    if (tid == 0) out[k] = hyb_state(r, te, t, bw);
                    k++;
                    continue;
                }
                te += r.cnt;
                tp = r.next;
            }
        }
        // targets the chain never reached: the stream's last window, or the window where it ended
        if (last || tst == 1)
            for (uint64_t q = k + tid; q < uint64_t(nseg); q += 64) out[q] = rle_sentinel();
    }
}

__global__ __launch_bounds__(NT) void k_count_seg(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                  const int2* __restrict__ list, DevChunkResult* res) {
    __shared__ LevelLds L;
    __shared__ uint32_t scan_tmp[NT / 64];
    const int pi = list[blockIdx.x].x, sg = list[blockIdx.x].y;
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    if (pg.seg_ok != 1 || res[pg.chunk].status != 0) return;
    __shared__ uint32_t bufR[SEG_LVL_CAP / 4], bufD[SEG_LVL_CAP / 4];
    Sections s;
    page_sections(pg, ck, s);   // (parsed by k_nest_lvl)
    const uint64_t e_b = uint64_t(sg) * uint32_t(pg.seg_len);
    const uint64_t e_e = min<uint64_t>(uint64_t(pg.num_values), e_b + uint32_t(pg.seg_len));
    {
        const RleState* cr = nest_ck(pg, 0);
        const RleState* cd = nest_ck(pg, 1);
        const bool last = sg + 1 >= pg.nseg;
        const uint64_t lr = stage_seg(bufR, SEG_LVL_CAP, s.rep, s.rep_n, cr[sg], last ? nullptr : &cr[sg + 1]);
        const uint64_t ld = ck.max_def > 0 ? stage_seg(bufD, SEG_LVL_CAP, s.def, s.def_n, cd[sg], last ? nullptr : &cd[sg + 1]) : 0;
        if (threadIdx.x == 0) {
            L.srep = cr[sg]; L.sdef = cd[sg]; L.err = 0;
            rle_rebase(L.srep, lr); rle_rebase(L.sdef, ld);
        }
    }
    __syncthreads();
    uint64_t slots = 0, vals = 0, rows = 0;
    for (uint64_t e0 = e_b; e0 < e_e; e0 += TILE) {
        const uint32_t want = uint32_t(min<uint64_t>(TILE, e_e - e0));
        decode_level_tile(L, s, ck, e0, want);
        if (L.err) break;
        uint32_t ns = 0, nv = 0, nr = 0;
        for (uint32_t i = threadIdx.x; i < want; i += NT) {
            const int d = L.def[i];
            ns += d >= ck.repeated_def;
            nv += d == ck.max_def;
            nr += L.rep[i] == 0;
        }
        uint32_t t;
        block_excl_scan<NT>(ns, scan_tmp, t); slots += t;
        block_excl_scan<NT>(nr, scan_tmp, t); rows += t;
        block_excl_scan<NT>(nv, scan_tmp, t); vals += t;
        __syncthreads();
    }
    if (L.err) { if (threadIdx.x == 0) set_status(res, pg.chunk, ST_CORRUPT, pi); return; }
    if (threadIdx.x == 0) {
        SegRec& r = nest_rec(pg)[sg];
        r.ns = uint32_t(slots); r.nv = uint32_t(vals); r.nr = uint32_t(rows); r.chars = 0;
    }
}

__global__ __launch_bounds__(64) void k_nest_scan(const DevChunk* __restrict__ chunks, DevPage* pages, const int* __restrict__ list,
                                                  DevChunkResult* res) {
    __shared__ __attribute__((aligned(16))) uint32_t st[(NW_BYTES + 64) / 4];
    __shared__ uint32_t vb[NEST_MAX_SEGS];
    const int pi = list[blockIdx.x];
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    if (pg.seg_ok != 1 || res[pg.chunk].status != 0) return;
    const int nseg = pg.nseg, lane = threadIdx.x;
    SegRec* R = nest_rec(pg);
    uint64_t cs = 0, cv = 0, cr = 0;
    for (int k0 = 0; k0 < nseg; k0 += 64) {
        const int k = k0 + lane;
        uint64_t ns = 0, nv = 0, nr = 0;
        if (k < nseg) { ns = R[k].ns; nv = R[k].nv; nr = R[k].nr; }
        uint64_t xs = ns, xv = nv, xr = nr;
        #pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t ys = __shfl_up(xs, d, 64), yv = __shfl_up(xv, d, 64), yr = __shfl_up(xr, d, 64);
            if (lane >= d) { xs += ys; xv += yv; xr += yr; }
        }
        if (k < nseg) {
            R[k].sb = uint32_t(cs + xs - ns); R[k].vb = uint32_t(cv + xv - nv); R[k].rb = uint32_t(cr + xr - nr);
            vb[k] = uint32_t(cv + xv - nv);
        }
        cs += __shfl(xs, 63, 64); cv += __shfl(xv, 63, 64); cr += __shfl(xr, 63, 64);
    }
    if (lane == 0) { pg.n_slots = int64_t(cs); pg.n_values = int64_t(cv); pg.n_rows = int64_t(cr); pg.n_chars = 0; }
    __syncthreads();
    // dictionary ids: the stream's state at each segment's first value
    if (is_dict_enc(pg.encoding)) {
        Sections s;
        page_sections(pg, ck, s);
        RleState* out = nest_ck(pg, 2);
        const int id_bw = s.val_n > 0 ? int(s.val[0]) : 0;
        if (s.val_n == 0 || id_bw > 32) {
            for (int k = lane; k < nseg; k += 64) out[k] = rle_sentinel();   // (decode reports it)
        } else {
            nest_walk(st, s.val, s.val_n, id_bw, 1, nseg, [](int k) { return uint64_t(vb[k]); }, out);
        }
    }
}

__global__ __launch_bounds__(NT) void k_nest_ids(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                 const int2* __restrict__ list, DevChunkResult* res) {
    __shared__ Piece pval[TILE];
    __shared__ uint32_t ids[TILE];
    __shared__ RleState sval;
    __shared__ int npval, verr;
    __shared__ unsigned long long chars_acc;
    const int pi = list[blockIdx.x].x, sg = list[blockIdx.x].y;
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    if (pg.seg_ok != 1 || res[pg.chunk].status != 0 || ck.ptype != 6 || !is_dict_enc(pg.encoding)) return;
    Sections s;
    page_sections(pg, ck, s);
    SegRec& rec = nest_rec(pg)[sg];
    const uint64_t v_b = rec.vb, v_e = v_b + rec.nv;
    const int id_bw = s.val_n > 0 ? int(s.val[0]) : 0;
    __shared__ uint32_t bufV[SEG_VAL_CAP / 4];
    const RleState* cv = nest_ck(pg, 2);
    const uint64_t lv = v_e > v_b ? stage_seg(bufV, SEG_VAL_CAP, s.val, s.val_n, cv[sg], sg + 1 < pg.nseg ? &cv[sg + 1] : nullptr) : 0;
    if (threadIdx.x == 0) { sval = cv[sg]; rle_rebase(sval, lv); verr = 0; chars_acc = 0; }
    __syncthreads();
    for (uint64_t v0 = v_b; v0 < v_e; v0 += TILE) {
        const uint32_t t = uint32_t(min<uint64_t>(TILE, v_e - v0));
        if (threadIdx.x == 0) {
            if (id_bw > 32 || !ck.dict_len) verr = 1;
            else {
                const uint32_t got = rle_walk(sval, s.val, s.val_n, id_bw, t, pval, TILE, npval);
                if (got != t || sval.err) verr = 1;
            }
        }
        __syncthreads();
        if (verr) break;
        rle_expand<uint32_t>(pval, npval, s.val, s.val_n, id_bw, ids);
        __syncthreads();
        uint64_t acc = 0;
        int bad = 0;
        for (uint32_t i = threadIdx.x; i < t; i += NT) {
            const uint32_t id = ids[i];
            if (int64_t(id) >= ck.dict_n) { bad = 1; continue; }
            acc += ck.dict_len[id];
            pg.aux[v0 + i] = id;
        }
        if (__syncthreads_or(bad)) { if (threadIdx.x == 0) verr = 1; __syncthreads(); break; }
        atomicAdd(&chars_acc, (unsigned long long)acc);
        __syncthreads();
    }
    if (verr) { if (threadIdx.x == 0) set_status(res, pg.chunk, ST_CORRUPT, pi); return; }
    __syncthreads();
    if (threadIdx.x == 0) rec.chars = chars_acc;
}

__global__ __launch_bounds__(64) void k_nest_chars(const DevChunk* __restrict__ chunks, DevPage* pages, const int* __restrict__ list,
                                                   DevChunkResult* res) {
    const int pi = list[blockIdx.x];
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    if (pg.seg_ok != 1 || res[pg.chunk].status != 0 || ck.ptype != 6) return;
    const int nseg = pg.nseg, lane = threadIdx.x;
    SegRec* R = nest_rec(pg);
    uint64_t cc = 0;
    for (int k0 = 0; k0 < nseg; k0 += 64) {
        const int k = k0 + lane;
        const uint64_t c = k < nseg ? R[k].chars : 0;
        uint64_t x = c;
        #pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (k < nseg) R[k].cb = cc + x - c;
        cc += __shfl(x, 63, 64);
    }
    if (lane == 0) pg.n_chars = int64_t(cc);
}

#ifndef PF_DSEG_WAVES
#define PF_DSEG_WAVES 4
#endif
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(PF_DSEG_WAVES))) void k_decode_seg(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                   const int2* __restrict__ list, DevChunkResult* res) {
    __shared__ DecodeLds S;
    __shared__ uint32_t bufR[SEG_LVL_CAP / 4], bufD[SEG_LVL_CAP / 4], bufV[SEG_VAL_CAP / 4];
    const int pi = list[blockIdx.x].x, sg = list[blockIdx.x].y;
    const DevPage& pg = pages[pi];
    if (pg.seg_ok != 1) return;
    const SegRec& rec = nest_rec(pg)[sg];
    DecodeRange R;
    R.e_b = uint64_t(sg) * uint32_t(pg.seg_len);
    R.e_e = min<uint64_t>(uint64_t(pg.num_values), R.e_b + uint32_t(pg.seg_len));
    R.slot_base = rec.sb; R.row_base = rec.rb; R.vidx = rec.vb;
    R.char_base = chunks[pg.chunk].ptype == 6 ? rec.cb : 0;
    R.st = nest_ck(pg, 0) + sg;
    R.nx = sg + 1 < pg.nseg ? R.st + 1 : nullptr;
    R.nseg = pg.nseg;
    R.buf[0] = bufR; R.buf[1] = bufD; R.buf[2] = bufV;
    decode_page(chunks, pages, pi, res, S, &R);
}

// ---- launchers -------------------------------------------------------------------------------
void launch_nest_lvl(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, int max_nwin, DevChunkResult* d_res,
                     hipStream_t st, bool force_timeout) {
    // windows in blockIdx.x: a window waits on the one before it, which the dispatcher starts first
    if (n > 0 && max_nwin > 0)
        hipLaunchKernelGGL(k_nest_lvl, dim3(max_nwin, 2, n), dim3(NL_NT), 0, st, d_chunks, d_pages, d_list, d_res,
                           force_timeout ? 0u : (1u << 22));
}
void launch_nest_count(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, const int2* d_segs, int n_segs,
                       DevChunkResult* d_res, hipStream_t st) {
    if (n <= 0 || n_segs <= 0) return;
    hipLaunchKernelGGL(k_count_seg, dim3(n_segs), dim3(NT), 0, st, d_chunks, d_pages, d_segs, d_res);
    hipLaunchKernelGGL(k_nest_scan, dim3(n), dim3(64), 0, st, d_chunks, d_pages, d_list, d_res);
    hipLaunchKernelGGL(k_nest_ids, dim3(n_segs), dim3(NT), 0, st, d_chunks, d_pages, d_segs, d_res);
    hipLaunchKernelGGL(k_nest_chars, dim3(n), dim3(64), 0, st, d_chunks, d_pages, d_list, d_res);
}
void launch_nest_decode(const DevChunk* d_chunks, DevPage* d_pages, const int2* d_segs, int n_segs, DevChunkResult* d_res,
                        hipStream_t st) {
    if (n_segs > 0) hipLaunchKernelGGL(k_decode_seg, dim3(n_segs), dim3(NT), 0, st, d_chunks, d_pages, d_segs, d_res);
}
void launch_count(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res, BaJob* d_bajobs,
                  hipStream_t st, int idle_grid) {
    // d_list: every page that needs counts; the ones launch_count_flat (pf_flat_count.hip, before this on the
    // stream) counted are skipped by their pg.counted mark
    if (n > 0) hipLaunchKernelGGL(k_count, dim3(std::min(n, idle_grid)), dim3(NT), 0, st, d_chunks, d_pages, d_list, n, d_res, d_bajobs);
}
void launch_scan(DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res,
                 uint8_t* arena, uint64_t cap, unsigned long long* used, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_scan, dim3(n), dim3(64), 0, st, d_chunks, d_pages, d_list, d_res, arena, cap, used);
}
void launch_decode(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, int n_first,
                   DevChunkResult* d_res, hipStream_t st, int idle_grid) {
    // n_first: pages at the head of the list that will need k_decode (host-known); the rest are
    // checked by the stride loop, which is nearly always idle: idle_grid blocks (each needs ~23 KiB of
    // LDS, and the launch ends only once every block has found a CU)
    const int g = std::min(n, std::max(idle_grid, n_first));
    if (n > 0) hipLaunchKernelGGL(k_decode, dim3(g), dim3(NT), 0, st, d_chunks, d_pages, d_list, n, d_res);
}

}  // namespace pf
