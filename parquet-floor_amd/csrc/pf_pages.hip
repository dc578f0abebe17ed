// pf_pages.hip — the fast path for data pages of flat columns (max_rep == 0) on gfx950.
//
// Replaces, for the pages it takes, the per-value work parquet-mr 1.12.2 does behind ColumnReader
// (called from src/main/java/blue/strategic/parquet/ParquetReader.java:141-168): the hybrid
// expansion of definition levels and dictionary ids (RunLengthBitPackingHybridDecoder,
// DictionaryValuesReader), the dictionary gather (PlainValuesDictionary.decodeToX), the PLAIN
// fixed-width and BYTE_ARRAY readers, and the def == maxDef null test of ParquetReader.java:146.
// A page it does not take keeps done == 0 and is decoded by k_decode (pf_decode.hip).
//
// Kernels (pages are cut into blocks of FBLK entries, pf_internal.h):
//   k_runs         per dictionary page: the id run table, walked once for all of the page's blocks,
//                  and whether every level is present
//   k_count_dict   per (page, block) of dictionary BYTE_ARRAY pages: the block's chars
//   k_count_flat   per all-present BYTE_ARRAY page: counts, chars bases of the blocks; PLAIN pages
//                  hand their value chain to the k_ba walk (pf_ba.hip)
//   k_lvl          per nullable fixed-width page: level run table and values before each block
//   k_flat_null<4|8>  per (page, block) with nulls, fixed width: null scatter from k_lvl's tables
//   k_flat_fixed   per (page, block), fixed width, all present
//   k_flat_dstr    per (page, block) of dictionary BYTE_ARRAY pages with a small dictionary of short values, all present
//   k_flat_all     per (page, block): every other flat page (BYTE_ARRAY, booleans, ...), and the
//                  fallback queue of blocks k_flat_null and k_flat_fixed did not take
//   k_page_null    (diagnostics build) k_lvl + k_flat_null for a whole page in one workgroup
//   k_debug_walk   (diagnostics build) wave_walk_runs against a one-lane reference walk
#include <hip/hip_runtime.h>

#include "pf_dstr_ids.h"
#include "pf_launch.h"
#include "pf_pages.h"
#include "pf_snappy_par.h"   // FB_WHOLE: what the Snappy executor wrote straight into the column

namespace pf {

// Phase stamps of -DPF_STAMPS builds (tools/probe_flat_all.py, tools/probe_wide.py): cycle sums
// per slot. A __device__ array belongs to one unit, so only this unit's kernels stamp.
#ifdef PF_STAMPS
#include "pf_stamps.h"   // (a macro only: nothing of it lands in this namespace)
PF_STAMP_TABLE(pf_pstamps, 16, pf_debug_pstamps)
#define PSTAMP(i, v) atomicAdd(&pf_pstamps[i], (unsigned long long)(v))
#else
#define PSTAMP(i, v) ((void)0)
#endif

// ---- k_flat: data pages of flat columns (max_rep == 0) ------------------------------------------
// The same per-value work as k_decode, organised for throughput. The definition-level and
// dictionary-id run headers of the page are walked ONCE (one lane of wave 0 and one of wave 1,
// concurrently) into LDS run tables; tiles of FT entries then expand them by binary search with no
// serial section, one workgroup scan for the value index (none when the page has no nulls) and one
// for BYTE_ARRAY char offsets. BYTE_ARRAY chars are copied cooperatively, one 16-byte output chunk
// per thread step (coalesced stores), instead of a byte loop per value.
// Pages it does not take (run tables full, BIT_PACKED levels, RLE booleans, BYTE_STREAM_SPLIT,
// corrupt section layout) keep done == 0 and are decoded by k_decode.
#ifndef PF_FT
#define PF_FT 2048   // r04 (string path; the fixed-width path has FTX): SF1 2.896-2.899 vs 2.938-2.953 ms with
                     // 1024 (profiles/r04_ab/tune.txt). r02, one tile size for both paths: 1024 beat 2048 (3.82 vs 3.94)
#endif
constexpr int FT = PF_FT;            // entries per tile (fewer registers per thread, more blocks resident)
constexpr int FEPT = FT / NT;        // consecutive entries per thread
static_assert(FT <= int(FBLK) && FBLK % FT == 0 && FEPT <= 32, "tiles divide blocks; a thread's entries fit a 32-bit mask");
#ifndef PF_FTX
#define PF_FTX 2048   // SF1 2.936 / 2.936 ms vs 3.000-3.019 with 1024 (4096: 2.93, scratch for the arrays)
#endif
constexpr int FTX = PF_FTX;          // tile of the all-present fixed-width path (flat_present_fixed): its
                                     // tiles' id loads and gathers per thread in flight together
constexpr int FEPTX = FTX / NT;
static_assert(FTX <= int(FBLK) && FBLK % FTX == 0, "fixed-width tiles divide blocks");
constexpr uint32_t DSTR_CAP = 256;   // string dictionaries up to this many entries: {pos, len} staged in LDS

// One 128-thread workgroup per dictionary data page of a flat chunk: walks the page's
// dictionary-id run headers ONCE (wave 1) and checks whether every definition level is present
// (wave 0), so that k_flat's blocks of the page load a ready run table instead of each walking
// the headers from the page start.
__global__ __launch_bounds__(128) void k_runs(const DevChunk* __restrict__ chunks, DevPage* pages,
                                              const int* __restrict__ list, DevChunkResult* res) {
    __shared__ Run R[RUN_CAP];
    __shared__ int s_allp, s_nr, s_res;
    __shared__ uint32_t s_cov;
    const int pi = list[blockIdx.x];
    DevPage& pg = pages[pi];
    IdRunTab* T = pg.runtab;
    if (!T) return;
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    Sections s;
    if (res[pg.chunk].status != 0 || !page_sections(pg, ck, s) || s.val_n == 0 || s.val[0] > 32) {
        if (tid == 0) T->all_present = 0;
        return;
    }
    const uint32_t ne = uint32_t(pg.num_values);
    const int id_bw = int(s.val[0]);
    if (tid == 0) {
        s_allp = ck.max_def == 0 ? 1 : (s.def_rle ? all_present(s.def, s.def_n, bit_width(ck.max_def), ne, uint32_t(ck.max_def)) : 0);
    } else if (tid >= 64) {   // wave 1: the id runs, discovered wave-parallel
        __shared__ RunWalk s_st;
        int nr = 0;
        uint32_t cov = 0;
        const int rr = wave_walk_runs(s.val + 1, s.val_n - 1, id_bw, 0, ne, R, RUN_CAP, nr, cov, s_st, RunWalk{0, 0});
        if (tid == 64) { s_res = rr; s_nr = nr; s_cov = cov; }
    }
    __syncthreads();
    const int nr = s_nr;
    if (s_res == 2) {   // too many runs for the table: blocks walk themselves
        if (tid == 0) { T->valid = 0; T->all_present = 0; }
        return;
    }
    for (int i = tid; i < nr; i += 128) {
        T->fp(i) = R[i].first | (R[i].packed << 31);
        T->data(i) = R[i].data;
    }
    if (tid == 0) { T->nruns = uint32_t(nr); T->covered = s_cov; T->valid = 1u; T->all_present = s_allp ? 1u : 0u; }
}

// Dictionary-string pages k_count_flat takes: flat, levels all present (k_runs), a run table.
__device__ __forceinline__ bool count_dict_page(const DevPage& pg, const DevChunk& ck, const Sections& s) {
    const IdRunTab* T = pg.runtab;
    return T != nullptr && T->all_present == 1u && T->nruns <= uint32_t(RUN_CAP) && T->covered >= uint32_t(pg.num_values) && ck.dict_len &&
           s.val_n > 0 && flat_block_chars(pg) != nullptr;
}

// k_count_dict (round 5): the chars of one 4096-entry block of a flat dictionary BYTE_ARRAY page per
// workgroup -- the block's ids from the page's run table (k_runs), their dictionary lengths summed --
// into the page's per-block chars word bc[block]; k_count_flat scans those words into the blocks'
// chars bases and the page's chars. (Round 4 summed a page's blocks one after another in
// k_count_flat's one workgroup per page: SF1's pages of ~1M entries were 256 dependent rounds.)
__global__ __launch_bounds__(NT) void k_count_dict(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                   const int2* __restrict__ blocks, DevChunkResult* res) {
    __shared__ Run R[RUN_CAP];
    __shared__ uint32_t s_len[DSTR_CAP];   // lengths of small dictionaries
    __shared__ unsigned long long s_acc;
    const int2 pb = blocks[blockIdx.x];
    DevPage& pg = pages[pb.x];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    if (res[pg.chunk].status != 0 || ck.max_rep != 0 || ck.ptype != 6 || !is_dict_enc(pg.encoding)) return;
    Sections s;
    if (!page_sections(pg, ck, s) || !count_dict_page(pg, ck, s)) return;
    const uint32_t ne = uint32_t(pg.num_values);
    const uint32_t b0 = uint32_t(pb.y) * FBLK;
    if (pb.y > 0 && b0 >= ne) return;
    const uint32_t b1 = min(ne, b0 + FBLK);
    const IdRunTab* T = pg.runtab;
    const uint32_t nr = T->nruns, cov = T->covered;
    for (uint32_t i = tid; i < nr; i += NT) R[i] = id_run(T, i, nr, cov);
    const bool lstage = ck.dict_n > 0 && ck.dict_n <= int64_t(DSTR_CAP);
    if (lstage)
        for (uint32_t i = tid; i < uint32_t(ck.dict_n); i += NT) s_len[i] = gptr(ck.dict_len)[i];
    if (tid == 0) s_acc = 0;
    __syncthreads();
    const uint8_t* ids = s.val + 1;
    const uint64_t ids_n = s.val_n - 1;
    const int id_bw = int(s.val[0]);
    constexpr int EPB = int(FBLK) / NT;   // entries of the block per thread
    int bad = 0;
    uint64_t acc = 0;
    // ids of the thread's EPB entries first (their loads in flight together), then the lengths
    uint32_t idk[EPB];
    int r = -1;
    #pragma unroll
    for (int k = 0; k < EPB; k++) {
        const uint32_t e = b0 + uint32_t(k) * NT + uint32_t(tid);
        idk[k] = 0xffffffffu;
        if (e >= b1) continue;
        if (r < 0) r = run_find(R, int(nr), e);
        while (e >= R[r].first + R[r].count) r++;
        const Run& Rr = R[r];
        uint32_t id = Rr.data;
        if (Rr.packed) {
            const uint64_t bit = uint64_t(Rr.data) + uint64_t(e - Rr.first) * uint64_t(id_bw);
            id = (bit >> 3) + 12 <= ids_n ? bits_fast(ids + (bit >> 3), uint32_t(bit & 7), id_bw)
                                          : bits_le(ids, ids_n, bit, id_bw);
        }
        if (int64_t(id) >= ck.dict_n) { bad = 1; continue; }
        idk[k] = id;
    }
    #pragma unroll
    for (int k = 0; k < EPB; k++)
        if (idk[k] != 0xffffffffu) acc += lstage ? s_len[idk[k]] : gptr(ck.dict_len)[idk[k]];
    if (acc) atomicAdd(&s_acc, (unsigned long long)acc);
    bad = __syncthreads_or(bad);
    if (tid == 0) flat_block_chars(pg)[pb.y] = bad ? BC_BAD : uint64_t(s_acc);
}

// k_count for flat BYTE_ARRAY pages whose levels are all present: slots = rows = values =
// entries; dictionary strings scan k_count_dict's per-block chars (k_flat's per-block chars bases,
// the page's chars); PLAIN pages hand their value chain to the k_ba walk. Marks the page counted
// (pg.counted) so k_count skips it; pages it leaves alone (nulls, corrupt) go through k_count.
__global__ __launch_bounds__(NT) void k_count_flat(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                   const int* __restrict__ page_list, DevChunkResult* res,
                                                   BaJob* bajobs) {
    __shared__ int s_ok;
    __shared__ unsigned long long s_scan[NT / 64];
    const int pi = page_list[blockIdx.x];
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    if (res[pg.chunk].status != 0 || ck.max_rep != 0 || ck.ptype != 6) return;
    Sections s;
    if (!page_sections(pg, ck, s)) return;
    const bool dict = is_dict_enc(pg.encoding);
    const uint32_t ne = uint32_t(pg.num_values);
    uint64_t total = 0;
    if (dict) {
        if (!count_dict_page(pg, ck, s)) return;
        // k_count_dict's block sums -> exclusive bases in place (a page of 1M entries: 256 words)
        uint64_t* bc = flat_block_chars(pg);
        const uint32_t nb = (ne + FBLK - 1) / FBLK;
        int bad = 0;
        for (uint32_t b = 0; b < nb; b += NT) {
            const uint32_t i = b + uint32_t(tid);
            uint64_t v = i < nb ? bc[i] : 0ull;
            if (v == BC_BAD) { bad = 1; v = 0; }
            uint64_t tot;
            const uint64_t ex = block_excl_scan64<NT>(v, s_scan, tot);
            if (i < nb) bc[i] = total + ex;
            total += tot;
        }
        if (__syncthreads_or(bad)) return;   // k_count reports the bad id
    } else {
        if (pg.encoding != 0 || pg.ba_job < 0) return;
        if (tid == 0)
            s_ok = ck.max_def == 0 ? 1
                                   : (s.def_rle ? all_present(s.def, s.def_n, bit_width(ck.max_def), ne, uint32_t(ck.max_def)) : 0);
        __syncthreads();
        if (!s_ok) return;
        if (tid == 0) {   // the value chain is walked by the k_ba_* kernels
            BaJob& J = bajobs[pg.ba_job];
            J.p = s.val;
            J.n = uint32_t(min<uint64_t>(s.val_n, J.n_cap));
            J.count = int64_t(ne);
            J.state = ne > 0 ? BA_OK : BA_SKIP;
        }
    }
    if (tid == 0) {
        pg.n_slots = int64_t(ne);
        pg.n_values = int64_t(ne);
        pg.n_rows = int64_t(ne);
        pg.n_chars = int64_t(total);
        pg.counted = 1;
    }
}

// One 16-byte output chunk at arena address c (tile chars start at a0, total bytes): chunks inside
// one value are one 16-byte source read (aligned dwords + v_alignbyte); a chunk spanning values is
// blended from one aligned window per value piece. v: a value at or before the chunk's first byte.
__device__ __forceinline__ void copy_chunk16(const uint32_t* coff, const uint32_t* csrc, uint32_t nv, uint32_t total,
                                    const uint8_t* sbase, const uint8_t* send, uintptr_t a0, uintptr_t c, uint32_t v) {
    const int64_t r0 = int64_t(c) - int64_t(a0);
    uint32_t vb = coff[v];
    uint32_t vend = v + 1 < nv ? coff[v + 1] : total;
    while (r0 >= 0 && uint32_t(r0) >= vend && v + 1 < nv) {   // zero-length values share a start
        v++;
        vb = coff[v];
        vend = v + 1 < nv ? coff[v + 1] : total;
    }
    uint8_t* dst = reinterpret_cast<uint8_t*>(c);
    if (r0 >= 0 && uint32_t(r0) >= vb && uint64_t(r0) + 16 <= vend) {
        const uint8_t* sp = sbase + csrc[v] + (uint32_t(r0) - vb);
        if (sp + 20 <= send) {
            const uintptr_t sa = reinterpret_cast<uintptr_t>(sp);
            const uint32_t* q = reinterpret_cast<const uint32_t*>(sa & ~uintptr_t(3));
            const uint32_t sh = uint32_t(sa & 3u);
            uint32_t d[5];
            #pragma unroll
            for (int k = 0; k < 5; k++) d[k] = q[k];
            uint4 o;
            if (sh) {
                o.x = __builtin_amdgcn_alignbyte(d[1], d[0], sh);
                o.y = __builtin_amdgcn_alignbyte(d[2], d[1], sh);
                o.z = __builtin_amdgcn_alignbyte(d[3], d[2], sh);
                o.w = __builtin_amdgcn_alignbyte(d[4], d[3], sh);
            } else {
                o = make_uint4(d[0], d[1], d[2], d[3]);
            }
            *reinterpret_cast<uint4*>(dst) = o;
            return;
        }
    }
    // the chunk spans values: one aligned 16-byte window per value piece, blended under a byte mask
    // (dword loads that overlap the piece's source bytes only, so every load stays in the source)
    uint32_t word[4] = {0, 0, 0, 0};
    for (;;) {
        const int64_t lo = max(max(r0, int64_t(vb)), int64_t(0)), hi = min(min(r0 + 16, int64_t(vend)), int64_t(total));
        if (lo < hi) {
            const uintptr_t need0 = reinterpret_cast<uintptr_t>(sbase) + csrc[v] + uint32_t(lo - vb);
            const uintptr_t need1 = need0 + uintptr_t(hi - lo);            // source bytes [need0, need1)
            const uintptr_t ws = need0 - uintptr_t(lo - r0);               // source of chunk byte 0
            const uintptr_t wa = ws & ~uintptr_t(3);
            const uint32_t sh = uint32_t(ws & 3u);
            uint32_t d[5];
            #pragma unroll
            for (int k = 0; k < 5; k++) {
                const uintptr_t da = wa + 4u * k;
                d[k] = (da + 4 > need0 && da < need1) ? *reinterpret_cast<const uint32_t*>(da) : 0u;
            }
            const uint32_t bm = (0xffffu >> (16 - uint32_t(hi - r0))) & ~((1u << uint32_t(lo - r0)) - 1u);
            #pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t w = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
                const uint32_t m = (((bm >> (4 * k)) & 0xfu) * 0x00204081u & 0x01010101u) * 0xffu;
                word[k] = (word[k] & ~m) | (w & m);
            }
        }
        if (int64_t(vend) >= r0 + 16 || v + 1 >= nv) break;
        v++;
        vb = coff[v];
        vend = v + 1 < nv ? coff[v + 1] : total;
    }
    if (r0 >= 0 && r0 + 16 <= int64_t(total)) {
        *reinterpret_cast<uint4*>(dst) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
        #pragma unroll
        for (int k = 0; k < 16; k++) {
            const int64_t r = r0 + k;
            if (r >= 0 && r < int64_t(total)) dst[k] = uint8_t(word[k >> 2] >> (8 * (k & 3)));
        }
    }
}

// Chars copy with a chunk -> value table (no per-chunk binary search) and 16-byte source reads
// (aligned dwords + v_alignbyte) for chunks inside one value; other chunks blended per value piece.
// cv: LDS table of CV_CAP u16; send: end of the readable source buffer.
constexpr uint32_t CV_CAP = 2048;   // (round 5: 4096 -> 2048 brought k_flat_all under 32 KiB of LDS, five workgroups per CU)
__device__ __forceinline__ void copy_chars_fast(const uint32_t* coff, const uint32_t* csrc, uint32_t nv, uint32_t total,
                                       const uint8_t* sbase, const uint8_t* send, uint8_t* obase, uint16_t* cv) {
    if (total == 0 || nv == 0) return;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(obase);
    const uintptr_t c0 = a0 & ~uintptr_t(15);
    const uint32_t nch = uint32_t(((a0 + total + 15) & ~uintptr_t(15)) - c0) / 16u;
    // value v owns the chunks whose first byte lies inside it (chunk 0 may start before the tile: 0);
    // tiles of more than CV_CAP chunks in passes of CV_CAP (round 5: the per-chunk search before)
    for (uint32_t p0 = 0; p0 < nch; p0 += CV_CAP) {
        const uintptr_t lo = c0 + uintptr_t(p0) * 16u, hi = c0 + uintptr_t(min(nch, p0 + CV_CAP)) * 16u;
        if (p0 > 0) __syncthreads();   // the previous pass's table reads are done
        if (threadIdx.x == 0 && p0 == 0) cv[0] = 0;
        for (uint32_t v = threadIdx.x; v < nv; v += blockDim.x) {
            const uint32_t b = coff[v], e = v + 1 < nv ? coff[v + 1] : total;
            if (e <= b) continue;
            const uintptr_t ab = max(a0 + b, lo), ae = min(a0 + e, hi);
            for (uintptr_t c = (ab + 15) & ~uintptr_t(15); c < ae; c += 16) cv[(c - lo) >> 4] = uint16_t(v);
        }
        __syncthreads();
        for (uint32_t ci = threadIdx.x; ci < uint32_t((hi - lo) >> 4); ci += blockDim.x)
            copy_chunk16(coff, csrc, nv, total, sbase, send, a0, lo + uintptr_t(ci) * 16u, cv[ci]);
    }
}

// PLAIN BYTE_ARRAY chars (round 4): the tile's values are consecutive in the page body, each after its
// 4-byte length, so output byte r of value v comes from csrc[0] + r + 4 v: the chars are the source
// range with a 4-byte hole before every value. A thread copies one 64-byte output span with ONE round
// of source loads (the span's bytes plus 4 per value starting inside it: <= 21 aligned dwords), then
// assembles each output dword from the two shifted source dwords around a hole (v_perm). copy_chars_fast
// issued one dependent round of loads per 16-byte chunk, and its chunks spanning values (most of them
// for ~27-byte comments) blended one value piece at a time. Spans at the tile's ends, and spans where
// more than SP_K values start (or two holes fall in one dword), take copy_chunk16 per chunk.
constexpr uint32_t SP_K = 4;
__device__ __forceinline__ uint32_t sp_pick(const uint32_t* Z, int d, uint32_t h) {   // Z[d + h], h <= SP_K
    uint32_t r = Z[d];
    #pragma unroll
    for (uint32_t k = 1; k <= SP_K; k++) r = h >= k ? Z[d + int(k)] : r;
    return r;
}
__device__ __forceinline__ void copy_chars_plain(const uint32_t* coff, const uint32_t* csrc, uint32_t nv, uint32_t total,
                                        const uint8_t* sbase, const uint8_t* send, uint8_t* obase, uint16_t* cv) {
    if (total == 0 || nv == 0) return;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(obase);
    const uintptr_t s0 = a0 & ~uintptr_t(63);
    const uint32_t nsp = uint32_t(((a0 + total + 63) & ~uintptr_t(63)) - s0) / 64u;
    // more spans than the table holds (values averaging over 64 bytes): the chunk copy, in passes
    if (nsp > CV_CAP) { copy_chars_fast(coff, csrc, nv, total, sbase, send, obase, cv); return; }
    // value v owns the spans whose first byte lies inside it
    if (threadIdx.x == 0) cv[0] = 0;
    for (uint32_t v = threadIdx.x; v < nv; v += blockDim.x) {
        const uint32_t b = coff[v], e = v + 1 < nv ? coff[v + 1] : total;
        if (e <= b) continue;
        const uintptr_t ab = a0 + b, ae = a0 + e;
        for (uintptr_t c = (ab + 63) & ~uintptr_t(63); c < ae; c += 64) cv[(c - s0) >> 6] = uint16_t(v);
    }
    __syncthreads();
    const uint32_t base0 = csrc[0] - coff[0];   // (coff[0] == 0)
    for (uint32_t si = threadIdx.x; si < nsp; si += blockDim.x) {
        const uintptr_t c = s0 + uintptr_t(si) * 64u;
        const int64_t r0 = int64_t(c) - int64_t(a0);
        const uint32_t v = si == 0 ? 0u : uint32_t(cv[si]);
        bool wide = r0 >= 0 && r0 + 64 <= int64_t(total);
        uint64_t M = 0;   // bit b: a value starts at span byte b (0 < b < 64)
        uint32_t K = 0;
        if (wide) {
            uint32_t u = v + 1, prev = 0;
            #pragma unroll
            for (uint32_t k = 0; k <= SP_K; k++) {
                const uint32_t b = u < nv ? coff[u] - uint32_t(r0) : 64u;
                if (b < 64u) {
                    wide &= k < SP_K && b != prev;   // (a zero-length value: two holes at one byte)
                    M |= 1ull << b;
                    K++;
                    prev = b;
                    u++;
                }
            }
        }
        const uintptr_t src = reinterpret_cast<uintptr_t>(sbase) + base0 + uint32_t(r0) + 4u * v;
        if (wide) wide = src + 64u + 4u * K + 4u <= reinterpret_cast<uintptr_t>(send);
        if (wide) {   // a dword holding two holes (values of 1-3 bytes) is not one v_perm
            #pragma unroll
            for (int d = 0; d < 16; d++) wide &= __popcll((M >> (4 * d + 1)) & 7ull) <= 1;
        }
        if (!wide) {
            #pragma unroll
            for (int k = 0; k < 4; k++) copy_chunk16(coff, csrc, nv, total, sbase, send, a0, c + 16u * uint32_t(k), v);
            continue;
        }
        const uint32_t sh = uint32_t(src & 3u);
        const PF_GLOBAL uint32_t* q = (const PF_GLOBAL uint32_t*)(src & ~uintptr_t(3));
        const uint32_t nd = (sh + 64u + 4u * K + 3u) >> 2;   // <= 21 dwords hold the span's source bytes
        uint32_t W[21];   // (all issued together: dwords past nd re-read the last one, never past send)
        #pragma unroll
        for (int k = 0; k < 21; k++) W[k] = q[min(uint32_t(k), nd - 1u)];
        uint32_t Z[20];   // Z[j]: the 4 source bytes at src + 4 j
        #pragma unroll
        for (int k = 0; k < 20; k++) Z[k] = __builtin_amdgcn_alignbyte(W[k + 1], W[k], sh);
        uint32_t o[16];
        #pragma unroll
        for (int d = 0; d < 16; d++) {
            const uint32_t h0 = uint32_t(__popcll(M & ((2ull << (4 * d)) - 1ull)));   // holes before byte 4 d + 1
            const uint32_t m3 = uint32_t(M >> (4 * d + 1)) & 7u;                          // a hole at byte 4 d + 1..3
            const uint32_t A = sp_pick(Z, d, h0);
            const uint32_t B = sp_pick(Z, d, min(h0 + 1u, SP_K));
            const uint32_t t = uint32_t(__ffs(m3));                                         // 1..3, 0: none
            const uint32_t sel = 0x03020100u | (t ? (0x04040404u & (0xffffffffu << (8u * t))) : 0u);
            o[d] = __builtin_amdgcn_perm(B, A, sel);
        }
        PF_GLOBAL u32x4* d4 = (PF_GLOBAL u32x4*)c;
        #pragma unroll
        for (int k = 0; k < 4; k++) d4[k] = u32x4{o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]};
    }
}

#ifndef PF_SHORT_AVG
#define PF_SHORT_AVG 32   // r05: SF1 2.624-2.626 vs 2.630-2.643 ms at 16 (24: 2.610-2.631), configs 1 / 5 unchanged
#endif
constexpr uint32_t SHORT_AVG = PF_SHORT_AVG;   // tiles averaging at most this many chars per value: copy_chars_short
// Short values (dictionary strings such as flags and modes: 1-16 chars): one value per thread,
// lane-consecutive values, so a wave's byte stores cover one contiguous run of the chars arena.
// Each 8-byte piece of a value is read as the aligned dwords around it (+ v_alignbyte); a chunk
// copy (copy_chars_fast) would blend up to 16 values into every 16-byte chunk one at a time.
__device__ inline void copy_chars_short(const uint32_t* coff, const uint32_t* csrc, uint32_t nv, uint32_t total,
                                        const uint8_t* sbase, uint8_t* obase) {
    for (uint32_t v = threadIdx.x; v < nv; v += blockDim.x) {
        const uint32_t b = coff[v], e = v + 1 < nv ? coff[v + 1] : total;
        const uint8_t* sp = sbase + csrc[v];
        uint8_t* dp = obase + b;
        for (uint32_t o = 0; o < e - b; o += 8) {
            const uint32_t len = min(8u, e - b - o);
            const uintptr_t a = reinterpret_cast<uintptr_t>(sp + o);
            const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
            const uint32_t sh = uint32_t(a & 3u);
            const uint32_t d0 = q[0];
            const uint32_t d1 = sh + len > 4u ? q[1] : 0u;
            const uint32_t d2 = sh + len > 8u ? q[2] : 0u;
            const uint64_t x = uint64_t(__builtin_amdgcn_alignbyte(d1, d0, sh)) |
                               (uint64_t(__builtin_amdgcn_alignbyte(d2, d1, sh)) << 32);
            for (uint32_t i = 0; i < len; i++) dp[o + i] = uint8_t(x >> (8 * i));
        }
    }
}

struct FlatLds {
    uint32_t dpos[DSTR_CAP], dlen[DSTR_CAP];
    Run drun[RUN_CAP];
    Run vrun[RUN_CAP];
    uint32_t coff[FT];
    uint32_t csrc[FT];
    uint16_t cv[CV_CAP];
    uint32_t vbits[FT / 32 + 2];
    uint32_t scan_tmp[NT / 64];
    RunWalk dst, vst;
    int ndrun, nvrun, dres, vres, allp;
    uint32_t dcover, vcover, vlo;
};

// k_flat, all levels present, fixed-width values: value index = entry index, lane-consecutive
// entries so every load and store of a wave is one contiguous run of memory. Returns err.
#ifndef PF_DICT_LDS
#define PF_DICT_LDS 16384   // 16 KiB: 0.8 % faster SF1 step than 32 KiB (occupancy), 64 KiB 8 % slower (tools/gpu_ab_libs.sh)
#endif
constexpr uint32_t DICT_LDS = PF_DICT_LDS;   // bytes of a fixed-width dictionary staged in LDS (k_flat_fixed)
#ifndef PF_FIX_IDS
#define PF_FIX_IDS 0   // extra LDS bytes behind the dictionary for a block's ids (6144, which fits the date
                       // columns' 10 + 12 KB, costs a workgroup per CU: SF1 2.660-2.663 vs 2.632-2.655 ms)
#endif
struct FixedLds {
    uint64_t dict[(DICT_LDS + PF_FIX_IDS) / 8 + 2];   // the dictionary, then the block's id bytes when they fit
    Run vrun[RUN_CAP];
    uint32_t coff[FTX / 64];
    RunWalk vst;
    int nvrun, vres, allp;
    uint32_t vcover, vlo;
    uint32_t ib[2];                   // the block's id byte range [ib[0], ib[1])
};

template <class Lds>
__device__ __forceinline__ int flat_present_fixed(Lds& S, const DevChunk& ck, const DevPage& pg, const Sections& s, bool dict,
                                  bool boolean, int enc, int w, const uint8_t* ids, uint64_t ids_n, int id_bw,
                                  uint64_t slot_base, uint32_t e_begin, uint32_t e_end, bool direct = false) {
    const int tid = threadIdx.x;
    const uint8_t* vend = s.val + s.val_n;
    const bool dalign = dict && (reinterpret_cast<uintptr_t>(ck.dict_data) & uintptr_t(w - 1)) == 0;
    // dictionary gather from LDS when the whole dictionary fits (north_star: K3 LDS / global)
    const bool dlds = DICT_LDS > 0 && dict && dalign && (w == 4 || w == 8) && ck.dict_data != nullptr &&
                      ck.dict_n > 0 && uint64_t(ck.dict_n) * uint64_t(w) <= DICT_LDS;
    // The block's dictionary ids, when the run table covers the block and their bytes fit behind the
    // dictionary: staged in LDS with the dictionary's loads (round 5), so the tiles read ids from LDS
    // instead of issuing a round of id loads per tile batch. Page id byte k is staged byte k - idd.
    const uint32_t dbytes = dlds ? (uint32_t(ck.dict_n) * uint32_t(w) + 15u) & ~15u : 0u;
    uint8_t* const sid = reinterpret_cast<uint8_t*>(S.dict) + dbytes;
    int64_t idd = 0;
    bool ilds = false;
    if (dict && dalign && (w == 4 || w == 8) && id_bw > 0 && id_bw <= 32 && s.val_n > 0 && S.vres != 2 &&
        S.vlo <= e_begin && e_end <= S.vcover) {
        if (tid == 0) { S.ib[0] = 0xffffffffu; S.ib[1] = 0u; }
        __syncthreads();
        for (int r = tid; r < S.nvrun; r += NT) {
            const Run R = S.vrun[r];
            const uint32_t f = max(R.first, e_begin), l = min(R.first + R.count, e_end);
            if (!R.packed || f >= l) continue;
            atomicMin(&S.ib[0], uint32_t((uint64_t(R.data) + uint64_t(f - R.first) * uint64_t(id_bw)) >> 3));
            atomicMax(&S.ib[1], uint32_t((uint64_t(R.data) + uint64_t(l - R.first) * uint64_t(id_bw) + 7u) >> 3));
        }
        __syncthreads();
        const uint32_t lo = S.ib[0], hi = S.ib[1];
        if (lo < hi && hi <= ids_n) {
            const uintptr_t a0 = (reinterpret_cast<uintptr_t>(ids) + lo) & ~uintptr_t(15);
            const uintptr_t aend = reinterpret_cast<uintptr_t>(ids) + ids_n;     // readable source end
            const uint32_t nb = (uint32_t(reinterpret_cast<uintptr_t>(ids) + hi - a0) + 8u + 15u) & ~15u;
            if (dbytes + nb <= uint32_t(sizeof(S.dict))) {
                ilds = true;
                idd = int64_t(a0) - int64_t(reinterpret_cast<uintptr_t>(ids));
                for (uint32_t c = tid; c < nb / 16u; c += NT) {
                    const uintptr_t a = a0 + 16u * c;
                    u32x4 x;
                    if (a + 16u <= aend) {
                        x = *reinterpret_cast<const PF_GLOBAL u32x4*>(a);
                    } else {   // the section's last bytes: no read past it
                        uint32_t q[4] = {0, 0, 0, 0};
                        for (uint32_t b = 0; b < 16u && a + b < aend; b++)
                            q[b >> 2] |= uint32_t(*reinterpret_cast<const PF_GLOBAL uint8_t*>(a + b)) << (8 * (b & 3));
                        x = u32x4{q[0], q[1], q[2], q[3]};
                    }
                    reinterpret_cast<u32x4*>(sid)[c] = x;
                }
            }
        }
    }
    if (dlds) {   // eight loads a thread in flight per round (a 2,526-entry date dictionary: 2 rounds, not 10)
        const uint32_t dn = uint32_t(ck.dict_n);
        if (w == 8) {
            const PF_GLOBAL uint64_t* g = (const PF_GLOBAL uint64_t*)(ck.dict_data);
            for (uint32_t i0 = tid; i0 < dn; i0 += 8u * NT) {
                uint64_t v[8];
                #pragma unroll
                for (uint32_t k = 0; k < 8; k++) v[k] = i0 + k * NT < dn ? g[i0 + k * NT] : 0ull;
                #pragma unroll
                for (uint32_t k = 0; k < 8; k++) if (i0 + k * NT < dn) S.dict[i0 + k * NT] = v[k];
            }
        } else {
            const PF_GLOBAL uint32_t* g = (const PF_GLOBAL uint32_t*)(ck.dict_data);
            uint32_t* d32 = reinterpret_cast<uint32_t*>(S.dict);
            for (uint32_t i0 = tid; i0 < dn; i0 += 8u * NT) {
                uint32_t v[8];
                #pragma unroll
                for (uint32_t k = 0; k < 8; k++) v[k] = i0 + k * NT < dn ? g[i0 + k * NT] : 0u;
                #pragma unroll
                for (uint32_t k = 0; k < 8; k++) if (i0 + k * NT < dn) d32[i0 + k * NT] = v[k];
            }
        }
    }
    if (dlds || ilds) __syncthreads();
    for (uint32_t e0 = e_begin, want = 0; e0 < e_end; e0 += want) {
        want = min(uint32_t(FTX), e_end - e0);
        int bad = 0;
        if (dict) {
            if ((S.vlo > e0 || e0 + want > S.vcover) && S.vres == 2) {
                __syncthreads();
                if (tid < 64) {   // next window of runs (re-walk from the page start), wave 0
                    if (tid == 0) { S.vst = RunWalk{0, 0}; S.vlo = e0; }
                    const int rr = wave_walk_runs(ids, ids_n, id_bw, e0, e_end, S.vrun, RUN_CAP, S.nvrun, S.vcover, S.vst, RunWalk{0, 0});
                    if (tid == 0) S.vres = rr;
                }
                __syncthreads();
                // a tile whose ids need more runs than the table holds (runs shorter than FTX / RUN_CAP
                // values): this tile is the part the table covers, the next window starts after it
                if (S.vres == 2 && S.vcover > e0 && e0 + want > S.vcover) want = S.vcover - e0;
            }
            if (id_bw > 32 || s.val_n == 0 || ck.dict_data == nullptr || e0 + want > S.vcover || S.vlo > e0) bad = 1;
            if (!bad && uint32_t(tid) < (want + 63) / 64) S.coff[tid] = uint32_t(run_find(S.vrun, S.nvrun, e0 + tid * 64));
            __syncthreads();
        }
        const bool wide = w == 4 || w == 8;
        if (direct) {
            // the executor wrote this page's values into the column (k_snappy_head): validity only
        } else if (!bad && wide && ((dict && dalign) || enc == 0 || enc == 5)) {
            // batched: the loads of FB entries per thread are in flight together
#ifndef PF_FB_DIV
#define PF_FB_DIV 2
#endif
            constexpr uint32_t FB = FEPTX / PF_FB_DIV;   // entries per thread per load batch
            for (uint32_t kb = 0; kb < FEPTX; kb += FB) {
            uint64_t v[FB];
            uint32_t id[FB];
            #pragma unroll
            for (uint32_t k = 0; k < FB; k++) {
                const uint32_t e = e0 + (kb + k) * NT + uint32_t(tid);
                id[k] = 0;
                v[k] = 0;
                if (e >= e0 + want) continue;
                if (dict) {
                    int r = int(S.coff[(e - e0) >> 6]);
                    while (e >= S.vrun[r].first + S.vrun[r].count) r++;
                    const Run R = S.vrun[r];
                    id[k] = R.data;
                    if (R.packed) {
                        const uint64_t bit = uint64_t(R.data) + uint64_t(e - R.first) * uint64_t(id_bw);
                        if (ilds) {
                            const uint32_t rb = uint32_t(int64_t(bit) - 8 * idd);
                            const uint32_t* q = reinterpret_cast<const uint32_t*>(sid) + (rb >> 5);
                            const uint64_t x = (uint64_t(q[0]) | (uint64_t(q[1]) << 32)) >> (rb & 31u);
                            id[k] = uint32_t(x & (id_bw == 32 ? 0xffffffffull : ((1ull << id_bw) - 1ull)));
                        } else {
                            id[k] = (bit >> 3) + 12 <= ids_n ? bits_fast(ids + (bit >> 3), uint32_t(bit & 7), id_bw)
                                                             : bits_le(ids, ids_n, bit, id_bw);
                        }
                    }
                } else if (enc == 0) {
                    if ((uint64_t(e) + 1) * uint64_t(w) > s.val_n) { bad = 1; continue; }
                    const uint8_t* src = s.val + uint64_t(e) * uint64_t(w);
                    if (w == 8) v[k] = src + 12 <= vend ? gld_u64_12(src) : ld64_bytes(src);
                    else v[k] = src + 8 <= vend ? gld_u32_8(src) : ld32le(src, 0, 4);
                } else {
                    v[k] = reinterpret_cast<const uint64_t*>(pg.aux)[e];
                }
            }
            if (dict) {   // all FB gathers issued together (entries past the tile / bad ids load element 0)
                const int64_t dn = ck.dict_n;
                #pragma unroll
                for (uint32_t k = 0; k < FB; k++) {
                    const uint32_t e = e0 + (kb + k) * NT + uint32_t(tid);
                    if (e < e0 + want && int64_t(id[k]) >= dn) bad = 1;
                    id[k] = int64_t(id[k]) < dn ? id[k] : 0u;
                }
                if (dlds) {
                    #pragma unroll
                    for (uint32_t k = 0; k < FB; k++)
                        v[k] = w == 8 ? S.dict[id[k]] : reinterpret_cast<const uint32_t*>(S.dict)[id[k]];
                } else if (w == 8) {
                    const PF_GLOBAL uint64_t* g = (const PF_GLOBAL uint64_t*)ck.dict_data;
                    #pragma unroll
                    for (uint32_t k = 0; k < FB; k++) v[k] = g[id[k]];
                } else {
                    const PF_GLOBAL uint32_t* g = (const PF_GLOBAL uint32_t*)ck.dict_data;
                    #pragma unroll
                    for (uint32_t k = 0; k < FB; k++) v[k] = g[id[k]];
                }
            }
            #pragma unroll
            for (uint32_t k = 0; k < FB; k++) {
                const uint32_t e = e0 + (kb + k) * NT + uint32_t(tid);
                if (e >= e0 + want) continue;
                uint8_t* dst = ck.values + (slot_base + e) * uint64_t(w);
                if (w == 8) *reinterpret_cast<uint64_t*>(dst) = v[k];
                else *reinterpret_cast<uint32_t*>(dst) = uint32_t(v[k]);
            }
            }
        } else if (!bad) {
            #pragma unroll 2
            for (uint32_t k = 0; k < FEPTX; k++) {
                const uint32_t e = e0 + k * NT + uint32_t(tid);
                if (e >= e0 + want) break;
                uint8_t* dst = ck.values + (slot_base + e) * uint64_t(w);
                if (dict) {
                    int r = int(S.coff[(e - e0) >> 6]);
                    while (e >= S.vrun[r].first + S.vrun[r].count) r++;
                    const Run R = S.vrun[r];
                    uint32_t id = R.data;
                    if (R.packed) {
                        const uint64_t bit = uint64_t(R.data) + uint64_t(e - R.first) * uint64_t(id_bw);
                        id = (bit >> 3) + 12 <= ids_n ? bits_fast(ids + (bit >> 3), uint32_t(bit & 7), id_bw)
                                                      : bits_le(ids, ids_n, bit, id_bw);
                    }
                    if (int64_t(id) >= ck.dict_n) { bad = 1; continue; }
                    const uint8_t* src = ck.dict_data + uint64_t(id) * uint64_t(w);
                    if (w == 8 && dalign) *reinterpret_cast<uint64_t*>(dst) = *reinterpret_cast<const uint64_t*>(src);
                    else if (w == 4 && dalign) *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src);
                    else copy_value(dst, src, w);
                } else if (boolean) {
                    if ((e >> 3) >= s.val_n) { bad = 1; continue; }
                    dst[0] = uint8_t((s.val[e >> 3] >> (e & 7)) & 1u);
                } else if (enc == 0) {
                    if ((uint64_t(e) + 1) * uint64_t(w) > s.val_n) { bad = 1; continue; }
                    const uint8_t* src = s.val + uint64_t(e) * uint64_t(w);
                    if (w == 8 && src + 12 <= vend) *reinterpret_cast<uint64_t*>(dst) = gld_u64_12(src);
                    else if (w == 4 && src + 8 <= vend) *reinterpret_cast<uint32_t*>(dst) = gld_u32_8(src);
                    else copy_value(dst, src, w);
                } else {   // DELTA_BINARY_PACKED, decoded by k_delta into aux
                    const uint64_t* dv = reinterpret_cast<const uint64_t*>(pg.aux);
                    if (w == 8) *reinterpret_cast<uint64_t*>(dst) = dv[e];
                    else *reinterpret_cast<uint32_t*>(dst) = uint32_t(dv[e]);
                }
            }
        }
        if (ck.max_def > 0 && ck.validity) {   // all present: the tile's validity bits are ones
            const uint64_t b0 = slot_base + e0, b1 = b0 + want;
            uint32_t* vw = reinterpret_cast<uint32_t*>(ck.validity);
            for (uint64_t wd = (b0 >> 5) + tid; wd <= ((b1 - 1) >> 5); wd += NT) {
                const uint64_t lo = max(b0, wd << 5), hi = min(b1, (wd + 1) << 5);
                const uint32_t m = uint32_t((hi - lo >= 32 ? 0xffffffffull : ((1ull << (hi - lo)) - 1ull)) << (lo & 31));
                if (lo == (wd << 5) && hi == ((wd + 1) << 5)) vw[wd] = m;
                else atomicOr(vw + wd, m);
            }
        }
        if (__syncthreads_or(bad)) return 1;
    }
    return 0;
}

// k_flat for fixed-width pages whose levels are all present (the common case), with a small LDS
// footprint and its own register budget: one workgroup per (page, FBLK block). Marks the page
// done; k_flat decodes everything else (strings, pages with nulls).
// Returns whether the block took its (page, block) (block-uniform); false: k_flat's body decodes it.
__device__ __forceinline__ bool flat_fixed_block(FixedLds& S, const DevChunk* __restrict__ chunks, DevPage* pages, const int2 pbk,
                                 DevChunkResult* res) {
    if (pbk.x < 0) return true;   // padding of the XCD-grouped block list (runtime)
    const int pi = pbk.x;
    const uint32_t blk = uint32_t(pbk.y) & 0x0fffffffu;
    const uint32_t bsz = FBLK << (uint32_t(pbk.y) >> 28);   // entries per block (runtime: wide blocks for no-null pages)
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    // the page's, chunk's and result's words are read in one round (bitwise ors: a short-circuit
    // chain puts a wait between each load)
    const int* jfb = pg.jfb;
    const bool dval = pg.direct == DIRECT_VALUES;
    const int jf = jfb != nullptr ? *jfb : FB_WHOLE + 1;
    const int done = pg.done;
    if (done & DONE_DSTR) return true;   // k_flat_dstr decoded the page
    if ((res[pg.chunk].status != 0) | (ck.max_rep != 0) | (ck.ptype == 6) | ((done & DONE_NULL) != 0)) return false;
    if (dval & (jf <= FB_WHOLE)) {
        // the executor wrote the values (k_snappy_head checked the levels): this block's validity bits
        const uint32_t ne = uint32_t(pg.num_values), e_begin = blk * bsz;
        if (e_begin >= ne && blk > 0) return true;
        const uint32_t e_end = min(ne, e_begin + bsz);
        if (ck.max_def > 0 && ck.validity && e_end > e_begin) {
            const uint64_t b0 = uint64_t(pg.entry_start) + e_begin, b1 = uint64_t(pg.entry_start) + e_end;
            uint32_t* vw = reinterpret_cast<uint32_t*>(ck.validity);
            for (uint64_t wd = (b0 >> 5) + threadIdx.x; wd <= ((b1 - 1) >> 5); wd += NT) {
                const uint64_t lo = max(b0, wd << 5), hi = min(b1, (wd + 1) << 5);
                const uint32_t m = uint32_t((hi - lo >= 32 ? 0xffffffffull : ((1ull << (hi - lo)) - 1ull)) << (lo & 31));
                if (lo == (wd << 5) && hi == ((wd + 1) << 5)) vw[wd] = m;
                else atomicOr(vw + wd, m);
            }
        }
        if (threadIdx.x == 0) {
            if (ck.needs_count == 0)
                atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values), (unsigned long long)(e_end - e_begin));
            atomicOr(&pg.done, DONE_FIXED);
        }
        return true;
    }
    Sections s;
    if (!page_sections(pg, ck, s)) return false;
    const int enc = pg.encoding;
    const bool boolean = ck.ptype == 0, dict = is_dict_enc(enc);
    const int w = ck.width;
    bool take = ck.max_def == 0 || s.def_rle;
    if (enc == 0) {
    } else if (dict) take = take && !boolean;
    else if (enc == 5) take = take && (ck.ptype == 1 || ck.ptype == 2) && pg.aux != nullptr;
    else take = false;
    if (!take) return false;
    const uint32_t ne = uint32_t(pg.num_values);
    if (blk > 0 && blk * bsz >= ne) return true;
    const int id_bw = (dict && s.val_n > 0) ? int(s.val[0]) : 0;
    const uint8_t* ids = dict && s.val_n > 0 ? s.val + 1 : s.val;
    const uint64_t ids_n = dict && s.val_n > 0 ? s.val_n - 1 : 0;
    const IdRunTab* T = pg.runtab;
    uint32_t t0 = 0, t3 = 0;
    if (T != nullptr) { t0 = T->nruns; t3 = T->all_present; }
    const bool tab = (t3 == 1u) & (t0 <= uint32_t(RUN_CAP));   // k_runs: levels all present
    if (tid == 0)
        S.allp = tab ? 1 : (ck.max_def == 0 ? 1 : all_present(s.def, s.def_n, bit_width(ck.max_def), ne, uint32_t(ck.max_def)));
    __syncthreads();
    if (!S.allp) return false;
    const uint32_t e_begin = blk * bsz;
    const uint32_t e_end = min(ne, e_begin + bsz);
#ifdef PF_STAMPS
    const unsigned long long ft0 = __builtin_amdgcn_s_memtime();
#endif
    if (dict) {
        if (tab) {
            const uint32_t nr = T->nruns, cov = T->covered;
            for (uint32_t i = tid; i < nr; i += NT) S.vrun[i] = id_run(T, i, nr, cov);
            if (tid == 0) { S.nvrun = int(nr); S.vcover = cov; S.vlo = 0; S.vres = cov >= ne ? 0 : 1; }
        } else if (tid < 64) {   // wave 0 walks the id runs of this block
            if (tid == 0) { S.nvrun = 0; S.vcover = 0; S.vres = 0; S.vlo = e_begin; S.vst = RunWalk{0, 0}; }
            if (s.val_n > 0 && id_bw <= 32) {
                const int rr = wave_walk_runs(ids, ids_n, id_bw, e_begin, e_end, S.vrun, RUN_CAP, S.nvrun, S.vcover, S.vst, RunWalk{0, 0});
                if (tid == 0) S.vres = rr;
            }
        }
        __syncthreads();
    }
    // values already in place: the executor decoded the page without falling back (a redo / serial
    // fallback writes the body to scratch instead, and the page is decoded from there)
    const bool direct = dval & (jf <= FB_WHOLE);
    const int err = flat_present_fixed(S, ck, pg, s, dict, boolean, enc, w, ids, ids_n, id_bw,
                                       uint64_t(pg.entry_start), e_begin, e_end, direct);
#ifdef PF_STAMPS
    if (tid == 0) { const unsigned long long dt_ = __builtin_amdgcn_s_memtime() - ft0; PSTAMP(1, dt_); PSTAMP(0, 1); atomicMax(&pf_pstamps[9], dt_); }
#endif
    if (tid == 0) {
        if (err) set_status(res, pg.chunk, ST_CORRUPT, pi);
        else if (ck.needs_count == 0)
            atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values), (unsigned long long)(e_end - e_begin));
        atomicOr(&pg.done, DONE_FIXED);
    }
    return true;
}

// Fallback queue (device, zeroed with the batch metadata): word 0 counts the (page, block) pairs that
// start at word 4; k_flat_null and k_flat_fixed append the blocks they do not take, the last workgroups of k_flat_all decode them.
__device__ __forceinline__ void null_fallback(int* fbq, int2 pbk) {
    if (threadIdx.x == 0) reinterpret_cast<int2*>(fbq + 4)[atomicAdd(fbq, 1)] = pbk;
}

// k_flat_fixed (round 5): the blocks of flat fixed-width pages, in a list of their own. Its register
// budget is the fixed-width body's (73 VGPRs, 21 KiB LDS: six workgroups per CU, against four of
// k_flat_all's 127-VGPR union of both bodies); blocks it does not take (a page with nulls that
// k_flat_null did not take, levels that are not RLE, ...) go to the fallback queue (k_flat_all's last workgroups).
#ifndef PF_FIXED_OCC
#define PF_FIXED_OCC 6
#endif
__global__ __launch_bounds__(NT, PF_FIXED_OCC) void k_flat_fixed(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                              const int2* __restrict__ blocks, DevChunkResult* res, int* fbq) {
    __shared__ FixedLds S;
    const int2 pbk = blocks[blockIdx.x];
    if (!flat_fixed_block(S, chunks, pages, pbk, res)) null_fallback(fbq, pbk);
}

// One workgroup per (page, FBLK block of entries). Pages whose levels are all present (max_def
// == 0 or RLE runs of max_def) are decoded block by block in parallel: value index = entry
// index, each block walks the dictionary-id run headers up to its own range (windowed when a
// block needs more than RUN_CAP runs) and takes its chars base from k_count's block table or,
// for PLAIN BYTE_ARRAY, from the value positions. Pages with nulls are decoded by block 0 alone.
__device__ __forceinline__ void flat_block(FlatLds& S, const DevChunk* __restrict__ chunks, DevPage* pages, const int2 pbk,
                           DevChunkResult* res) {
    if (pbk.x < 0) return;   // padding of the XCD-grouped block list (runtime)
    const int pi = pbk.x;
    const uint32_t blk = uint32_t(pbk.y) & 0x0fffffffu;
    const uint32_t bsz = FBLK << (uint32_t(pbk.y) >> 28);   // (wide blocks: fixed-width pages only)
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    // DONE_FIXED: k_flat_fixed took the page, DONE_DSTR: k_flat_dstr. Never test DONE_FLAT here: this kernel's own
    // blocks of the same page set it when they finish, and a block that starts later must still run.
    if ((res[pg.chunk].status != 0) | (ck.max_rep != 0) | ((pg.done & (DONE_FIXED | DONE_NULL | DONE_DSTR)) != 0)) return;
    Sections s;
    if (!page_sections(pg, ck, s)) return;                 // k_decode reports it
    const int enc = pg.encoding;
    const bool binary = ck.ptype == 6, boolean = ck.ptype == 0, dict = is_dict_enc(enc);
    const int w = ck.width;
    bool take = ck.max_def == 0 || s.def_rle;
    if (enc == 0) {
    } else if (dict) take = take && !boolean;
    else if (enc == 5) take = take && (ck.ptype == 1 || ck.ptype == 2) && pg.aux != nullptr;
    else take = false;
    if (!take) return;

    const int bwd = bit_width(ck.max_def);
    const uint32_t ne = uint32_t(pg.num_values);
    const int id_bw = (dict && s.val_n > 0) ? int(s.val[0]) : 0;
    const uint8_t* ids = dict && s.val_n > 0 ? s.val + 1 : s.val;
    const uint64_t ids_n = dict && s.val_n > 0 ? s.val_n - 1 : 0;
    const bool counted = ck.needs_count != 0;
    const uint64_t slot_base = uint64_t(pg.entry_start);   // flat: slot == entry
    if (blk > 0 && blk * bsz >= ne) return;
    const IdRunTab* T = pg.runtab;
    uint32_t t0 = 0, t3 = 0;
    if (T != nullptr) { t0 = T->nruns; t3 = T->all_present; }
    const bool tab = (t3 == 1u) & (t0 <= uint32_t(RUN_CAP));   // k_runs: levels all present
    if (tid == 0) S.allp = tab ? 1 : (ck.max_def == 0 ? 1 : all_present(s.def, s.def_n, bwd, ne, uint32_t(ck.max_def)));
    __syncthreads();
    const bool split = S.allp;
    if (!split && blk > 0) return;                          // block 0 decodes the whole page
    const uint32_t e_begin = split ? blk * bsz : 0u;
    const uint32_t e_end = split ? min(ne, e_begin + bsz) : ne;
#ifdef PF_STAMPS
    const unsigned long long ft0 = __builtin_amdgcn_s_memtime();
    if (tid == 0) { PSTAMP(0, 1); if (dict) PSTAMP(6, 1); if (binary) PSTAMP(7, 1); }
#endif
    if (tid < 64) {   // wave 0: definition-level runs (pages with nulls)
        if (tid == 0) { S.ndrun = 0; S.dcover = ne; S.dres = 0; S.dst = RunWalk{0, 0}; }
        if (!split && ck.max_def > 0) {
            const int rr = wave_walk_runs(s.def, s.def_n, bwd, 0, ne, S.drun, RUN_CAP, S.ndrun, S.dcover, S.dst, RunWalk{0, 0});
            if (tid == 0) S.dres = rr;
        }
    } else if (tid < 128 && !(split && tab)) {   // wave 1: dictionary-id runs
        if (tid == 64) { S.nvrun = 0; S.vcover = 0; S.vres = 0; S.vlo = e_begin; S.vst = RunWalk{0, 0}; }
        if (dict && s.val_n > 0 && id_bw <= 32) {
            const int rr = wave_walk_runs(ids, ids_n, id_bw, e_begin, split ? e_end : ne, S.vrun, RUN_CAP, S.nvrun,
                                          S.vcover, S.vst, RunWalk{0, 0});
            if (tid == 64) S.vres = rr;
        }
    }
    if (split && tab) {   // the page's run table (k_runs), loaded by all threads
        const uint32_t nr = T->nruns, cov = T->covered;
        for (uint32_t i = tid; i < nr; i += NT) S.vrun[i] = id_run(T, i, nr, cov);
        if (tid == 0) { S.nvrun = int(nr); S.vcover = cov; S.vlo = 0; S.vres = cov >= ne ? 0 : 1; }
    }
    // small string dictionaries: {pos, len} from LDS (visible after the tile loop's first barrier)
    const bool dstage = binary && dict && ck.dict_pos != nullptr && ck.dict_n > 0 && ck.dict_n <= int64_t(DSTR_CAP);
    if (dstage) {
        const PF_GLOBAL uint32_t* gp = gptr(ck.dict_pos);
        const PF_GLOBAL uint32_t* gl = gptr(ck.dict_len);
        for (uint32_t i = uint32_t(tid); i < uint32_t(ck.dict_n); i += NT) { S.dpos[i] = gp[i]; S.dlen[i] = gl[i]; }
    }
    __syncthreads();
#ifdef PF_STAMPS
    unsigned long long ft1 = __builtin_amdgcn_s_memtime();
    if (tid == 0) PSTAMP(2, ft1 - ft0);
#endif
    if (!split && (S.dres == 2 || S.vres == 2)) return;    // too many runs: k_decode takes the page
    bool allp = true, lvl_bad = S.dres != 0;
    if (!split) {
        for (int r = 0; r < S.ndrun; r++) {
            const Run& R = S.drun[r];
            if (R.packed || R.data != uint32_t(ck.max_def)) allp = false;
            if (!R.packed && R.data > uint32_t(ck.max_def)) lvl_bad = true;
        }
    }
    if (lvl_bad) {
        if (tid == 0) { set_status(res, pg.chunk, ST_CORRUPT, pi); atomicOr(&pg.done, DONE_FLAT); }
        return;
    }
    uint64_t char_base = 0;
    if (binary && counted) {
        char_base = uint64_t(pg.char_start);
        if (e_begin > 0) {
            if (dict) char_base += flat_block_chars(pg)[blk];
            else char_base += uint64_t(pg.aux[e_begin]) - 4ull * (uint64_t(e_begin) + 1);
        }
    }
    uint64_t vidx = e_begin;                                // page-relative index of the next present value
    int err = 0;
#ifdef PF_STAMPS   // tile sub-phases (tools/probe_flat_all.py): 11 levels, 12 values, 13 scan, 14 offsets, 15 chars
    unsigned long long fs_ = __builtin_amdgcn_s_memtime();
#define FSTAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (tid == 0) PSTAMP(i, t_ - fs_); fs_ = t_; } while (0)
#else
#define FSTAMP(i) ((void)0)
#endif


    for (uint32_t e0 = e_begin, want = 0; e0 < e_end; e0 += want) {
        want = min(uint32_t(FT), e_end - e0);
        if (split && dict && S.vres == 2 && (uint64_t(S.vlo) > uint64_t(e0) || e0 + want > S.vcover)) {
            // all levels present: value index = entry index. Next window of id runs before the levels,
            // and a tile needing more runs than the table holds shrinks to what it covers
            __syncthreads();
            if (tid < 64) {
                if (tid == 0) { S.vst = RunWalk{0, 0}; S.vlo = e0; }
                const int rr = wave_walk_runs(ids, ids_n, id_bw, e0, e_end, S.vrun, RUN_CAP, S.nvrun, S.vcover, S.vst,
                                              RunWalk{0, 0});
                if (tid == 0) S.vres = rr;
            }
            __syncthreads();
            if (S.vres == 2 && S.vcover > e0 && e0 + want > S.vcover) want = S.vcover - e0;
        }
        const uint32_t eb = uint32_t(tid) * FEPT;
        for (uint32_t i = tid; i < FT / 32 + 2; i += NT) S.vbits[i] = 0;
        // ---- definition levels -> present bits of this thread's entries
        uint32_t fv = 0;
        int bad = 0;
        if (eb < want) {
            const uint32_t m = min(uint32_t(FEPT), want - eb);
            if (allp) {
                fv = m >= 32 ? 0xffffffffu : (1u << m) - 1u;
            } else {
                const uint32_t e = e0 + eb;
                int r = run_find(S.drun, S.ndrun, e);
                for (uint32_t k = 0; k < m; k++) {
                    while (e + k >= S.drun[r].first + S.drun[r].count) r++;
                    const uint32_t d = run_value(S.drun[r], s.def, s.def_n, e + k, bwd);
                    bad |= d > uint32_t(ck.max_def);
                    fv |= uint32_t(d == uint32_t(ck.max_def)) << k;
                }
            }
        }
        uint32_t tv;
        uint32_t vo;
        if (allp) { vo = min(eb, want); tv = want; }
        else vo = block_excl_scan<NT>(__popc(fv), S.scan_tmp, tv);
        // ---- dictionary: this tile's values [vidx, vidx + tv) must be in the run table
        if (tv > 0 && dict) {
            if (split && (uint64_t(S.vlo) > vidx || vidx + tv > uint64_t(S.vcover)) && S.vres == 2) {
                __syncthreads();
                if (tid < 64) {   // next window of runs (re-walk from the page start), wave 0
                    if (tid == 0) { S.vst = RunWalk{0, 0}; S.vlo = uint32_t(vidx); }
                    const int rr = wave_walk_runs(ids, ids_n, id_bw, uint32_t(vidx), e_end, S.vrun, RUN_CAP, S.nvrun,
                                                  S.vcover, S.vst, RunWalk{0, 0});
                    if (tid == 0) S.vres = rr;
                }
                __syncthreads();
            }
            if (id_bw > 32 || s.val_n == 0 || (binary ? ck.dict_pos == nullptr : ck.dict_data == nullptr) ||
                vidx + tv > uint64_t(S.vcover) || uint64_t(S.vlo) > vidx)
                bad = 1;
        }
        if (__syncthreads_or(bad)) { err = 1; break; }
        FSTAMP(11);
        // ---- values
        uint32_t lsum = 0;
        uint32_t my_src[FEPT], my_len[FEPT];   // indexed by entry k (static after unrolling)
        {
            uint32_t j = 0;
            int vr = -1;
            #pragma unroll
            for (uint32_t k = 0; k < FEPT; k++) {
                my_src[k] = 0;
                my_len[k] = 0;
                if (eb + k >= want) continue;
                const uint64_t slot = slot_base + e0 + eb + k;
                const bool present = (fv >> k) & 1u;
                if (!binary) {
                    uint8_t* dst = ck.values + slot * uint64_t(w);
                    if (!present) { zero_value(dst, w); continue; }
                    const uint64_t gv = vidx + vo + j++;
                    if (dict) {
                        if (vr < 0) vr = run_find(S.vrun, S.nvrun, uint32_t(gv));
                        while (gv >= uint64_t(S.vrun[vr].first) + S.vrun[vr].count) vr++;
                        const uint32_t id = run_value(S.vrun[vr], ids, ids_n, uint32_t(gv), id_bw);
                        if (int64_t(id) >= ck.dict_n) { bad = 1; continue; }
                        copy_value(dst, ck.dict_data + uint64_t(id) * uint64_t(w), w);
                    } else if (boolean) {
                        if ((gv >> 3) >= s.val_n) { bad = 1; continue; }
                        dst[0] = uint8_t((s.val[gv >> 3] >> (gv & 7)) & 1u);
                    } else if (enc == 0) {
                        if ((gv + 1) * uint64_t(w) > s.val_n) { bad = 1; continue; }
                        copy_value(dst, s.val + gv * uint64_t(w), w);
                    } else {   // DELTA_BINARY_PACKED, decoded by k_delta into aux
                        const uint64_t* dv = reinterpret_cast<const uint64_t*>(pg.aux);
                        if (w == 8) *reinterpret_cast<uint64_t*>(dst) = dv[gv];
                        else *reinterpret_cast<uint32_t*>(dst) = uint32_t(dv[gv]);
                    }
                } else if (present) {
                    // strings: ids / positions of all FEPT entries first (their loads in flight
                    // together), the dictionary {pos, len} gathers in a second pass
                    const uint64_t gv = vidx + vo + j;
                    if (dict) {
                        if (vr < 0) vr = run_find(S.vrun, S.nvrun, uint32_t(gv));
                        while (gv >= uint64_t(S.vrun[vr].first) + S.vrun[vr].count) vr++;
                        const Run R = S.vrun[vr];
                        uint32_t id = R.data;
                        if (R.packed) {
                            const uint64_t bit = uint64_t(R.data) + uint64_t(uint32_t(gv) - R.first) * uint64_t(id_bw);
                            id = (bit >> 3) + 12 <= ids_n ? bits_fast(ids + (bit >> 3), uint32_t(bit & 7), id_bw)
                                                          : bits_le(ids, ids_n, bit, id_bw);
                        }
                        my_src[k] = id;
                        my_len[k] = 1;   // present (the length comes from the dictionary)
                    } else {   // PLAIN: value positions from the k_ba walk; a value's length is the
                               // distance to the next position (the walk checked the chain), the
                               // page's last value reads its length prefix
                        const PF_GLOBAL uint32_t* ax = gptr(pg.aux);
                        const uint32_t p = ax[gv];
                        uint32_t ln;
                        if (split && gv + 1 < uint64_t(ne)) {
                            const uint32_t nx = ax[gv + 1];
                            ln = nx >= p + 4 ? nx - p - 4 : 0xffffffffu;
                        } else {
                            ln = (p >= 4 && p <= s.val_n) ? ld32le(s.val, p - 4, s.val_n) : 0xffffffffu;
                        }
                        if (p >= 4 && p <= s.val_n && ln <= s.val_n - p) { my_src[k] = p; my_len[k] = ln; lsum += ln; }
                        else bad = 1;
                    }
                    j++;
                }
            }
            if (binary && dict) {
                const PF_GLOBAL uint32_t* gp = gptr(ck.dict_pos);
                const PF_GLOBAL uint32_t* gl = gptr(ck.dict_len);
                #pragma unroll
                for (uint32_t k = 0; k < FEPT; k++) {
                    if (!my_len[k]) continue;
                    const uint32_t id = my_src[k];
                    uint32_t src = 0, l = 0;
                    if (int64_t(id) >= ck.dict_n) bad = 1;
                    else if (dstage) { src = S.dpos[id]; l = S.dlen[id]; }
                    else { src = gp[id]; l = gl[id]; }
                    my_src[k] = src;
                    my_len[k] = l;
                    lsum += l;
                }
            }
        }
        FSTAMP(12);
        uint32_t tchars = 0;
        const uint32_t lo = binary ? block_excl_scan<NT>(lsum, S.scan_tmp, tchars) : 0;
        if (binary && char_base + tchars > uint64_t(pg.char_start + pg.n_chars)) bad = 1;   // k_count disagrees
        if (__syncthreads_or(bad)) { err = 1; break; }
        FSTAMP(13);
        if (binary) {
            uint32_t c = lo, j = 0;
            #pragma unroll
            for (uint32_t k = 0; k < FEPT; k++) {
                if (eb + k >= want) continue;
                if ((fv >> k) & 1u) {
                    S.coff[vo + j] = c;
                    S.csrc[vo + j] = my_src[k];
                    c += my_len[k];
                    j++;
                }
                ck.offsets[slot_base + e0 + eb + k + 1] = int32_t(char_base + c);
            }
        }
        // validity bits of this thread's entries
        if (ck.max_def > 0 && fv) {
            const uint64_t abase = (slot_base + e0) & ~uint64_t(31);
            const uint64_t rb = slot_base + e0 + eb - abase;
            const uint32_t sh = uint32_t(rb & 31);
            atomicOr(&S.vbits[rb >> 5], fv << sh);
            if (sh + FEPT > 32 && sh) atomicOr(&S.vbits[(rb >> 5) + 1], fv >> (32 - sh));
        }
        __syncthreads();
#ifdef PF_STAMPS
        { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (tid == 0) { PSTAMP(4, t_ - ft1); PSTAMP(3, 1); PSTAMP(14, t_ - fs_); } ft1 = t_; fs_ = t_; }
#endif
        if (binary) {
            const uint8_t* sb = dict ? ck.dict_data : s.val;
            const uint8_t* se = dict ? pages[ck.dict_page].body + pages[ck.dict_page].body_len : s.val + s.val_n;
            if (tchars <= SHORT_AVG * tv) copy_chars_short(S.coff, S.csrc, tv, tchars, sb, ck.chars + char_base);
            else if (!dict) copy_chars_plain(S.coff, S.csrc, tv, tchars, sb, se, ck.chars + char_base, S.cv);
            else copy_chars_fast(S.coff, S.csrc, tv, tchars, sb, se, ck.chars + char_base, S.cv);
        }
        FSTAMP(15);
        if (ck.max_def > 0 && ck.validity) flush_bits(S.vbits, slot_base + e0, want, ck.validity);
        vidx += tv;
        char_base += tchars;
        __syncthreads();
#ifdef PF_STAMPS
        { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (tid == 0) PSTAMP(5, t_ - ft1); ft1 = t_; }
#endif
    }
#ifdef PF_STAMPS
    if (tid == 0) {
        const unsigned long long dt_ = __builtin_amdgcn_s_memtime() - ft0;
        PSTAMP(1, dt_);
        atomicMax(&pf_pstamps[binary ? 8 : 9], dt_);
        if (!split) PSTAMP(10, 1);
    }
#endif
    if (tid == 0) {
        if (err) set_status(res, pg.chunk, ST_CORRUPT, pi);
        else if (!counted) atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values),
                                     (unsigned long long)(vidx - e_begin));
        atomicOr(&pg.done, DONE_FLAT);
    }
}

// ---- k_flat_dstr: flat dictionary BYTE_ARRAY pages with a small dictionary of short values ---------
// (flags, modes, instructions: a few values of 1-25 chars.) One pass over the FBLK entries of a (page,
// block) pair of k_count_dict's list, 16 consecutive entries per thread, with everything a value needs
// in LDS: the page's run table, the dictionary's {pos, len} and chars, and the block's id bytes. A
// thread's chars are contiguous, so they are assembled in an LDS window and leave as aligned 16-byte
// stores. The page is taken when the test below holds; it depends on the page, its dictionary and the
// count stage only, so all blocks of a page decide alike, and k_flat_all's blocks of a taken page
// return at DONE_DSTR. A page it declines is decoded by k_flat_all as before.
#ifndef PF_DSTR_LMAX
#define PF_DSTR_LMAX 32     // longest dictionary value taken (= SHORT_AVG: the pages copy_chars_short served)
#endif
#ifndef PF_DSTR_DICT
#define PF_DSTR_DICT 4096   // bytes of the dictionary page body staged in LDS
#endif
#ifndef PF_DSTR_WIN
#define PF_DSTR_WIN 16384   // bytes of the chars window (first the block's id bytes)
#endif
#ifndef PF_DSTR_OCC
#define PF_DSTR_OCC 6
#endif
constexpr uint32_t DSTR_LMAX = PF_DSTR_LMAX, DSTR_DICT = PF_DSTR_DICT, DSTR_WIN = PF_DSTR_WIN;
static_assert(DSTR_WIN % 16 == 0 && DSTR_DICT % 16 == 0 && DSTR_DICT + 16 < 65536 && DSTR_LMAX < 65536,
              "{pos, len} of a staged dictionary value share one word");
static_assert(RUN_CAP <= NT && int(DSTR_CAP) <= NT && FBLK == 16u * NT, "one run, one dictionary value, 16 entries per thread");
struct DstrLds {
    uint32_t rt[2 * RUN_CAP];             // k_runs' rows
    uint32_t dpl[DSTR_CAP];               // staged position | length << 16
    u32x4 dict[DSTR_DICT / 16 + 2];       // the dictionary page body from the 16-byte boundary at or before it
    u32x4 win[DSTR_WIN / 16 + 2];
    uint32_t scan_tmp[NT / 64];
    uint32_t wlo[NT / 64], whi[NT / 64];  // id byte range of the block's packed runs, per wave
};
#ifdef PF_DIAG   // diagnostics build: blocks k_flat_dstr decoded, pages it declined (tests)
__device__ unsigned long long pf_dstr_counts[2];
extern "C" int pf_debug_dstr_counts(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pf_dstr_counts), sizeof(unsigned long long) * 2) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pf_dstr_counts), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#define DSTR_COUNT(i) (threadIdx.x == 0 ? (void)atomicAdd(&pf_dstr_counts[i], 1ull) : (void)0)
#else
#define DSTR_COUNT(i) ((void)0)
#endif

// The 16 bytes at the aligned address a; bytes outside [beg, end) are not read and give zero.
__device__ __forceinline__ u32x4 ld16_within(uintptr_t a, uintptr_t beg, uintptr_t end) {
    if (a >= beg && a + 16u <= end) return *reinterpret_cast<const PF_GLOBAL u32x4*>(a);
    uint32_t q[4] = {0, 0, 0, 0};
    #pragma unroll
    for (uint32_t b = 0; b < 16u; b++)
        if (a + b >= beg && a + b < end) q[b >> 2] |= uint32_t(*reinterpret_cast<const PF_GLOBAL uint8_t*>(a + b)) << (8 * (b & 3));
    return u32x4{q[0], q[1], q[2], q[3]};
}

// A thread's 16 consecutive int32 at p: LEAD single words up to the 16-byte boundary, then 16-byte stores.
template <int LEAD>
__device__ __forceinline__ void store_offs16(int32_t* p, const uint32_t (&o)[16]) {
    #pragma unroll
    for (int k = 0; k < LEAD; k++) p[k] = int32_t(o[k]);
    #pragma unroll
    for (int k = LEAD; k + 4 <= 16; k += 4) *reinterpret_cast<u32x4*>(p + k) = u32x4{o[k], o[k + 1], o[k + 2], o[k + 3]};
    #pragma unroll
    for (int k = LEAD + (16 - LEAD) / 4 * 4; k < 16; k++) p[k] = int32_t(o[k]);
}

__global__ __launch_bounds__(NT, PF_DSTR_OCC) void k_flat_dstr(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                            const int2* __restrict__ blocks, DevChunkResult* res) {
    __shared__ DstrLds S;
    const int2 pb = blocks[blockIdx.x];
    const int pi = pb.x;
    const uint32_t blk = uint32_t(pb.y);
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    const uint32_t ne = uint32_t(pg.num_values);
    const uint32_t b0 = blk * FBLK;
    if (blk > 0 && b0 >= ne) return;
    // ---- does the page qualify (block-uniform, and the same for every block of the page)
    bool ok = (res[pg.chunk].status == 0) & (ck.max_rep == 0) & (ck.ptype == 6) & is_dict_enc(pg.encoding) & (pg.counted == 1) &
              (pg.num_values > 0) & (ck.dict_n > 0) & (ck.dict_n <= int64_t(DSTR_CAP)) & (ck.dict_page >= 0);
    ok = ok && ck.dict_pos != nullptr && ck.dict_len != nullptr && ck.dict_data != nullptr && ck.chars != nullptr &&
         ck.offsets != nullptr;
    Sections s;
    ok = ok && page_sections(pg, ck, s) && count_dict_page(pg, ck, s) && s.val[0] <= 32;
    const uintptr_t dbeg = reinterpret_cast<uintptr_t>(ck.dict_data);
    uintptr_t dend = dbeg;
    if (ok) {
        const DevPage& dp = pages[ck.dict_page];
        dend = reinterpret_cast<uintptr_t>(dp.body) + dp.body_len;
        ok = dend > dbeg && dend - dbeg <= uintptr_t(DSTR_DICT);
    }
    if (!ok) {
        if (blk == 0) DSTR_COUNT(1);
        return;
    }
    const uint32_t b1 = min(ne, b0 + FBLK);
    const IdRunTab* T = pg.runtab;
    const uint32_t nr = T->nruns, cov = T->covered;
    const uint32_t dn = uint32_t(ck.dict_n), dbytes = uint32_t(dend - dbeg);
    const int id_bw = int(s.val[0]);
    const uint8_t* ids = s.val + 1;
    const uint64_t ids_n = s.val_n - 1;
    const uint64_t bc_blk = blk > 0 ? flat_block_chars(pg)[blk] : 0ull;
    // ---- stage: run table, dictionary {pos, len}, dictionary body (one round of loads)
    int bad = 0;
    uint32_t mylo = 0xffffffffu, myhi = 0u;   // id bytes [mylo, myhi) of this thread's run inside the block
    if (uint32_t(tid) < nr) {
        const uint32_t f = T->fp(tid), d = T->data(tid);
        const uint32_t nf = uint32_t(tid) + 1 < nr ? T->next_first(tid) : cov;
        S.rt[2 * tid] = f;
        S.rt[2 * tid + 1] = d;
        const uint32_t first = f & 0x7fffffffu;
        const uint32_t a = max(first, b0), z = min(nf, b1);
        if ((f >> 31) && a < z) {
            mylo = uint32_t((uint64_t(d) + uint64_t(a - first) * uint64_t(id_bw)) >> 3);
            myhi = uint32_t((uint64_t(d) + uint64_t(z - first) * uint64_t(id_bw) + 7u) >> 3);
        }
    }
    const uint32_t doff = uint32_t(dbeg & 15u);
    if (uint32_t(tid) < dn) {
        const uint32_t pos = gptr(ck.dict_pos)[tid], len = gptr(ck.dict_len)[tid];
        bad = (len > DSTR_LMAX) | (pos > dbytes) | (len > dbytes - min(pos, dbytes));
        S.dpl[tid] = (doff + pos) | (len << 16);
    }
    for (uint32_t c = tid; c < (doff + dbytes + 15u) / 16u; c += NT) S.dict[c] = ld16_within(dbeg - doff + 16u * c, dbeg, dend);
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mylo = min(mylo, uint32_t(__shfl_xor(mylo, d, 64)));
        myhi = max(myhi, uint32_t(__shfl_xor(myhi, d, 64)));
    }
    if ((tid & 63) == 0) { S.wlo[tid >> 6] = mylo; S.whi[tid >> 6] = myhi; }
    if (__syncthreads_or(bad)) {   // a long value, or one that leaves the dictionary page: k_flat_all's
        if (blk == 0) DSTR_COUNT(1);
        return;
    }
    // ---- the block's id bytes into the window (a block of wide ids that does not fit reads them bytewise)
    uint32_t lo = 0xffffffffu, hi = 0u;
    #pragma unroll
    for (int w = 0; w < NT / 64; w++) { lo = min(lo, S.wlo[w]); hi = max(hi, S.whi[w]); }
    const uintptr_t ibeg = reinterpret_cast<uintptr_t>(ids), iend = ibeg + ids_n;
    const uintptr_t ia0 = (ibeg + (lo < hi ? lo : 0u)) & ~uintptr_t(15);
    const uint32_t inb = lo < hi ? (uint32_t(ibeg + hi - ia0) + 8u + 15u) & ~15u : 0u;
    const bool ilds = inb > 0 && inb <= uint32_t(sizeof(S.win));
    if (ilds) {
        for (uint32_t c = tid; c < inb / 16u; c += NT) S.win[c] = ld16_within(ia0 + 16u * c, ibeg, iend);
        __syncthreads();
    }
    const int64_t bias = ilds ? 8 * (int64_t(ibeg) - int64_t(ia0)) : 0;
    const uint32_t* const wl = reinterpret_cast<const uint32_t*>(S.win);
    const auto W = [&](uint32_t w) -> uint32_t {
        if (ilds) return wl[w];
        return ld32le(ids, uint64_t(w) * 4u, ids_n);
    };
    // ---- ids -> {pos, len}, chars before each value
    const uint32_t e0 = b0 + 16u * uint32_t(tid);
    const uint32_t n = e0 < b1 ? min(16u, b1 - e0) : 0u;
    uint32_t pl[16];
    uint32_t lsum = 0;
    {
        uint32_t id[16];
        dstr_ids16(S.rt, nr, cov, e0, n, id_bw, bias, W, id);
        #pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            pl[k] = 0;
            if (k >= n) continue;
            if (id[k] >= dn) { bad = 1; continue; }
            pl[k] = S.dpl[id[k]];
            lsum += pl[k] >> 16;
        }
    }
    uint32_t tot;
    const uint32_t lo_c = block_excl_scan<NT>(lsum, S.scan_tmp, tot);
    const uint64_t char_base = uint64_t(pg.char_start) + bc_blk;
    if (char_base + tot > uint64_t(pg.char_start + pg.n_chars)) bad = 1;   // the count stage disagrees
    if (__syncthreads_or(bad)) {   // (also: every thread has read its ids before the window is reused)
        if (tid == 0) {
            set_status(res, pg.chunk, ST_CORRUPT, pi);
            atomicOr(&pg.done, DONE_DSTR | DONE_FLAT);
        }
        return;
    }
    // ---- offsets
    const uint64_t slot_base = uint64_t(pg.entry_start);
    if (n > 0) {
        uint32_t o[16];
        uint32_t c = uint32_t(char_base) + lo_c;
        #pragma unroll
        for (uint32_t k = 0; k < 16; k++) { c += pl[k] >> 16; o[k] = c; }
        int32_t* op = ck.offsets + slot_base + e0 + 1;
        if (n == 16) {
            switch ((4u - uint32_t((reinterpret_cast<uintptr_t>(op) >> 2) & 3u)) & 3u) {
                case 0: store_offs16<0>(op, o); break;
                case 1: store_offs16<1>(op, o); break;
                case 2: store_offs16<2>(op, o); break;
                default: store_offs16<3>(op, o); break;
            }
        } else {
            #pragma unroll
            for (uint32_t k = 0; k < 16; k++) if (k < n) op[k] = int32_t(o[k]);
        }
    }
    // ---- validity: every level is present
    if (ck.max_def > 0 && ck.validity) {
        const uint64_t v0 = slot_base + b0, v1 = slot_base + b1;
        uint32_t* vw = reinterpret_cast<uint32_t*>(ck.validity);
        for (uint64_t wd = (v0 >> 5) + tid; wd <= ((v1 - 1) >> 5); wd += NT) {
            const uint64_t l = max(v0, wd << 5), h = min(v1, (wd + 1) << 5);
            const uint32_t m = uint32_t((h - l >= 32 ? 0xffffffffull : ((1ull << (h - l)) - 1ull)) << (l & 31));
            if (l == (wd << 5) && h == ((wd + 1) << 5)) vw[wd] = m;
            else atomicOr(vw + wd, m);
        }
    }
    // ---- chars: windows of DSTR_WIN bytes of the 16-byte grid of the output, assembled in LDS.
    // Position v of that grid is output address g0 + v; the block's chars are [a0c, vend).
    const uintptr_t gout = reinterpret_cast<uintptr_t>(ck.chars + char_base);
    const uint32_t a0c = uint32_t(gout & 15u);
    const uintptr_t g0 = gout - a0c;
    const uint32_t vend = a0c + tot, my0 = a0c + lo_c;
    uint8_t* const w8 = reinterpret_cast<uint8_t*>(S.win);
    const uint8_t* const d8 = reinterpret_cast<const uint8_t*>(S.dict);
    for (uint32_t w0 = 0; w0 < vend && tot > 0; w0 += DSTR_WIN) {
        const uint32_t w1 = min(vend, w0 + DSTR_WIN);
        if (w0 > 0) __syncthreads();   // the previous window has left
        if (my0 < w1 && my0 + lsum > w0) {
            uint32_t v = my0;
            #pragma unroll
            for (uint32_t k = 0; k < 16; k++) {
                const uint32_t len = pl[k] >> 16, pos = pl[k] & 0xffffu;
                const uint32_t s0 = max(v, w0), s1 = min(v + len, w1);
                for (uint32_t b = s0; b < s1; b++) w8[b - w0] = d8[pos + (b - v)];
                v += len;
            }
        }
        __syncthreads();
        for (uint32_t ci = tid; ci < (w1 - w0 + 15u) / 16u; ci += NT) {
            const uint32_t vp = w0 + 16u * ci;
            if (vp >= a0c && vp + 16u <= vend) {
                *reinterpret_cast<PF_GLOBAL u32x4*>(g0 + vp) = S.win[ci];
            } else {   // the block's first and last chunk: the other bytes are a neighbour's
                for (uint32_t b = 0; b < 16u; b++)
                    if (vp + b >= a0c && vp + b < vend) reinterpret_cast<uint8_t*>(g0 + vp)[b] = w8[16u * ci + b];
            }
        }
    }
    if (tid == 0) {
        // DONE_FLAT with it: the page was decoded by a flat kernel, which is what that bit tells k_decode and the tools
        atomicOr(&pg.done, DONE_DSTR | DONE_FLAT);
        DSTR_COUNT(0);
    }
}

// k_flat_fixed and k_flat in one launch over the same (page, block) list: a block decodes its page
// with the fixed-width body when that applies, else with the general body. One stage instead of
// two in stream order (the fixed-width columns' blocks no longer wait for the string blocks or the
// other way round); the LDS of the two bodies is shared (they never run in one block together).
#ifndef PF_FLAT_OCC
#define PF_FLAT_OCC 5   // round 5 (with CV_CAP 2048 and the chars copies inlined): SF1 2.74 -> 2.69 ms; 4 before
#endif
// Workgroups n.. of the grid take the fallback queue (round 6: k_flat_fb's launch folded in; the producers
// of the queue, k_flat_fixed and k_flat_null, are earlier in stream order): a grid stride over the queued
// blocks, nearly always none.
__global__ __launch_bounds__(NT, PF_FLAT_OCC) void k_flat_all(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                 const int2* __restrict__ blocks, int n, const int* __restrict__ fbq,
                                                 DevChunkResult* res) {
    __shared__ union FlatAllLds {
        FixedLds f;
        FlatLds g;
    } S;
    if (int(blockIdx.x) >= n) {
        const int nq = fbq[0], g = int(gridDim.x) - n;
        for (int i = int(blockIdx.x) - n; i < nq; i += g) {
            const int2 pq = reinterpret_cast<const int2*>(fbq + 4)[i];
            if (!flat_fixed_block(S.f, chunks, pages, pq, res)) {
                __syncthreads();
                flat_block(S.g, chunks, pages, pq, res);
            }
            __syncthreads();   // the block's LDS reads are done before the next one reuses it
        }
        return;
    }
    const int2 pbk = blocks[blockIdx.x];
    if (flat_fixed_block(S.f, chunks, pages, pbk, res)) return;
    __syncthreads();   // the fixed body's LDS reads are done before the general body reuses it
    flat_block(S.g, chunks, pages, pbk, res);
}

// ---- nullable flat pages: definition-level run table + block-parallel decode ------------------
//
// north_star K2/K6: "RLE/bit-packed-hybrid expansion of definition levels ... using prefix scans to
// find run boundaries" and null scatter. k_lvl walks a page's level run headers once (they are few:
// ~300 per 20,000 entries at 30 % random nulls), counts the present values of every run in parallel
// and scans them, so that every 4096-entry block of the page knows the value index of its first
// present entry. k_flat_null then decodes the blocks in parallel: levels -> present bits -> block
// scan -> value index -> dictionary gather / PLAIN load; null slots are zero.
constexpr uint32_t LVL_STAGE = 4096;   // level sections up to this size are decoded from LDS (k_lvl)

// Bits [bit, bit + k) (k <= 32) of an LDS byte array (LSB-first), from the two aligned dwords around it.
__device__ __forceinline__ uint32_t lds_bits(const uint8_t* st, uint32_t bit, uint32_t k) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(st);
    const uint32_t wi = bit >> 5, sh = bit & 31u;
    const uint64_t v = uint64_t(w[wi]) | (uint64_t(w[wi + 1]) << 32);
    return uint32_t(v >> sh) & (k >= 32 ? 0xffffffffu : ((1u << k) - 1u));
}

// Last level run with first entry <= e (runs: k_lvl's run rows, runs[0].first == 0).
__device__ __forceinline__ uint32_t lvl_run_at(const LvlRun* runs, uint32_t nr, uint32_t e) {
    return last_row_le(nr, e, [runs](uint32_t r) { return lvl_run(runs, r).first; });
}
// Present values before entry e, which lies in run r (its present-before count plus the present
// levels of the run before e, from the staged level section).
__device__ inline uint32_t lvl_values_before(const LvlRun* runs, uint32_t r, uint32_t e, const uint8_t* stage,
                                             uint32_t woff, int bw, uint32_t maxd) {
    const uint32_t first = lvl_run(runs, r).first, data = lvl_run(runs, r).data;
    const uint32_t before = e - first;
    uint32_t vb = lvl_run(runs, r).before;
    if (!lvl_run(runs, r).packed()) return vb + (data == maxd ? before : 0u);
    if (bw == 1) {
        for (uint32_t i = 0; i < before; i += 32) {
            const uint32_t k = min(32u, before - i), bb = woff * 8u + data + i;
            if (bb + k <= LVL_STAGE * 8u) vb += __popc(lds_bits(stage, bb, k));
        }
    } else {
        for (uint32_t i = 0; i < before; i++) {
            const uint32_t bb = woff * 8u + data + i * uint32_t(bw);
            if (bb + uint32_t(bw) <= LVL_STAGE * 8u) vb += lds_bits(stage, bb, uint32_t(bw)) == maxd;
        }
    }
    return vb;
}
// Dictionary-id run (k_runs table T) holding value v.
__device__ __forceinline__ uint32_t id_run_at(const IdRunTab* T, uint32_t nr, uint32_t v) {
    return last_row_le(nr, v, [T](uint32_t r) { return T->first(r); });
}

constexpr int LT_NT = 256;                // k_lvl: four waves per page
constexpr uint32_t LVL_RUNS_LDS = 512;    // level runs k_lvl keeps in LDS (pages with more read them from HBM)
constexpr uint32_t LVL_NXT = 4096;        // = LVL_STAGE: k_lvl's all-positions header tables cover its sections
constexpr uint32_t LVL_JUMP = 8;          // runs per step of k_lvl's chain walk (jump table: 3 doubling passes)
constexpr uint32_t LVL_S8 = LVL_NXT / LVL_JUMP;   // walk steps (a run is at least one byte)
constexpr uint32_t LVL_PPT = LVL_NXT / LT_NT;     // section positions per thread in the table passes
static_assert(LVL_PPT == 16, "k_lvl's mark words: two threads per 32 positions");
#ifndef PF_LVL_OCC
#define PF_LVL_OCC 1   // k_lvl workgroups per CU the register budget must allow (1: the compiler's choice, 114 VGPRs;
                       // 5: 96 VGPRs + 80 B scratch, config 4 3.70-3.75 vs 3.68-3.74 ms, not kept)
#endif
__global__ __launch_bounds__(LT_NT, PF_LVL_OCC) void k_lvl(const DevChunk* __restrict__ chunks, DevPage* pages, const int* __restrict__ list,
                                               DevChunkResult* res, uint32_t dcap, uint32_t icap) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[LVL_STAGE + 48];
    __shared__ uint32_t scan_tmp[LT_NT / 64];
    __shared__ uint32_t s_ns8;
    // next-header positions of every byte position (0xffff: not a header, or its run passes the
    // section end; dn: the chain ends there), then the page's dictionary-id runs (k_runs) for the
    // block table
    __shared__ union { uint16_t nxt[LVL_NXT]; IdRunTab T; } s_u;
    // the 8-run jump table during the chain walk, then the LDS copy of the level runs
    __shared__ union { uint16_t jmp[LVL_NXT]; LvlRun runs[LVL_RUNS_LDS]; } s_a;
    __shared__ uint16_t s_s8[LVL_S8];         // chain positions of runs 0, 8, 16, ...
    __shared__ uint32_t s_mark[LVL_NXT / 32];  // chain positions (run headers)
    static_assert(sizeof(uint16_t) * LVL_NXT >= sizeof(IdRunTab), "s_u sized by the header table");
    uint16_t* const s_nxt = s_u.nxt;
    IdRunTab* const s_T = &s_u.T;
    uint16_t* const s_jmp = s_a.jmp;
    LvlRun* const s_runs = s_a.runs;
    const int pi = list[blockIdx.x];
    DevPage& pg = pages[pi];
    LvlHead* LT = pg.lvltab;
    if (!LT) return;
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    Sections s;
    if (pg.done & DONE_PAGE) {   // k_page_null decoded the page
        if (tid == 0) LT->fit = 0;
        return;
    }
    if (res[pg.chunk].status != 0 || ck.max_rep != 0 || ck.max_def <= 0 || !page_sections(pg, ck, s) || !s.def_rle ||
        s.def_n > LVL_STAGE) {   // (longer level sections: k_flat / k_decode)
        if (tid == 0) LT->fit = 0;
        return;
    }
    const uint32_t ne = uint32_t(pg.num_values);
    const int bw = bit_width(uint32_t(ck.max_def));
    const uint32_t maxd = uint32_t(ck.max_def);
    const uint32_t dn = uint32_t(s.def_n);
#ifdef PF_STAMPS   // phase cycles per page (tools/probe_wide.py): 8 pages, 9 stage, 10 header table, 11 chain,
                   // 12 run decode, 13 present counts, 14 block table, 15 total; 6 runs, 7 level bytes
    unsigned long long lt_ = __builtin_amdgcn_s_memtime(), lt0_ = lt_;
#define LTS(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (tid == 0) PSTAMP(i, t_ - lt_); lt_ = t_; } while (0)
    if (tid == 0) { PSTAMP(8, 1); PSTAMP(7, dn); }
#else
#define LTS(i) ((void)0)
#endif
    // stage the level section with aligned 16-byte loads: section byte i is stage[woff + i]; bytes
    // past the section read as zero (parquet-mr zero-pads a truncated bit-packed run)
    const uintptr_t sa = reinterpret_cast<uintptr_t>(s.def);
    const uint32_t woff = uint32_t(sa & 15u);
    if (woff + dn > LVL_STAGE) {
        if (tid == 0) LT->fit = 0;
        return;
    }
    {
        const PF_GLOBAL u32x4* src = (const PF_GLOBAL u32x4*)(sa - woff);
        const uint32_t nchunk = (woff + dn + 15u) / 16u;
        for (uint32_t c = tid; c < nchunk; c += LT_NT) reinterpret_cast<u32x4*>(stage)[c] = src[c];
        if (uint32_t(tid) < LVL_NXT / 32) s_mark[tid] = 0;
        __syncthreads();
        for (uint32_t i = woff + dn + uint32_t(tid); i < nchunk * 16u + 16u; i += LT_NT) stage[i] = 0;
        __syncthreads();
    }
    LTS(9);
    LvlRun* runs = lvl_runs(LT);
    const uint32_t cap = pg.lvl_cap;
    const uint8_t* const stw = stage + woff;
    // (1) every byte position decoded as a run header: the position of the next header
    for (uint32_t p = tid; p < dn; p += LT_NT) {
        uint32_t h = 0, hl = 0, nx = 0xffffu;
        #pragma unroll
        for (uint32_t k = 0; k < 3; k++) {   // headers over 2^21 are no runs of a <= 4 KiB section
            const uint32_t c = p + k < dn ? uint32_t(stw[p + k]) : 0x80u;
            h |= (c & 0x7fu) << (7 * k);
            if (!(c & 0x80u)) { hl = k + 1; break; }
        }
        if (hl) {
            const uint32_t pay = (h & 1u) ? (h >> 1) * uint32_t(bw) : (uint32_t(bw) + 7u) >> 3;
            if (p + hl + pay <= dn) nx = p + hl + pay;   // a truncated run ends the chain
        }
        s_nxt[p] = uint16_t(nx);
    }
    __syncthreads();
    LTS(10);
    // (2) the chain from position 0 (north_star K2: run boundaries by wavefront passes). The 8-run jump
    // table by three doubling passes, one thread walks it eight runs a step, then one thread per
    // 8-run stretch walks the runs in between and marks their headers. Terminal values stay put:
    // 0xffff (broken chain) and positions >= dn (the section end).
    {
        uint32_t J[LVL_PPT];
        #pragma unroll
        for (uint32_t k = 0; k < LVL_PPT; k++) {
            const uint32_t p = uint32_t(tid) + k * LT_NT;
            const uint32_t q = p < dn ? uint32_t(s_nxt[p]) : 0xffffu;
            J[k] = q < dn ? uint32_t(s_nxt[q]) : q;
        }
        #pragma unroll
        for (uint32_t k = 0; k < LVL_PPT; k++) s_jmp[uint32_t(tid) + k * LT_NT] = uint16_t(J[k]);
        __syncthreads();
        for (int pass = 0; pass < 2; pass++) {   // 2 -> 4 -> 8 runs
            #pragma unroll
            for (uint32_t k = 0; k < LVL_PPT; k++) J[k] = J[k] < dn ? uint32_t(s_jmp[J[k]]) : J[k];
            __syncthreads();
            #pragma unroll
            for (uint32_t k = 0; k < LVL_PPT; k++) s_jmp[uint32_t(tid) + k * LT_NT] = uint16_t(J[k]);
            __syncthreads();
        }
    }
    if (tid == 0) {
        uint32_t p = 0, k = 0;
        while (p < dn && k < LVL_S8) {
            s_s8[k++] = uint16_t(p);
            const uint32_t q = s_jmp[p];
            if (q >= dn) break;   // the chain ends (or breaks) within the next 8 runs
            p = q;
        }
        s_ns8 = k;
    }
    __syncthreads();
    const uint32_t ns8 = s_ns8;
    for (uint32_t j = tid; j < ns8; j += LT_NT) {
        uint32_t p = s_s8[j];
        for (uint32_t i = 0; i < LVL_JUMP && p < dn; i++) {
            const uint32_t q = s_nxt[p];
            if (q == 0xffffu) break;   // no run header here: the chain is broken
            atomicOr(&s_mark[p >> 5], 1u << (p & 31u));
            p = q;
        }
    }
    __syncthreads();
    LTS(11);
    // (3) the marked headers in position order: runs decoded at their headers in parallel, their
    // first entries an exclusive scan of the counts, runs with entries at or past the page's dropped
    const uint32_t mw = s_mark[tid >> 1];   // a thread's 16 positions: half a mark word
    const uint32_t mbits = (mw >> (16u * (uint32_t(tid) & 1u))) & 0xffffu;
    const uint32_t p0 = 16u * uint32_t(tid);
    uint32_t hcnt[LVL_PPT], hdat[LVL_PPT], hpk = 0;
    uint64_t csum = 0;
    #pragma unroll
    for (uint32_t k = 0; k < LVL_PPT; k++) {
        hcnt[k] = 0;
        hdat[k] = 0;
        if (!((mbits >> k) & 1u)) continue;
        const uint32_t P = p0 + k;
        uint32_t h = 0, hl = 0;
        for (uint32_t b = 0; b < 3; b++) {
            const uint32_t c = stw[P + b];
            h |= (c & 0x7fu) << (7 * b);
            if (!(c & 0x80u)) { hl = b + 1; break; }
        }
        const uint32_t packed = h & 1u;
        hcnt[k] = packed ? (h >> 1) * 8u : (h >> 1);
        if (packed) hdat[k] = (P + hl) * 8u;
        else for (uint32_t b = 0; b < ((uint32_t(bw) + 7u) >> 3); b++) hdat[k] |= uint32_t(stw[P + hl + b]) << (8 * b);
        hpk |= packed << k;
        csum += hcnt[k];
    }
    __shared__ unsigned long long scan64[LT_NT / 64];
    uint64_t ctot;
    const uint64_t cbase = block_excl_scan64<LT_NT>(csum, scan64, ctot);
    uint32_t emask = 0, bad = 0;
    {
        uint64_t f = cbase;
        #pragma unroll
        for (uint32_t k = 0; k < LVL_PPT; k++) {
            if (hcnt[k] > 0 && f < ne) {
                emask |= 1u << k;
                if (!((hpk >> k) & 1u) && hdat[k] > maxd) bad = 1;
            }
            f += hcnt[k];
        }
    }
    __syncthreads();   // scan_tmp is reused
    uint32_t nr;
    const uint32_t rbase = block_excl_scan<LT_NT>(__popc(emask), scan_tmp, nr);
    {
        uint64_t f = cbase;
        uint32_t rank = rbase;
        #pragma unroll
        for (uint32_t k = 0; k < LVL_PPT; k++) {
            if ((emask >> k) & 1u && nr <= cap) {   // (emitted: f < ne)
                const uint32_t c = uint32_t(min<uint64_t>(hcnt[k], uint64_t(ne) - f));
                const uint32_t cw = c | (((hpk >> k) & 1u) << 31);
                lvl_run(runs, rank).first = uint32_t(f);
                lvl_run(runs, rank).data = hdat[k];
                lvl_run(runs, rank).cw = cw;
                if (rank < LVL_RUNS_LDS) {
                    lvl_run(s_runs, rank).first = uint32_t(f);
                    lvl_run(s_runs, rank).data = hdat[k];
                    lvl_run(s_runs, rank).cw = cw;
                }
                rank++;
            }
            f += hcnt[k];
        }
    }
    __threadfence_block();   // the run records (HBM and LDS) before the other waves read them
    const bool ok = __syncthreads_or(bad) == 0 && nr <= cap && ctot >= ne;   // (a broken chain covers too few)
    LTS(12);
    if (!ok) {
        if (tid == 0) LT->fit = 0;
        return;
    }
    LvlRun* const R = nr <= LVL_RUNS_LDS ? s_runs : runs;   // the scans below read this copy
    uint32_t carry = 0;
    for (uint32_t r0 = 0; r0 < nr; r0 += LT_NT) {
        const uint32_t r = r0 + uint32_t(tid);
        uint32_t pc = 0;
        if (r < nr) {
            const uint32_t data = lvl_run(R, r).data, cnt = lvl_run(R, r).count();
            if (!lvl_run(R, r).packed()) pc = data == maxd ? cnt : 0u;
            else {
                // packed levels [data, data + cnt * bw) bits (the stage is zero past the section)
                const uint32_t nbits = cnt * uint32_t(bw);
                const uint32_t b0 = woff * 8u + data;
                if (bw == 1) {
                    for (uint32_t i = 0; i < nbits; i += 32) {
                        const uint32_t k = min(32u, nbits - i);
                        if (b0 + i + k <= LVL_STAGE * 8u) pc += __popc(lds_bits(stage, b0 + i, k));
                    }
                } else {
                    for (uint32_t i = 0; i < cnt; i++) {
                        const uint32_t b = b0 + i * uint32_t(bw);
                        if (b + uint32_t(bw) <= LVL_STAGE * 8u) pc += lds_bits(stage, b, uint32_t(bw)) == maxd;
                    }
                }
            }
        }
        uint32_t tot;
        const uint32_t ex = block_excl_scan<LT_NT>(pc, scan_tmp, tot);
        if (r < nr) {
            lvl_run(runs, r).before = carry + ex;
            if (R != runs) lvl_run(R, r).before = carry + ex;
        }
        carry += tot;
        __syncthreads();   // scan_tmp is reused
    }
    LTS(13);
    // per FBLK block (k_flat_null): the runs it overlaps [r0, r1), the value indices of its first and
    // end entries, the level bytes its packed runs read and the dictionary-id bytes of its values
    __threadfence_block();
    const uint32_t nblk = (ne + FBLK - 1) / FBLK;
    // dictionary id runs (k_runs, same stream): value index -> bit offset in the id stream
    const IdRunTab* TG = pg.runtab;
    const bool dict = is_dict_enc(pg.encoding) && TG != nullptr && TG->valid == 1u && TG->nruns <= uint32_t(RUN_CAP) && s.val_n > 0;
    const uint32_t tnr = dict ? TG->nruns : 0u, tcov = dict ? TG->covered : 0u;
    if (dict)
        for (uint32_t i = tid; i < id_tab_words(tnr); i += LT_NT)
            reinterpret_cast<uint32_t*>(s_T)[i] = reinterpret_cast<const uint32_t*>(TG)[i];
    __syncthreads();
    const IdRunTab* T = s_T;
    const uint32_t id_bw = dict ? uint32_t(s.val[0]) : 0u;
    uint32_t fit = 1;
    for (uint32_t b = tid; b < nblk; b += LT_NT) {
        const uint32_t eb = b * FBLK, ee = min(ne, eb + FBLK);
        const uint32_t lo = lvl_run_at(R, nr, eb);
        uint32_t a = lo, z = nr;    // first run with first >= ee
        while (a < z) {
            const uint32_t m = (a + z) >> 1;
            if (lvl_run(R, m).first < ee) a = m + 1; else z = m;
        }
        const uint32_t vb = lvl_values_before(R, lo, eb, stage, woff, bw, maxd);
        const uint32_t ve = ee == ne ? carry : lvl_values_before(R, lvl_run_at(R, nr, ee), ee, stage, woff, bw, maxd);
        // level bytes: from the first packed run's first bit to the last packed run's end
        uint32_t d0 = 0, d1 = 0;
        for (uint32_t r = lo; r < a; r++) {
            if (!lvl_run(R, r).packed()) continue;
            const uint32_t f = lvl_run(R, r).first;
            d0 = (lvl_run(R, r).data + (max(eb, f) - f) * uint32_t(bw)) >> 3;
            break;
        }
        for (uint32_t r = a; r > lo; r--) {
            if (!lvl_run(R, r - 1).packed()) continue;
            const uint32_t f = lvl_run(R, r - 1).first, end = min(ee, f + lvl_run(R, r - 1).count());
            d1 = (lvl_run(R, r - 1).data + (end - f) * uint32_t(bw) + 7u) >> 3;
            break;
        }
        // dictionary-id bytes of values [vb, ve)
        uint32_t i0 = 0, i1 = 0;
        if (dict && ve > vb) {
            if (ve > tcov) fit = 0;
            else {
                const uint32_t q0 = id_run_at(T, tnr, vb), q1 = id_run_at(T, tnr, ve - 1);
                for (uint32_t q = q0; q <= q1; q++) {
                    if (!T->packed(q)) continue;
                    const uint32_t f = T->first(q);
                    i0 = uint32_t((uint64_t(T->data(q)) + uint64_t(max(vb, f) - f) * id_bw) >> 3);
                    break;
                }
                for (uint32_t q = q1 + 1; q > q0; q--) {
                    if (!T->packed(q - 1)) continue;
                    const uint32_t f = T->first(q - 1);
                    const uint32_t nf = q < tnr ? T->first(q) : tcov;
                    i1 = uint32_t((uint64_t(T->data(q - 1)) + uint64_t(min(ve, nf) - f) * id_bw + 7u) >> 3);
                    break;
                }
            }
        }
        if (a - lo > LT_BLOCK_RUNS || d1 - d0 + 16u > dcap || i1 - i0 + 16u > icap || ve < vb) fit = 0;
        *lvl_block(LT, cap, b) = LvlBlock{lo, a, vb, ve, d0, d1, i0, i1};
    }
    fit = __syncthreads_and(fit) ? 1u : 0u;
    if (tid == 0) { LT->nruns = nr; LT->present = carry; LT->fit = fit; }
    LTS(14);
#ifdef PF_STAMPS
    if (tid == 0) PSTAMP(15, __builtin_amdgcn_s_memtime() - lt0_);
    if (tid == 0) PSTAMP(6, nr);
#endif
#undef LTS
}

// k_flat_null<W>: one 256-thread workgroup per 4096-entry block of a nullable W-byte page, 16
// consecutive entries per thread. The block's level runs, the page's id runs and the level / id bytes
// the block reads (k_lvl's block table) are all fetched at once into LDS, so the workgroup waits on one
// round of loads, then on the dictionary gather; no spread step: entry k of a thread takes the value of
// rank popc(fv & (2^k - 1)). The stage is latency-bound (Σ block latency / resident blocks), so what
// sets it is the entries in flight per CU: 16 per lane (round 5; 8 per lane at 512 threads: config 4's
// flat launch 0.97 -> 0.81 ms, gpurun_out/ntn). The runtime gives the kernel only nullable pages of its
// width (its own block lists); a page it does not take goes to the fallback queue (k_flat_all's last workgroups).
#ifndef PF_NTN
#define PF_NTN 256
#endif
constexpr int NTN = PF_NTN;
constexpr int NEPT = FBLK / NTN;   // 8 (512 threads) or 16 (256)
static_assert(NEPT % 4 == 0 && NEPT <= 16, "k_flat_null's stores and present masks");
// Runs in LDS as {first | packed << 31, data}: a run ends where the next begins (k_lvl's level runs
// and k_runs' id runs are contiguous), and one sentinel row after the last holds its end.
struct NullLds {
    uint2 drun[LT_BLOCK_RUNS + 1];
    uint2 vrun[RUN_CAP + 1];
    uint32_t vbits[FBLK / 32 + 2];
    uint32_t scan_tmp[NTN / 64];
};
__device__ __forceinline__ uint32_t rl_first(uint2 r) { return r.x & 0x7fffffffu; }
__device__ __forceinline__ int rl_find(const uint2* runs, int nr, uint32_t i) {   // run holding i (runs[0] first <= i)
    return last_row_le(nr, i, [runs](int r) { return rl_first(runs[r]); });
}

// Dynamic LDS, sized by the host per batch (NullCaps): the block's level bytes (dcap + 32), its
// dictionary-id bytes (icap + 32) -- caps from the batch's level and id bit widths, which k_lvl's
// block table was checked against -- and dictionaries of at most dlds bytes (the batch's largest
// fitting one, <= NULL_DICT_LDS; 0 when it has none), gathered from LDS (north_star K3: "dictionary
// staged in LDS when it fits"); larger ones are gathered from L2 / HBM. Config 4 (1-bit levels,
// 17-bit ids): ~16.6 KiB a workgroup, eight resident per CU (the VGPR limit) instead of five.

template <int W> struct WidthType { using type = uint64_t; };
template <> struct WidthType<4> { using type = uint32_t; };

template <int W>
__global__ __launch_bounds__(NTN) void k_flat_null(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                   const int2* __restrict__ blocks, DevChunkResult* res, NullCaps nc,
                                                   int stagger, int* fbq) {
    using VT = typename WidthType<W>::type;
    __shared__ __attribute__((aligned(16))) NullLds S;
    extern __shared__ __attribute__((aligned(16))) uint64_t DYN[];
    uint32_t* const s_dst = reinterpret_cast<uint32_t*>(DYN);
    uint32_t* const s_ist = s_dst + (nc.dcap + 32u) / 4u;
    uint64_t* const DL = reinterpret_cast<uint64_t*>(s_ist + (nc.icap + 32u) / 4u);
    const uint32_t dlds = nc.dlds;
    const int2 pbk = blocks[blockIdx.x];
#ifdef PF_DIAG   // diagnostics build (tests): blocks after a page's first start late, after it has finished
    if (stagger && pbk.y > 0)
        for (int i = 0; i < stagger; i++) __builtin_amdgcn_s_sleep(127);
#else
    (void)stagger;
#endif
    if (pbk.x < 0) return;   // padding of the XCD-grouped block list (runtime)
#ifdef PF_STAMPS   // phase cycles per block: 0 blocks, 1 tables, 2 LDS stage, 3 levels + scan, 4 gather + store
    unsigned long long t_ph = __builtin_amdgcn_s_memtime(), t_beg = t_ph;
#define NSTAMP(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (threadIdx.x == 0) PSTAMP(i, t_ - t_ph); t_ph = t_; }
#else
#define NSTAMP(i) ((void)0)
#endif
    const int pi = pbk.x;
    const uint32_t blk = uint32_t(pbk.y) & 0x0fffffffu;   // (pages with a level table always have FBLK blocks)
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    LvlHead* const LT = pg.lvltab;
    // pages this kernel does not take (whole pages: the conditions are the page's) go to the fallback queue
    // (not DONE_NULL: blocks of this page that finished first set it, and a block starting later must still run)
    if (!LT || res[pg.chunk].status != 0 || ck.max_rep != 0 || ck.width != W ||
        (pg.done & (DONE_FIXED | DONE_PAGE)) || LT->fit != 1u) {   // (k_page_null took it, or no block table)
        null_fallback(fbq, pbk);
        return;
    }
    Sections s;
    const int enc = pg.encoding;
    const bool dict = is_dict_enc(enc);
    const IdRunTab* T = pg.runtab;
    if (!page_sections(pg, ck, s) || (!dict && enc != 0) ||
        (dict && !(T != nullptr && T->valid == 1u && T->nruns <= uint32_t(RUN_CAP) && s.val_n > 0 && ck.dict_data != nullptr))) {
        null_fallback(fbq, pbk);
        return;
    }
    const uint32_t ne = uint32_t(pg.num_values);
    const uint32_t e_begin = blk * FBLK;
    if (blk > 0 && e_begin >= ne) return;
    const uint32_t e_end = min(ne, e_begin + FBLK);
    constexpr int w = W;
    const int bw = bit_width(uint32_t(ck.max_def));
    const uint32_t maxd = uint32_t(ck.max_def);
    const uint32_t nr = LT->nruns;
    const LvlRun* runs = lvl_runs(LT);
    const LvlBlock& bt = *lvl_block(LT, pg.lvl_cap, blk);
    const uint32_t r0 = bt.r0, r1 = bt.r1, vb = bt.vb, ve = bt.ve, d0 = bt.d0, d1 = bt.d1, i0 = bt.i0, i1 = bt.i1;
    const uint32_t id_bw = dict ? uint32_t(s.val[0]) : 0u;
    const uint32_t vnr = dict ? T->nruns : 0u;
    const uint32_t idcov = dict ? T->covered : 0u;
    const uint8_t* ids = dict ? s.val + 1 : nullptr;
    const uint64_t ids_n = dict ? s.val_n - 1 : 0;
    if (r1 < r0 || (r1 == r0 && e_end > e_begin) || r1 - r0 > LT_BLOCK_RUNS || r1 > nr || id_bw > 32 || ve < vb || d1 < d0 || d1 - d0 + 16u > nc.dcap ||
        i1 < i0 || i1 - i0 + 16u > nc.icap || (dict && ve > idcov) || (!dict && uint64_t(ve) * uint64_t(w) > s.val_n)) {
        if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi);
        return;
    }
    NSTAMP(1);
    // one round of loads: level runs, id runs, level bytes, id bytes
    const uint32_t nrun = r1 - r0;
    for (uint32_t i = tid; i < nrun; i += NTN) {
        const LvlRun& q = lvl_run(runs, r0 + i);
        const uint32_t f = q.first, d = q.data, c = q.cw;
        S.drun[i] = make_uint2(f | (c & 0x80000000u), d);
        if (i + 1 == nrun) S.drun[nrun] = make_uint2(f + (c & 0x7fffffffu), 0u);
    }
    for (uint32_t i = tid; i <= vnr; i += NTN)
        S.vrun[i] = i < vnr ? make_uint2(T->fp(i), T->data(i)) : make_uint2(idcov, 0u);
    const uint32_t doff = stage_bytes(s_dst, s.def, s.def_n, d0, d1);
    const uint32_t ioff = dict ? stage_bytes(s_ist, ids, ids_n, i0, i1) : 0u;
    for (uint32_t i = tid; i < FBLK / 32 + 2; i += NTN) S.vbits[i] = 0;
    const bool dl = dict && dlds != 0 && ck.dict_n > 0 && uint64_t(ck.dict_n) * uint64_t(w) <= dlds &&
                    (reinterpret_cast<uintptr_t>(ck.dict_data) & 7u) == 0;
    if (dl) {   // the dictionary into LDS (8-byte loads; the page body is 16-byte aligned scratch)
        const uint64_t* g = reinterpret_cast<const uint64_t*>(ck.dict_data);
        const uint32_t nw = uint32_t((uint64_t(ck.dict_n) * uint64_t(w) + 7u) / 8u);
        for (uint32_t i = tid; i < nw; i += NTN) DL[i] = g[i];
    }
    __syncthreads();
    NSTAMP(2);
    const uint8_t* dst8 = reinterpret_cast<const uint8_t*>(s_dst);
    const uint8_t* ist8 = reinterpret_cast<const uint8_t*>(s_ist);
    const uint32_t dbase = d0 * 8u - doff * 8u;   // stream bit of LDS bit 0
    const uint32_t ibase = i0 * 8u - ioff * 8u;
    const uint32_t dlim = (d1 - d0 + doff + 16u) * 8u;   // readable LDS bits
    const uint32_t ilim = (i1 - i0 + ioff + 16u) * 8u;
    int bad = 0;
    // present bits of this thread's entries
    const uint32_t e = e_begin + uint32_t(tid) * NEPT;
    const uint32_t m = e < e_end ? min(uint32_t(NEPT), e_end - e) : 0u;
    uint32_t fv = 0;
    if (m) {
        int r = rl_find(S.drun, int(nrun), e);
        const uint2 R = S.drun[r];
        const uint32_t Rf = rl_first(R), Rp = R.x >> 31;
        if (e + m <= rl_first(S.drun[r + 1]) && (!Rp || bw == 1)) {   // one run
            if (!Rp) fv = R.y == maxd ? ((1u << m) - 1u) : 0u;
            else {
                const uint32_t b = R.y + (e - Rf) - dbase;
                fv = b + m <= dlim ? lds_bits(dst8, b, m) : 0u;
                bad |= b + m > dlim;
            }
        } else {
            for (uint32_t k = 0; k < m; k++) {
                while (r + 1 < int(nrun) && e + k >= rl_first(S.drun[r + 1])) r++;
                const uint2 Rk = S.drun[r];
                uint32_t dl = Rk.y;
                if (Rk.x >> 31) {
                    const uint32_t b = Rk.y + (e + k - rl_first(Rk)) * uint32_t(bw) - dbase;
                    bad |= b + uint32_t(bw) > dlim;
                    dl = b + uint32_t(bw) <= dlim ? lds_bits(dst8, b, uint32_t(bw)) : 0u;
                }
                bad |= dl > maxd;
                fv |= uint32_t(dl == maxd) << k;
            }
        }
    }
    uint32_t tv;
    const uint32_t vo = block_excl_scan<NTN>(__popc(fv), S.scan_tmp, tv);
    if (tv != ve - vb) bad = 1;   // the block table disagrees with the levels
    NSTAMP(3);
    const uint32_t gv0 = vb + vo;   // value index of this thread's first present entry
    VT v[NEPT];
    #pragma unroll
    for (int k = 0; k < NEPT; k++) v[k] = 0;
    if (fv && !bad) {
        // Two phases: the ids of the present entries (LDS only), then ALL of the thread's gathers
        // issued back to back through global-address-space loads (absent entries load element 0 and
        // are zeroed after), so the wave waits on one round of L2 / HBM latency instead of one per
        // entry (flat loads under per-entry branches each ended in a vmcnt(0) wait).
        if (dict) {
            uint32_t idv[NEPT];
            #pragma unroll
            for (int k = 0; k < NEPT; k++) idv[k] = 0;
            int vr = rl_find(S.vrun, int(vnr), gv0);
            const uint2 V0 = S.vrun[vr];
            // the thread's present values are gv0, gv0 + 1, ...: when one id run holds them all, their
            // ids are consecutive fields of that run (no run search per value)
            const bool one_run = gv0 + uint32_t(__popc(fv)) <= rl_first(S.vrun[vr + 1]);
            const uint32_t b0 = (V0.x >> 31) ? uint32_t(uint64_t(V0.y) + uint64_t(gv0 - rl_first(V0)) * id_bw - ibase) : 0u;
            const int64_t dn = ck.dict_n;
            uint32_t r = 0;
            #pragma unroll
            for (int k = 0; k < NEPT; k++) {
                if (!((fv >> k) & 1u)) continue;
                uint32_t id;
                if (one_run) {
                    id = V0.y;
                    if (V0.x >> 31) {
                        const uint32_t b = b0 + r * id_bw;
                        bad |= b + id_bw > ilim;
                        id = b + id_bw <= ilim ? lds_bits(ist8, b, id_bw) : 0u;
                    }
                } else {
                    const uint32_t gv = gv0 + r;
                    while (vr + 1 < int(vnr) && gv >= rl_first(S.vrun[vr + 1])) vr++;
                    const uint2 V = S.vrun[vr];
                    id = V.y;
                    if (V.x >> 31) {
                        const uint32_t b = uint32_t(uint64_t(V.y) + uint64_t(gv - rl_first(V)) * id_bw - ibase);
                        bad |= b + id_bw > ilim;
                        id = b + id_bw <= ilim ? lds_bits(ist8, b, id_bw) : 0u;
                    }
                }
                r++;
                bad |= int64_t(id) >= dn;
                idv[k] = int64_t(id) < dn ? id : 0u;
            }
            const uintptr_t da = reinterpret_cast<uintptr_t>(ck.dict_data);
            if (dl) {
                #pragma unroll
                for (int k = 0; k < NEPT; k++) v[k] = reinterpret_cast<const VT*>(DL)[idv[k]];
            } else if ((da & uintptr_t(w - 1)) == 0) {   // (dictionary pages start 16-byte aligned in scratch)
                const PF_GLOBAL VT* g = (const PF_GLOBAL VT*)ck.dict_data;
                #pragma unroll
                for (int k = 0; k < NEPT; k++) v[k] = g[idv[k]];
            } else {
                #pragma unroll
                for (int k = 0; k < NEPT; k++) {
                    const uint8_t* src = ck.dict_data + uint64_t(idv[k]) * uint64_t(w);
                    if constexpr (W == 4) v[k] = ld_u32_any(src); else v[k] = ld_u64_any(src);
                }
            }
        } else {
            // value of entry k: gv0 + present entries before k (absent entries load their successor's,
            // clamped to the thread's last present value)
            const uint32_t last = gv0 + uint32_t(__popc(fv)) - 1u;
            uint32_t vi[NEPT];
            #pragma unroll
            for (int k = 0; k < NEPT; k++) vi[k] = min(gv0 + uint32_t(__popc(fv & ((1u << k) - 1u))), last);
            if ((reinterpret_cast<uintptr_t>(s.val) & uintptr_t(w - 1)) == 0) {
                const PF_GLOBAL VT* g = (const PF_GLOBAL VT*)s.val;
                #pragma unroll
                for (int k = 0; k < NEPT; k++) v[k] = g[vi[k]];
            } else {
                #pragma unroll
                for (int k = 0; k < NEPT; k++) {
                    const uint8_t* src = s.val + uint64_t(vi[k]) * uint64_t(w);
                    if constexpr (W == 4) v[k] = ld_u32_any(src); else v[k] = ld_u64_any(src);
                }
            }
        }
        #pragma unroll
        for (int k = 0; k < NEPT; k++)
            if (!((fv >> k) & 1u)) v[k] = 0;
    }
    const uint64_t slot_base = uint64_t(pg.entry_start);
    if (m && !bad) {
        uint8_t* dst0 = ck.values + (slot_base + e) * uint64_t(w);
        if (m == NEPT && (reinterpret_cast<uintptr_t>(dst0) & 15u) == 0) {
            u32x4* d4 = reinterpret_cast<u32x4*>(dst0);
            if constexpr (W == 4) {
                #pragma unroll
                for (int q = 0; q < NEPT / 4; q++) d4[q] = u32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
            } else {
                #pragma unroll
                for (int q = 0; q < NEPT / 2; q++)
                    d4[q] = u32x4{uint32_t(v[2 * q]), uint32_t(v[2 * q] >> 32), uint32_t(v[2 * q + 1]), uint32_t(v[2 * q + 1] >> 32)};
            }
        } else {
            for (uint32_t k = 0; k < m; k++) {
                uint32_t* d = reinterpret_cast<uint32_t*>(dst0 + uint64_t(k) * uint64_t(w));   // 4-byte aligned
                d[0] = uint32_t(v[k]);
                if constexpr (W == 8) d[1] = uint32_t(uint64_t(v[k]) >> 32);
            }
        }
    }
    if (ck.validity && fv) {
        const uint64_t abase = (slot_base + e_begin) & ~uint64_t(31);
        const uint64_t rb = slot_base + e - abase;
        const uint32_t sh = uint32_t(rb & 31);
        atomicOr(&S.vbits[rb >> 5], fv << sh);
        if (sh + NEPT > 32 && sh) atomicOr(&S.vbits[(rb >> 5) + 1], fv >> (32 - sh));
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi);
        return;
    }
    if (ck.validity) flush_bits(S.vbits, slot_base + e_begin, e_end - e_begin, ck.validity);
    if (tid == 0) {
        if (ck.needs_count == 0) atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values), (unsigned long long)tv);
        atomicOr(&pg.done, DONE_NULL);
    }
#ifdef PF_STAMPS
    NSTAMP(4);
    if (tid == 0) { PSTAMP(0, 1); PSTAMP(5, t_ph - t_beg); }
#endif
#undef NSTAMP
}

#ifdef PF_DIAG   // diagnostics build only (VERDICT r05 hygiene)
// k_page_null: one 512-thread workgroup per nullable flat page (fixed width 4 / 8, dictionary or
// PLAIN), for pages whose level section (<= LVL_STAGE bytes), level runs (<= PN_RUNS) and
// dictionary-id bytes (<= PN_IST) fit its LDS. It runs before k_lvl in the levels stage and does
// k_lvl's and k_flat_null's work for the page in one launch: the level and id sections are staged
// once, the level run headers are found by the all-positions chain (every byte decoded as a
// header, the chain from 0 followed in LDS), decoded in parallel and prefix-summed, and the page's
// 4096-entry blocks are then decoded in a loop (8 consecutive entries per thread, present bits ->
// block scan -> value index -> id from LDS -> gathers issued together -> 16-byte stores). The
// page's metadata chain, its section staging and the level parse are paid once per page instead of
// once per block, and k_lvl's one-wave block-table pass is gone. Anything it cannot decode
// exactly (a broken chain, an id past the dictionary, too many runs) leaves the page unmarked:
// k_lvl / k_flat_null / k_decode then take it and report it as before.
constexpr int PN_NT = 512;
constexpr uint32_t PN_RUNS = 512;        // level runs held in LDS
constexpr uint32_t PN_IST = 32768;       // dictionary-id bytes staged in LDS
constexpr uint32_t PN_MAX_BLOCKS = 16;   // entries <= 16 * FBLK
constexpr int PN_NEPT = FBLK / PN_NT;    // 8 consecutive entries per thread
struct PageNullLds {
    uint32_t lv[(LVL_STAGE + 64) / 4];
    uint16_t nxt[LVL_STAGE];
    Run drun[PN_RUNS];
    Run vrun[RUN_CAP];
    uint32_t ist[PN_IST / 4 + 8];
    uint32_t vbits[FBLK / 32 + 2];
    uint32_t scan_tmp[PN_NT / 64];
    uint32_t nh, ok, take;
};
__global__ __launch_bounds__(PN_NT) void k_page_null(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                    const int* __restrict__ list, DevChunkResult* res) {
    __shared__ __attribute__((aligned(16))) PageNullLds S;
    const int pi = list[blockIdx.x];
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    const IdRunTab* T = pg.runtab;
    Sections s;
    const int w = ck.width;
    const bool dict = is_dict_enc(pg.encoding);
    const uint32_t ne = uint32_t(pg.num_values);
    // (uniform: every thread evaluates the same loads)
    bool take = pg.lvltab != nullptr && res[pg.chunk].status == 0 && ck.max_rep == 0 && ck.max_def > 0 &&
                (w == 4 || w == 8) && ck.values != nullptr && !(pg.done & (DONE_FIXED | DONE_NULL)) &&
                (dict || pg.encoding == 0) && ne > 0 && ne <= PN_MAX_BLOCKS * FBLK && page_sections(pg, ck, s) &&
                s.def_rle && s.def_n > 0 && s.def_n <= LVL_STAGE;
    uint32_t id_bw = 0, idn = 0, vnr = 0, idcov = 0;
    if (take && dict) {
        take = T != nullptr && T->valid == 1u && T->nruns <= uint32_t(RUN_CAP) && T->nruns > 0 && s.val_n > 1 && s.val[0] <= 32 &&
               s.val_n - 1 <= PN_IST && ck.dict_data != nullptr && ck.dict_n > 0;
        if (take) { id_bw = s.val[0]; idn = uint32_t(s.val_n - 1); vnr = T->nruns; idcov = T->covered; }
    }
    if (!take) return;
    const int bw = bit_width(uint32_t(ck.max_def));
    const uint32_t maxd = uint32_t(ck.max_def);
    const uint32_t dn = uint32_t(s.def_n);
    // ---- stage: level bytes, id bytes, id runs (one round of loads)
    const uint32_t doff = stage_bytes(S.lv, s.def, dn, 0, dn);
    const uint32_t ioff = dict ? stage_bytes(S.ist, s.val + 1, idn, 0, idn) : 0u;
    for (uint32_t i = tid; i < vnr; i += PN_NT) S.vrun[i] = id_run(T, i, vnr, idcov);
    __syncthreads();
    const uint8_t* lv8 = reinterpret_cast<const uint8_t*>(S.lv);
    const uint8_t* stw = lv8 + doff;   // stw[i] = level section byte i (zero past the section)
    // ---- level run headers: every byte position as a header (position of the next one)
    for (uint32_t p = tid; p < dn; p += PN_NT) {
        uint32_t h = 0, hl = 0, nx = 0xffffu;
        #pragma unroll
        for (uint32_t k = 0; k < 3; k++) {   // (a header of > 3 bytes counts > 2^20 entries: no run here)
            const uint32_t c = p + k < dn ? uint32_t(stw[p + k]) : 0x80u;
            h |= (c & 0x7fu) << (7 * k);
            if (!(c & 0x80u)) { hl = k + 1; break; }
        }
        if (hl) {
            const uint32_t pay = (h & 1u) ? (h >> 1) * uint32_t(bw) : (uint32_t(bw) + 7u) >> 3;
            if (p + hl + pay <= dn) nx = p + hl + pay;
        }
        S.nxt[p] = uint16_t(nx);
    }
    __syncthreads();
    if (tid == 0) {   // the chain from position 0 (one LDS load per run)
        uint32_t p = 0, nh = 0;
        bool ok = true;
        while (p < dn) {
            if (nh == PN_RUNS) { ok = false; break; }
            S.drun[nh++].data = p;   // header position (decoded below)
            const uint32_t q = S.nxt[p];
            if (q == 0xffffu) { ok = false; break; }   // no valid run at p
            p = q;
        }
        S.nh = nh;
        S.ok = ok ? 1u : 0u;
    }
    __syncthreads();
    if (!S.ok) return;   // k_lvl / k_decode take the page (and report what is wrong with it)
    const uint32_t nh = S.nh;
    {   // decode the headers in parallel; first entries by a block scan of the counts
        uint32_t cnt = 0, data = 0, packed = 0;
        bool bad = false;
        const uint32_t k = uint32_t(tid);
        if (k < nh) {
            const uint32_t P = S.drun[k].data;
            uint32_t h = 0, hl = 0;
            for (uint32_t b = 0; b < 3; b++) {
                const uint32_t c = stw[P + b];
                h |= (c & 0x7fu) << (7 * b);
                if (!(c & 0x80u)) { hl = b + 1; break; }
            }
            packed = h & 1u;
            cnt = packed ? (h >> 1) * 8u : (h >> 1);
            if (packed) data = (doff + P + hl) * 8u;   // LDS bit offset of the run's first level
            else {
                for (uint32_t b = 0; b < ((uint32_t(bw) + 7u) >> 3); b++) data |= uint32_t(stw[P + hl + b]) << (8 * b);
                bad = data > maxd;
            }
        }
        uint32_t tot;
        const uint32_t first = block_excl_scan<PN_NT>(cnt, S.scan_tmp, tot);
        if (k < nh) {
            Run r;
            r.first = first;
            r.count = cnt;
            r.data = data;
            r.packed = packed;
            S.drun[k] = r;
        }
        if (__syncthreads_or(bad || (tid == 0 && tot < ne))) return;
    }
    // ---- the page's blocks
    const uint64_t slot_base = uint64_t(pg.entry_start);
    const uint8_t* ist8 = reinterpret_cast<const uint8_t*>(S.ist);
    const uint32_t ilim = (ioff + idn) * 8u;   // staged id bits
    const uint32_t nblk = (ne + FBLK - 1) / FBLK;
    const uintptr_t da = reinterpret_cast<uintptr_t>(dict ? ck.dict_data : s.val);
    const bool galign = (da & uintptr_t(w - 1)) == 0;
    const int64_t dnn = dict ? ck.dict_n : 0;
    uint32_t vbase = 0;   // page-relative index of the block's first present value
    for (uint32_t b = 0; b < nblk; b++) {
        const uint32_t e_begin = b * FBLK, e_end = min(ne, e_begin + FBLK);
        for (uint32_t i = tid; i < FBLK / 32 + 2; i += PN_NT) S.vbits[i] = 0;
        const uint32_t e = e_begin + uint32_t(tid) * PN_NEPT;
        const uint32_t m = e < e_end ? min(uint32_t(PN_NEPT), e_end - e) : 0u;
        uint32_t fv = 0;
        int bad = 0;
        if (m) {
            int r = run_find(S.drun, int(nh), e);
            const Run R = S.drun[r];
            if (e + m <= R.first + R.count && (!R.packed || bw == 1)) {   // one run
                if (!R.packed) fv = R.data == maxd ? ((1u << m) - 1u) : 0u;
                else fv = lds_bits(lv8, R.data + (e - R.first), m);
            } else {
                for (uint32_t k = 0; k < m; k++) {
                    while (r + 1 < int(nh) && e + k >= S.drun[r].first + S.drun[r].count) r++;
                    const Run& Rk = S.drun[r];
                    uint32_t dl = Rk.data;
                    if (Rk.packed) dl = lds_bits(lv8, Rk.data + (e + k - Rk.first) * uint32_t(bw), uint32_t(bw));
                    bad |= dl > maxd;
                    fv |= uint32_t(dl == maxd) << k;
                }
            }
        }
        uint32_t tv;
        const uint32_t vo = block_excl_scan<PN_NT>(__popc(fv), S.scan_tmp, tv);
        const uint32_t gv0 = vbase + vo;
        uint32_t idv[PN_NEPT];
        #pragma unroll
        for (int k = 0; k < PN_NEPT; k++) idv[k] = 0;
        if (fv) {
            if (dict) {
                if (gv0 + uint32_t(__popc(fv)) > idcov) bad = 1;
                int vr = run_find(S.vrun, int(vnr), gv0);
                uint32_t j = 0;
                #pragma unroll
                for (int k = 0; k < PN_NEPT; k++) {
                    if (!((fv >> k) & 1u)) continue;
                    const uint32_t gv = gv0 + j++;
                    while (vr + 1 < int(vnr) && gv >= S.vrun[vr].first + S.vrun[vr].count) vr++;
                    const Run& V = S.vrun[vr];
                    uint32_t id = V.data;
                    if (V.packed) {
                        const uint64_t bb = uint64_t(V.data) + uint64_t(ioff) * 8u + uint64_t(gv - V.first) * id_bw;
                        bad |= bb + id_bw > ilim;
                        id = bb + id_bw <= ilim ? lds_bits(ist8, uint32_t(bb), id_bw) : 0u;
                    }
                    bad |= int64_t(id) >= dnn;
                    idv[k] = int64_t(id) < dnn ? id : 0u;
                }
            } else {
                const uint32_t last = gv0 + uint32_t(__popc(fv)) - 1u;
                if (uint64_t(last + 1) * uint64_t(w) > s.val_n) bad = 1;
                #pragma unroll
                for (int k = 0; k < PN_NEPT; k++) idv[k] = bad ? 0u : min(gv0 + uint32_t(__popc(fv & ((1u << k) - 1u))), last);
            }
        }
        if (__syncthreads_or(bad)) return;   // (nothing counted or marked: the fallback redoes the page)
        uint64_t v[PN_NEPT];
        #pragma unroll
        for (int k = 0; k < PN_NEPT; k++) v[k] = 0;
        if (!fv) {
        } else if (galign) {
            if (w == 4) {
                const PF_GLOBAL uint32_t* g = (const PF_GLOBAL uint32_t*)da;
                #pragma unroll
                for (int k = 0; k < PN_NEPT; k++) v[k] = g[idv[k]];
            } else {
                const PF_GLOBAL uint64_t* g = (const PF_GLOBAL uint64_t*)da;
                #pragma unroll
                for (int k = 0; k < PN_NEPT; k++) v[k] = g[idv[k]];
            }
        } else {
            #pragma unroll
            for (int k = 0; k < PN_NEPT; k++) {
                const uint8_t* src = reinterpret_cast<const uint8_t*>(da) + uint64_t(idv[k]) * uint64_t(w);
                v[k] = w == 4 ? uint64_t(ld_u32_any(src)) : ld_u64_any(src);
            }
        }
        #pragma unroll
        for (int k = 0; k < PN_NEPT; k++)
            if (!((fv >> k) & 1u)) v[k] = 0;
        if (m) {
            uint8_t* dst0 = ck.values + (slot_base + e) * uint64_t(w);
            if (m == PN_NEPT && (reinterpret_cast<uintptr_t>(dst0) & 15u) == 0) {
                u32x4* d4 = reinterpret_cast<u32x4*>(dst0);
                if (w == 4) {
                    d4[0] = u32x4{uint32_t(v[0]), uint32_t(v[1]), uint32_t(v[2]), uint32_t(v[3])};
                    d4[1] = u32x4{uint32_t(v[4]), uint32_t(v[5]), uint32_t(v[6]), uint32_t(v[7])};
                } else {
                    #pragma unroll
                    for (int q = 0; q < 4; q++)
                        d4[q] = u32x4{uint32_t(v[2 * q]), uint32_t(v[2 * q] >> 32), uint32_t(v[2 * q + 1]), uint32_t(v[2 * q + 1] >> 32)};
                }
            } else {
                for (uint32_t k = 0; k < m; k++) {
                    uint32_t* d = reinterpret_cast<uint32_t*>(dst0 + uint64_t(k) * uint64_t(w));   // 4-byte aligned
                    d[0] = uint32_t(v[k]);
                    if (w == 8) d[1] = uint32_t(v[k] >> 32);
                }
            }
        }
        if (ck.validity && fv) {
            const uint64_t abase = (slot_base + e_begin) & ~uint64_t(31);
            const uint64_t rb = slot_base + e - abase;
            const uint32_t sh = uint32_t(rb & 31);
            atomicOr(&S.vbits[rb >> 5], fv << sh);
            if (sh + PN_NEPT > 32 && sh) atomicOr(&S.vbits[(rb >> 5) + 1], fv >> (32 - sh));
        }
        __syncthreads();
        if (ck.validity) flush_bits(S.vbits, slot_base + e_begin, e_end - e_begin, ck.validity);
        vbase += tv;
        __syncthreads();   // (vbits / scan_tmp reused by the next block)
    }
    if (tid == 0) {
        if (ck.needs_count == 0) atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values), (unsigned long long)vbase);
        atomicOr(&pg.done, DONE_NULL | DONE_PAGE);
    }
}

// Diagnostics (tests/test_gpu_runs.py): walk_runs (one lane) and wave_walk_runs (one wave) over the
// same stream; out = {ret, nruns, covered, pos, first, runs[cap] x 4} for each.
// walk_runs is the reference: the run walk's contract (RunWalk, pf_pages.h) header by header.
__device__ int walk_runs(const uint8_t* p, uint64_t n, int bw, uint32_t lo, uint32_t limit, Run* runs, int cap,
                         int& nruns, uint32_t& covered, RunWalk& st) {
    nruns = 0;
    covered = st.first;
    while (st.first < limit) {
        uint64_t pos = st.pos, h;
        if (!uvarint(p, n, pos, h)) return 1;
        Run r;
        uint64_t cnt;
        if (h & 1) {
            cnt = (h >> 1) * 8;
            const uint64_t nb = (h >> 1) * uint64_t(bw);
            r.data = uint32_t(pos * 8);
            r.packed = 1;
            pos += nb < n - pos ? nb : n - pos;   // truncated to what is left (zero-padded)
        } else {
            cnt = h >> 1;
            const int nbv = (bw + 7) >> 3;
            if (pos + nbv > n) return 1;
            uint32_t v = 0;
            for (int b = 0; b < nbv; b++) v |= uint32_t(p[pos + b]) << (8 * b);
            pos += nbv;
            r.data = v;
            r.packed = 0;
        }
        if (cnt == 0) { st.pos = pos; continue; }
        const uint32_t c = uint32_t(cnt < uint64_t(limit - st.first) ? cnt : uint64_t(limit - st.first));
        if (st.first + c > lo) {
            if (nruns == cap) return 2;
            r.first = st.first;
            r.count = c;
            runs[nruns++] = r;
            covered = st.first + c;
        } else {
            covered = st.first + c;
        }
        st.pos = pos;
        st.first += c;
    }
    return 0;
}

__global__ __launch_bounds__(64) void k_debug_walk(const uint8_t* p, uint64_t n, int bw, uint32_t lo, uint32_t limit, int cap,
                                                    uint32_t pos0, uint32_t first0, uint32_t* out) {
    __shared__ Run R[RUN_CAP];
    __shared__ int s_nr;
    __shared__ uint32_t s_cov;
    __shared__ RunWalk s_st;
    const int tid = threadIdx.x;
    uint32_t* o1 = out;
    uint32_t* o2 = out + 5 + 4 * cap;
    if (tid == 0) {
        RunWalk st{pos0, first0};
        int nr = 0;
        uint32_t cov = 0;
        const int r = walk_runs(p, n, bw, lo, limit, R, cap, nr, cov, st);
        o1[0] = uint32_t(r); o1[1] = uint32_t(nr); o1[2] = cov; o1[3] = uint32_t(st.pos); o1[4] = st.first;
        for (int i = 0; i < nr; i++) { o1[5 + 4 * i] = R[i].first; o1[6 + 4 * i] = R[i].count; o1[7 + 4 * i] = R[i].data; o1[8 + 4 * i] = R[i].packed; }
        s_st = RunWalk{pos0, first0};
    }
    __syncthreads();
    const int r = wave_walk_runs(p, n, bw, lo, limit, R, cap, s_nr, s_cov, s_st, RunWalk{pos0, first0});
    __syncthreads();
    if (tid == 0) {
        o2[0] = uint32_t(r); o2[1] = uint32_t(s_nr); o2[2] = s_cov; o2[3] = uint32_t(s_st.pos); o2[4] = s_st.first;
    }
    for (int i = tid; i < s_nr; i += 64) { o2[5 + 4 * i] = R[i].first; o2[6 + 4 * i] = R[i].count; o2[7 + 4 * i] = R[i].data; o2[8 + 4 * i] = R[i].packed; }
}

extern "C" int pf_debug_walk_runs(const uint8_t* stream, uint64_t n, int bw, uint32_t lo, uint32_t limit, int cap,
                                  uint32_t pos0, uint32_t first0, uint32_t* out) {
    if (cap > int(RUN_CAP) || cap < 0) return -1;
    uint8_t* d = nullptr;
    uint32_t* o = nullptr;
    const size_t ob = 4 * size_t(2 * (5 + 4 * cap));
    if (hipMalloc(&d, n + 64) != hipSuccess) return -1;
    if (hipMalloc(&o, ob) != hipSuccess) { (void)hipFree(d); return -1; }
    int rc = 0;
    if (hipMemset(d, 0, n + 64) != hipSuccess || hipMemcpy(d, stream, n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(o, 0, ob) != hipSuccess)
        rc = -1;
    if (!rc) {
        hipLaunchKernelGGL(k_debug_walk, dim3(1), dim3(64), 0, 0, d, n, bw, lo, limit, cap, pos0, first0, o);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, o, ob, hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    }
    (void)hipFree(d);
    (void)hipFree(o);
    return rc;
}
#endif  // PF_DIAG

// ---- launchers -------------------------------------------------------------------------------
// The flat half of the count stage; launch_count (pf_decode.hip) follows it on the stream.
void launch_count_flat(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, int n_flat, const int2* d_dblk,
                       int n_dblk, DevChunkResult* d_res, BaJob* d_bajobs, hipStream_t st) {
    // d_list: the count list of n pages, whose first n_flat are the flat BYTE_ARRAY pages (k_count_flat's
    // grid; none: no launch). d_dblk: (page, block) pairs of the flat dictionary BYTE_ARRAY pages
    // (k_count_dict, before k_count_flat)
    if (n <= 0) return;
    if (n_dblk > 0) hipLaunchKernelGGL(k_count_dict, dim3(n_dblk), dim3(NT), 0, st, d_chunks, d_pages, d_dblk, d_res);
    if (n_flat > 0) hipLaunchKernelGGL(k_count_flat, dim3(n_flat), dim3(NT), 0, st, d_chunks, d_pages, d_list, d_res, d_bajobs);
}
void launch_runs(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res,
                 hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_runs, dim3(n), dim3(128), 0, st, d_chunks, d_pages, d_list, d_res);
}
void launch_lvl(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res,
                hipStream_t st, bool page_null, NullCaps nc) {
    if (n <= 0) return;
    // page_null (diagnostics option): k_page_null first (one 512-thread workgroup and ~57 KiB of LDS per
    // page; under the bench's four streams its workgroups wait for whole CUs: config 4 5.57 ms with it, 4.47 without)
#ifdef PF_DIAG
    if (page_null) hipLaunchKernelGGL(k_page_null, dim3(n), dim3(PN_NT), 0, st, d_chunks, d_pages, d_list, d_res);
#else
    (void)page_null;
#endif
    hipLaunchKernelGGL(k_lvl, dim3(n), dim3(LT_NT), 0, st, d_chunks, d_pages, d_list, d_res, nc.dcap, nc.icap);
}
void launch_flat(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int nfix, int n, int n4, int n8, int* d_fbq,
                 const int2* d_dblk, int n_dblk, DevChunkResult* d_res, hipStream_t st, NullCaps nc, int stagger) {
    // d_list: nfix (page, block) pairs of flat fixed-width pages (k_flat_fixed), then n of every other
    // flat page (k_flat_all), then n4 / n8 of nullable 4 / 8-byte pages (k_flat_null<4> / <8>; they mark
    // their pages DONE_NULL). Blocks k_flat_null and k_flat_fixed do not take are queued in d_fbq for
    // k_flat_all's last workgroups. nc: k_flat_null's LDS stages (dictionary: nc.dlds bytes); stagger (diagnostics build,
    // tests): k_flat_null's blocks > 0 of a page wait that many sleep rounds (~3 us each) for block 0
    const int2* blocks = reinterpret_cast<const int2*>(d_list);
    const size_t dyn = size_t(nc.dcap) + 32u + nc.icap + 32u + nc.dlds;
    if (n4 > 0)
        hipLaunchKernelGGL(k_flat_null<4>, dim3(n4), dim3(NTN), dyn, st, d_chunks, d_pages, blocks + nfix + n, d_res, nc, stagger, d_fbq);
    if (n8 > 0)
        hipLaunchKernelGGL(k_flat_null<8>, dim3(n8), dim3(NTN), dyn, st, d_chunks, d_pages, blocks + nfix + n + n4, d_res, nc, stagger,
                           d_fbq);
    if (nfix > 0) hipLaunchKernelGGL(k_flat_fixed, dim3(nfix), dim3(NT), 0, st, d_chunks, d_pages, blocks, d_res, d_fbq);
    // d_dblk: k_count_dict's (page, block) pairs, the blocks of flat dictionary BYTE_ARRAY pages: k_flat_dstr takes
    // the pages with a small dictionary of short values, k_flat_all's blocks of those then return at once
    if (n_dblk > 0) hipLaunchKernelGGL(k_flat_dstr, dim3(n_dblk), dim3(NT), 0, st, d_chunks, d_pages, d_dblk, d_res);
    // k_flat_all last, with min(nq, 32) more workgroups for the fallback queue (nearly always empty; each
    // needs a CU with room for a k_flat_all workgroup: a grid of min(nq, 1024) waited ~0.1 ms under load,
    // and a launch of its own added one more wait per batch)
    const int nq = nfix + n4 + n8;
    const int nqw = nq < 32 ? nq : 32;
    if (n + nqw > 0)
        hipLaunchKernelGGL(k_flat_all, dim3(n + nqw), dim3(NT), 0, st, d_chunks, d_pages, blocks + nfix, n, d_fbq, d_res);
}

}  // namespace pf
