// pf_flat_ids.hip — the kernels of a kept-dictionary chunk (pf_decode_row_group_dict): its data pages
// become indices into the dictionary instead of values, and the dictionary itself is laid out as an output array.
//   k_flat_ids      per (page, block) of the planner's L_IDS list: FBLK entries -> index_width-byte indices + validity
//   k_dict_offsets  per kept BYTE_ARRAY chunk: the dictionary's offsets (a scan of the lengths the dictionary walk
//                   left in dict_len) and its room in the chars arena
//   k_dict_pack     per kept chunk: the dictionary's chars, or the bytes of a fixed-width dictionary
// launch_flat_ids puts them at the end of the flat stage. The id unpack is pf_dstr_ids.h (dstr_ids16), shared with
// k_flat_dstr and checked on the host by tests/native/pf_dstr_ids_check.cpp; no existing kernel's text is touched:
// a kept chunk's pages are on none of the lists the expanding kernels read.
#include <hip/hip_runtime.h>

#include "pf_dstr_ids.h"
#include "pf_flat.h"
#include "pf_launch.h"

namespace pf {

#ifdef PF_DIAG   // diagnostics build: blocks the fast path decoded, pages the slow path decoded (tests)
__device__ unsigned long long pf_ids_counts[2];
extern "C" int pf_debug_ids_counts(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pf_ids_counts), sizeof(unsigned long long) * 2) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pf_ids_counts), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#define IDS_COUNT(i) (threadIdx.x == 0 ? (void)atomicAdd(&pf_ids_counts[i], 1ull) : (void)0)
#else
#define IDS_COUNT(i) ((void)0)
#endif

constexpr uint32_t IDS_WIN = 16384;   // bytes of the LDS window: first the block's id bytes, then its indices
static_assert(IDS_WIN >= 4 * FBLK && RUN_CAP <= NT && FBLK == 16u * NT, "one run and 16 entries per thread; a block's indices fit the window");

// Fast path: everything a block needs in LDS.
struct IdsFast {
    uint32_t rt[2 * RUN_CAP];             // k_runs' rows
    u32x4 win[IDS_WIN / 16 + 2];
    LvlRun lruns[LT_BLOCK_RUNS];          // the level runs the block overlaps (k_lvl)
    uint32_t vbits[FBLK / 32 + 2];        // validity bits of the block's slots, from the 32-slot boundary at or before them
    uint32_t scan_tmp[NT / 64];
    uint32_t wlo[NT / 64], whi[NT / 64];  // id byte range of the block's packed runs, per wave
};
// Slow path: the tile-wise walk of the hybrid streams, as k_decode does it.
struct IdsSlow {
    LevelLds L;
    Piece pval[TILE];
    uint32_t ids[TILE];
    uint32_t vbits[TILE / 32 + 2];
    uint32_t scan_tmp[NT / 64];
    RleState sval;
    int npval, verr;
};
union IdsLds {
    IdsFast f;
    IdsSlow s;
};

// One index of `iw` bytes at element i of an iw-aligned array.
__device__ __forceinline__ void put_index(uint8_t* base, uint64_t i, uint32_t iw, uint32_t v) {
    if (iw == 1) base[i] = uint8_t(v);
    else if (iw == 2) reinterpret_cast<uint16_t*>(base)[i] = uint16_t(v);
    else reinterpret_cast<uint32_t*>(base)[i] = v;
}

// A whole page by one workgroup, tile after tile, from the streams themselves: pages whose run tables the fast path
// cannot use (no valid id run table, more than RUN_CAP runs, level tables that do not fit or were not made). Element
// stores only, so a word shared with a neighbouring page is never read; validity bits through flush_bits.
__device__ __forceinline__ void ids_slow_page(IdsSlow& S, const DevChunk& ck, DevPage& pg, const int pi, DevChunkResult* res,
                                              const Sections& s, const bool sec_ok, const uint32_t iw, const uint64_t dn) {
    LevelLds& L = S.L;
    const int tid = threadIdx.x;
    if (tid == 0) {
        rle_init(L.srep);
        rle_init(L.sdef);
        rle_init(S.sval);
        S.sval.pos = 1;   // (behind the id width byte)
        L.err = sec_ok ? 0 : 1;
        S.verr = 0;
    }
    __syncthreads();
    const int id_bw = s.val_n > 0 ? int(s.val[0]) : 0;
    if (L.err || !is_dict_enc(pg.encoding) || id_bw > 32) {
        if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi);
        return;
    }
    uint64_t slot_base = uint64_t(pg.entry_start);
    uint64_t vidx = 0;
    const uint64_t e_e = uint64_t(pg.num_values);
    for (uint64_t e0 = 0; e0 < e_e; e0 += TILE) {
        const uint32_t want = uint32_t(min<uint64_t>(TILE, e_e - e0));
        decode_level_tile(L, s, ck, e0, want);
        if (L.err) break;
        const uint32_t eb = uint32_t(tid) * EPT;
        uint32_t fv = 0;
        #pragma unroll
        for (int k = 0; k < EPT; k++)
            if (eb + k < want) fv |= uint32_t(L.def[eb + k] == ck.max_def) << k;
        uint32_t tv;
        const uint32_t vo = block_excl_scan<NT>(__popc(fv), S.scan_tmp, tv);
        if (tv > 0) {
            if (tid == 0) {
                const uint32_t got = rle_walk(S.sval, s.val, s.val_n, id_bw, tv, S.pval, TILE, S.npval);
                if (got != tv || S.sval.err) S.verr = 1;
            }
            __syncthreads();
            if (S.verr) break;
            rle_expand<uint32_t>(S.pval, S.npval, s.val, s.val_n, id_bw, S.ids);
        }
        for (uint32_t i = tid; i < TILE / 32 + 2; i += NT) S.vbits[i] = 0;
        __syncthreads();
        {
            uint32_t vv = vo;
            #pragma unroll
            for (int k = 0; k < EPT; k++) {
                const uint32_t e = eb + k;
                if (e >= want) break;
                const uint64_t slot = slot_base + e;
                uint32_t idx = 0;
                if ((fv >> k) & 1u) {
                    idx = S.ids[vv++];
                    if (uint64_t(idx) >= dn) { S.verr = 1; idx = 0; }
                    const uint64_t rb = slot - (slot_base & ~uint64_t(31));
                    atomicOr(&S.vbits[rb >> 5], 1u << (rb & 31));
                }
                put_index(ck.values, slot, iw, idx);
            }
        }
        __syncthreads();
        if (S.verr) break;
        if (ck.max_def > 0 && ck.validity) flush_bits(S.vbits, slot_base, want, ck.validity);
        slot_base += want;
        vidx += tv;
        __syncthreads();
    }
    if (L.err || S.verr) {
        if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi);
        return;
    }
    if (tid == 0) atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values), (unsigned long long)vidx);
}

// ---- k_flat_ids: one FBLK block of a kept chunk's data page per workgroup, 16 consecutive entries per thread --------
// The page's id run table (k_runs) and, for a page with nulls, the level runs its block overlaps (k_lvl) are staged in
// LDS with the block's id bytes; a thread's present mask gives, after one block scan, the value index of its first
// present entry; dstr_ids16 unpacks the ids of its present values, which are then spread over its 16 entries (null
// slots get 0). Every id of a present value is checked against the dictionary's size. The indices are packed in the
// LDS window and leave as aligned 16-byte stores; the block's first and last chunk, which it may share with the
// neighbouring page's workgroup, are stored bytewise, its own bytes only. Validity words at the block's edges are
// or-ed into (flush_bits, fill_valid_ones). The choice between this path and the slow one depends on the page's
// tables only, so all blocks of a page decide alike; the slow path decodes the whole page in its block 0.
__global__ __launch_bounds__(NT) void k_flat_ids(const DevChunk* __restrict__ chunks, DevPage* pages, const int2* __restrict__ blocks,
                                                 DevChunkResult* res, const DevKeep* __restrict__ keeps,
                                                 const int* __restrict__ keep_of) {
    __shared__ IdsLds U;
    const int2 pb = blocks[blockIdx.x];
    const int pi = pb.x;
    const uint32_t blk = uint32_t(pb.y);
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    if (res[pg.chunk].status != 0) return;
    const int kx = keep_of[pg.chunk];
    if (kx < 0 || !ck.values || pg.num_values < 0) return;
    const uint32_t iw = uint32_t(keeps[kx].index_width);
    const uint64_t dn = uint64_t(ck.dict_n > 0 ? ck.dict_n : 0);
    const uint32_t ne = uint32_t(pg.num_values);
    const uint32_t b0 = blk * FBLK;
    if (blk > 0 && b0 >= ne) return;
    Sections s;
    const bool sec_ok = page_sections(pg, ck, s);
    const IdRunTab* T = pg.runtab;
    const LvlHead* LT = pg.lvltab;
    // ---- fast or slow (block-uniform, and the same for every block of the page)
    bool fast = sec_ok && is_dict_enc(pg.encoding) && ne > 0 && s.val_n > 0 && s.val[0] <= 32 && T != nullptr && T->valid == 1u &&
                T->nruns <= uint32_t(RUN_CAP);
    bool allp = false;
    if (fast) {
        allp = ck.max_def == 0 || T->all_present == 1u;
        if (!allp) fast = LT != nullptr && LT->fit == 1u && LT->nruns <= pg.lvl_cap && s.def_rle != 0;
    }
    if (!fast) {
        if (blk == 0) {
            ids_slow_page(U.s, ck, pg, pi, res, s, sec_ok, iw, dn);
            IDS_COUNT(1);
        }
        return;
    }
    IdsFast& S = U.f;
    const uint32_t b1 = min(ne, b0 + FBLK);
    const uint32_t nr = T->nruns, cov = T->covered;
    const int id_bw = int(s.val[0]);
    const uint8_t* ids = s.val + 1;
    const uint64_t ids_n = s.val_n - 1;
    const uint32_t e0 = b0 + 16u * uint32_t(tid);
    const uint32_t n = e0 < b1 ? min(16u, b1 - e0) : 0u;
    const uint32_t nmask = n >= 16u ? 0xffffu : ((1u << n) - 1u);
    const uint64_t slot0 = uint64_t(pg.entry_start) + b0, slot1 = uint64_t(pg.entry_start) + b1;
    int bad = 0;
    // ---- present mask of the thread's entries, values before the block
    uint32_t pm = nmask, vb = b0;
    if (!allp) {
        const LvlBlock LB = *lvl_block(const_cast<LvlHead*>(LT), pg.lvl_cap, blk);
        const uint32_t nlr = LB.r1 > LB.r0 ? LB.r1 - LB.r0 : 0u;
        const int bw = bit_width(uint32_t(ck.max_def));
        const uint32_t maxd = uint32_t(ck.max_def);
        vb = LB.vb;
        if (nlr == 0 || nlr > LT_BLOCK_RUNS || LB.r1 > LT->nruns) bad = 1;
        else {
            const LvlRun* G = lvl_runs(const_cast<LvlHead*>(LT));
            for (uint32_t i = tid; i < nlr; i += NT) S.lruns[i] = G[LB.r0 + i];
        }
        for (uint32_t i = tid; i < FBLK / 32 + 2; i += NT) S.vbits[i] = 0;
        if (__syncthreads_or(bad)) {
            if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi);
            return;
        }
        pm = 0;
        if (n > 0) {
            uint32_t r = last_row_le(nlr, e0, [&](uint32_t i) { return S.lruns[i].first; });
            const LvlRun R0 = S.lruns[r];
            if (e0 >= R0.first && e0 + n <= R0.first + R0.count() && (!R0.packed() || bw == 1)) {   // one run holds all 16
                if (!R0.packed()) {
                    if (R0.data > maxd) bad = 1;
                    pm = R0.data == maxd ? nmask : 0u;
                } else {
                    pm = bits_le(s.def, s.def_n, uint64_t(R0.data) + uint64_t(e0 - R0.first), 16) & nmask;
                }
            } else {
                for (uint32_t k = 0; k < n; k++) {
                    const uint32_t e = e0 + k;
                    while (r + 1 < nlr && e >= S.lruns[r + 1].first) r++;
                    const LvlRun R = S.lruns[r];
                    if (e < R.first || e >= R.first + R.count()) { bad = 1; break; }
                    const uint32_t lv = R.packed() ? bits_le(s.def, s.def_n, uint64_t(R.data) + uint64_t(e - R.first) * uint64_t(bw), bw)
                                                   : R.data;
                    if (lv > maxd) bad = 1;
                    pm |= uint32_t(lv == maxd) << k;
                }
            }
        }
    }
    const uint32_t cnt = __popc(pm);
    uint32_t v0 = e0, tot = b1 - b0;   // value index of the thread's first present entry, present values of the block
    if (!allp) v0 = vb + block_excl_scan<NT>(cnt, S.scan_tmp, tot);
    const uint32_t ve = vb + tot;
    if (ve > cov) bad = 1;   // the id stream ends before the page's values do
    // ---- stage: run table; the id bytes of values [vb, ve)
    uint32_t mylo = 0xffffffffu, myhi = 0u;
    if (uint32_t(tid) < nr) {
        const uint32_t f = T->fp(tid), d = T->data(tid);
        const uint32_t nf = uint32_t(tid) + 1 < nr ? T->next_first(tid) : cov;
        S.rt[2 * tid] = f;
        S.rt[2 * tid + 1] = d;
        const uint32_t first = f & 0x7fffffffu;
        const uint32_t a = max(first, vb), z = min(nf, ve);
        if ((f >> 31) && a < z) {
            mylo = uint32_t((uint64_t(d) + uint64_t(a - first) * uint64_t(id_bw)) >> 3);
            myhi = uint32_t((uint64_t(d) + uint64_t(z - first) * uint64_t(id_bw) + 7u) >> 3);
        }
    }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mylo = min(mylo, uint32_t(__shfl_xor(mylo, d, 64)));
        myhi = max(myhi, uint32_t(__shfl_xor(myhi, d, 64)));
    }
    if ((tid & 63) == 0) { S.wlo[tid >> 6] = mylo; S.whi[tid >> 6] = myhi; }
    if (__syncthreads_or(bad)) {
        if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi);
        return;
    }
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
    // ---- ids of the thread's present values, spread over its entries
    uint32_t out[16];
    {
        uint32_t id[16];
        dstr_ids16(S.rt, nr, cov, v0, cnt, id_bw, bias, W, id);
        #pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            if (k < cnt && uint64_t(id[k]) >= dn) bad = 1;
        if (allp) {
            #pragma unroll
            for (uint32_t k = 0; k < 16; k++) out[k] = id[k];
        } else {
            uint32_t j = 0;   // present entries before entry k
            #pragma unroll
            for (uint32_t k = 0; k < 16; k++) {
                uint32_t v = 0;
                #pragma unroll
                for (uint32_t m = 0; m <= k; m++) v = j == m ? id[m] : v;
                const uint32_t p = (pm >> k) & 1u;
                out[k] = p ? v : 0u;
                j += p;
            }
        }
    }
    if (__syncthreads_or(bad)) {   // (also: every thread has read its ids before the window is reused)
        if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi);
        return;
    }
    // ---- indices: packed in the window on the 16-byte grid of the output, then aligned 16-byte stores
    const uintptr_t gout = reinterpret_cast<uintptr_t>(ck.values) + uintptr_t(slot0) * iw;
    const uint32_t a0 = uint32_t(gout & 15u);
    const uintptr_t g0 = gout - a0;
    const uint32_t vend = a0 + (b1 - b0) * iw;
    uint8_t* const w8 = reinterpret_cast<uint8_t*>(S.win);
    if (n > 0) {
        uint8_t* const mine = w8 + a0;   // (a0 is a multiple of iw: the array is 256-byte aligned)
        #pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            if (k < n) put_index(mine, uint64_t(e0 - b0 + k), iw, out[k]);
    }
    if (!allp && n > 0 && pm) {   // validity bits of the thread's entries
        const uint64_t rb = (slot0 + (e0 - b0)) - (slot0 & ~uint64_t(31));
        const uint64_t m = uint64_t(pm) << (rb & 31u);
        atomicOr(&S.vbits[rb >> 5], uint32_t(m));
        if (m >> 32) atomicOr(&S.vbits[(rb >> 5) + 1], uint32_t(m >> 32));
    }
    __syncthreads();
    for (uint32_t ci = tid; ci < (vend + 15u) / 16u; ci += NT) {
        const uint32_t vp = 16u * ci;
        if (vp >= a0 && vp + 16u <= vend) {
            *reinterpret_cast<PF_GLOBAL u32x4*>(g0 + vp) = S.win[ci];
        } else {   // the block's first and last chunk: the other bytes are a neighbour's
            for (uint32_t b = 0; b < 16u; b++)
                if (vp + b >= a0 && vp + b < vend) reinterpret_cast<uint8_t*>(g0 + vp)[b] = w8[vp + b];
        }
    }
    if (ck.max_def > 0 && ck.validity) {
        if (allp) fill_valid_ones(ck, slot0, slot1);
        else flush_bits(S.vbits, slot0, b1 - b0, ck.validity);
    }
    if (tid == 0) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values), (unsigned long long)tot);
        IDS_COUNT(0);
    }
}

// ---- k_dict_offsets: one workgroup per kept chunk. BYTE_ARRAY: offsets[i] = chars of entries [0, i), an exclusive
// scan of the lengths the dictionary walk (k_ba) left in dict_len, every {pos, len} checked against the dictionary
// page; then the dictionary's room in the chars arena, taken as k_scan takes a chunk's (a full arena is
// PF_ERR_CAPACITY, and the chars count towards the rerun's need through the chunk's num_chars).
__global__ __launch_bounds__(NT) void k_dict_offsets(const DevChunk* __restrict__ chunks, const DevPage* __restrict__ pages,
                                                     DevKeep* keeps, DevChunkResult* res, uint8_t* chars_arena, uint64_t arena_cap,
                                                     unsigned long long* arena_used) {
    __shared__ unsigned long long scan64[NT / 64];
    DevKeep& kp = keeps[blockIdx.x];
    const int c = kp.chunk;
    const DevChunk& ck = chunks[c];
    const int tid = threadIdx.x;
    if (res[c].status != 0 || ck.width != 0 || !kp.d_offsets) return;
    const uint64_t n = uint64_t(kp.n_entries > 0 ? kp.n_entries : 0);
    const uint64_t body = ck.dict_page >= 0 ? uint64_t(pages[ck.dict_page].body_len) : 0;
    int bad = (n > 0 && (!ck.dict_pos || !ck.dict_len || !ck.dict_data)) ? 1 : 0;
    uint64_t carry = 0;
    for (uint64_t i0 = 0; i0 < n && !bad; i0 += 16ull * NT) {
        const uint64_t i = i0 + 16ull * uint64_t(tid);
        uint32_t len[16];
        uint64_t sum = 0;
        #pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            len[k] = 0;
            if (i + k < n) {
                const uint64_t pos = ck.dict_pos[i + k];
                len[k] = ck.dict_len[i + k];
                if (pos > body || uint64_t(len[k]) > body - pos) { bad = 1; len[k] = 0; }
            }
            sum += len[k];
        }
        uint64_t tot;
        uint64_t at = carry + block_excl_scan64<NT>(sum, scan64, tot);
        #pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            at += len[k];
            if (i + k < n && at <= 0x7fffffffull) kp.d_offsets[i + k + 1] = int32_t(at);
        }
        carry += tot;
        bad = __syncthreads_or(bad);
    }
    bad = __syncthreads_or(bad);
    if (tid != 0) return;
    if (bad) { set_status(res, c, ST_CORRUPT, ck.dict_page); return; }
    kp.d_offsets[0] = 0;
    res[c].num_chars = int64_t(carry);
    kp.num_chars = int64_t(carry);
    if (carry > 0x7fffffffull) { set_status(res, c, ST_CAPACITY, -1); kp.d_chars = nullptr; return; }
    const unsigned long long need = (unsigned long long)((carry + 255) & ~uint64_t(255));
    const unsigned long long at = atomicAdd(arena_used, need);
    if (at + need > arena_cap) { set_status(res, c, ST_CAPACITY, -1); kp.d_chars = nullptr; }
    else kp.d_chars = chars_arena + at;
}

// ---- k_dict_pack: gridDim.y workgroups per kept chunk. A fixed-width dictionary is the decoded PLAIN page: its
// n_entries * width bytes, copied word by word. A BYTE_ARRAY dictionary's chars: one group of 16 lanes per entry of up
// to DICT_LONG bytes, the whole workgroup for a longer one.
__global__ __launch_bounds__(NT) void k_dict_pack(const DevChunk* __restrict__ chunks, const DevKeep* __restrict__ keeps,
                                                  const DevChunkResult* __restrict__ res) {
    const DevKeep& kp = keeps[blockIdx.x];
    const DevChunk& ck = chunks[kp.chunk];
    const uint32_t tid = threadIdx.x;
    if (res[kp.chunk].status != 0 || kp.n_entries <= 0 || !ck.dict_data) return;
    const uint64_t n = uint64_t(kp.n_entries);
    if (ck.width > 0) {
        if (!kp.d_values) return;
        const uint64_t bytes = n * uint64_t(ck.width);
        const uint8_t* src = ck.dict_data;
        for (uint64_t w = uint64_t(blockIdx.y) * NT + tid; 4 * w < bytes; w += uint64_t(gridDim.y) * NT) {
            if (4 * w + 4 <= bytes) {
                reinterpret_cast<uint32_t*>(kp.d_values)[w] = uint32_t(src[4 * w]) | uint32_t(src[4 * w + 1]) << 8 |
                                                              uint32_t(src[4 * w + 2]) << 16 | uint32_t(src[4 * w + 3]) << 24;
            } else {
                for (uint64_t b = 4 * w; b < bytes; b++) kp.d_values[b] = src[b];
            }
        }
        return;
    }
    if (!kp.d_chars || !kp.d_offsets || !ck.dict_pos || !ck.dict_len) return;
    const uint32_t grp = tid >> 4, l16 = tid & 15u;
    for (uint64_t i = uint64_t(blockIdx.y) * (NT / 16) + grp; i < n; i += uint64_t(gridDim.y) * (NT / 16)) {
        const uint32_t len = ck.dict_len[i];
        if (len > DICT_LONG) continue;
        const uint8_t* src = ck.dict_data + ck.dict_pos[i];
        uint8_t* dst = kp.d_chars + uint32_t(kp.d_offsets[i]);
        for (uint32_t b = l16; b < len; b += 16u) dst[b] = src[b];
    }
    for (uint64_t i = blockIdx.y; i < n; i += gridDim.y) {
        const uint32_t len = ck.dict_len[i];
        if (len <= DICT_LONG) continue;
        const uint8_t* src = ck.dict_data + ck.dict_pos[i];
        uint8_t* dst = kp.d_chars + uint32_t(kp.d_offsets[i]);
        for (uint32_t b = tid; b < len; b += NT) dst[b] = src[b];
    }
}

// d_blocks: the planner's L_IDS pairs; d_keeps / d_keep_of: the kept chunks' table and every chunk's entry in it.
// Nothing is launched for a batch without a kept chunk.
void launch_flat_ids(const DevChunk* d_chunks, DevPage* d_pages, const int2* d_blocks, int n_blocks, DevKeep* d_keeps, int n_keeps,
                     const int* d_keep_of, DevChunkResult* d_res, uint8_t* chars_arena, uint64_t arena_cap,
                     unsigned long long* arena_used, hipStream_t st) {
    if (n_keeps <= 0) return;
    if (n_blocks > 0)
        hipLaunchKernelGGL(k_flat_ids, dim3(n_blocks), dim3(NT), 0, st, d_chunks, d_pages, d_blocks, d_res, d_keeps, d_keep_of);
    hipLaunchKernelGGL(k_dict_offsets, dim3(n_keeps), dim3(NT), 0, st, d_chunks, d_pages, d_keeps, d_res, chars_arena, arena_cap,
                       arena_used);
    hipLaunchKernelGGL(k_dict_pack, dim3(n_keeps, 16), dim3(NT), 0, st, d_chunks, d_keeps, d_res);
}

}  // namespace pf
