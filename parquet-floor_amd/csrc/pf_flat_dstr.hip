// pf_flat_dstr.hip — k_flat_dstr, the lean kernel of the flat stage for small-dictionary string pages
// (DESIGN §4.34). Its id unpack is pf_dstr_ids.h, shared with the host check; launch_flat (pf_flat.hip)
// puts it on the stream between k_flat_fixed and k_flat_all through launch_flat_dstr.
#include <hip/hip_runtime.h>

#include "pf_dstr_ids.h"
#include "pf_flat.h"
#include "pf_launch.h"

namespace pf {

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
    if (ck.max_def > 0 && ck.validity) fill_valid_ones(ck, slot_base + b0, slot_base + b1);
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

// d_dblk: k_count_dict's (page, block) pairs (none: no launch)
void launch_flat_dstr(const DevChunk* d_chunks, DevPage* d_pages, const int2* d_dblk, int n_dblk, DevChunkResult* d_res,
                      hipStream_t st) {
    if (n_dblk > 0) hipLaunchKernelGGL(k_flat_dstr, dim3(n_dblk), dim3(NT), 0, st, d_chunks, d_pages, d_dblk, d_res);
}

}  // namespace pf
