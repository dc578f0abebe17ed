// pf_snappy_head.hip — Snappy pages that need no parse, decided from the page's layout.
//
// parquet-mr 1.12.2 hands every compressed page to snappy-java (DecompressorStream.java:101-173),
// whatever the stream holds. These two
// kernels run before the parse kernels (pf_snappy_parse.hip) and take the streams that are literals
// only; they read the page descriptors (DevPage / DevChunk) and the level section (pf_pages.h),
// which is why they are a unit of the page decode and not of the Snappy parser.
//
// Kernels:
//   k_snappy_head     one thread per job: single-literal pages stay in place, literal-only streams
//                     get a copy table, all-present PLAIN fixed-width pages are marked for direct
//                     writes into the column
//   k_snappy_litcopy  LC_SPLIT workgroups per literal-only page: its literals -> the scratch body
#include <hip/hip_runtime.h>

#include "pf_launch.h"
#include "pf_pages.h"
#include "pf_snappy_par.h"

namespace pf {

// ---- k_snappy_head: pages whose Snappy stream needs no executor or no scratch ----------------
//
// One thread per Snappy job of a data page, before the parse kernels (DecompressorStream.java:101-173
// hands every page to snappy-java; here two common shapes skip work):
//  * INPLACE: the stream is a single literal (incompressible pages: bit-packed dictionary ids,
//    dictionary pages of random data): the decompressed body IS the literal's bytes in the
//    compressed input. The page's body points there and every Snappy kernel skips the job
//    (FB_INPLACE): no index / chain / repair / splits / executor work, no scratch copy.
//  * VALUES: a PLAIN fixed-width page of a flat chunk whose levels are all present (v2: the level
//    section; v1: the first literal must hold the level section, as it does for parquet-mr and
//    Arrow pages) and whose values section is exactly num_values * width bytes: the executor
//    writes the values straight into the column (SnappyJob.ddst) and k_flat_fixed only sets the
//    validity bits of the page (north_star's fusion of decompression with the PLAIN decode).
// Anything else, and every page whose stream turns out not to parse, takes the normal path.
__global__ __launch_bounds__(64) void k_snappy_head(SnappyJob* __restrict__ jobs, int n_jobs, DevPage* __restrict__ pages,
                                                    const DevChunk* __restrict__ chunks, int* __restrict__ fb,
                                                    const DevChunkResult* __restrict__ res) {
    const int j = int(blockIdx.x) * 64 + int(threadIdx.x);
    if (j >= n_jobs || fb[j] != FB_OK) return;
    SnappyJob& J = jobs[j];
    DevPage& pg = pages[J.page];
    const DevChunk& ck = chunks[pg.chunk];
    if (res[pg.chunk].status != 0) return;
    const uint8_t* in = J.src;
    const uint64_t n = J.src_len;
    uint64_t pos = 0, ulen = 0;
    if (!uvarint(in, n, pos, ulen) || ulen != J.dst_len || pos >= n) return;
    const SnapTok t = snap_tok(glb_read8(in, n, pos));
    if (t.kind != 0) return;
    const uint64_t data = pos + t.arg;   // the first literal's bytes: in[data, data + t.ol)
    if (data + t.ol > n) return;
    const bool one = pos + t.tl == n && t.ol == J.dst_len;   // one literal covers the page
    if ((J.dflags & 2u) && !(one && !(pg.flags & PG_DICT))) {
        // a stream of literals only (incompressible data: Snappy emits one literal per 64 KiB block,
        // e.g. a 400 KB dictionary of random values is 7): copied to the scratch body by
        // k_snappy_litcopy from a table {data offset, output offset} per literal, kept in the job's
        // token bitmap (unused: no index pass runs on the job), without any parse. Dictionary pages
        // always take this (their decoded pointers were set from the scratch body, and gathers want it
        // aligned); data pages only when flagged by the host (compressed size >= uncompressed).
        uint32_t* tab = J.tokmap;
        uint64_t p = pos, o = 0;
        uint32_t cnt = 0;
        while (p < n && cnt < LC_MAX) {
            const SnapTok u = snap_tok(glb_read8(in, n, p));
            const uint64_t d = p + u.arg;
            if (u.kind != 0 || d + u.ol > n) break;
            tab[2 * cnt] = uint32_t(d);
            tab[2 * cnt + 1] = uint32_t(o);
            o += u.ol;
            p = d + u.ol;
            cnt++;
        }
        if (p == n && o == J.dst_len && cnt > 0) {
            J.lit = cnt;
            fb[j] = FB_LITCOPY;
            return;
        }
        // not a literal-only stream after all (a copy token, or more than LC_MAX literals): a data
        // page still gets the VALUES setup below (the partial table is overwritten by k_snappy_index)
    }
    if (pg.flags & PG_DICT) return;
    if (one) {
        pg.body = in + data;
        pg.direct = DIRECT_INPLACE;
        fb[j] = FB_INPLACE;
        return;
    }
    // PLAIN fixed width, flat, all present
    const int w = ck.width;
    if (pg.encoding != 0 || ck.max_rep != 0 || ck.ptype == 0 || ck.ptype == 6 || w <= 0 || !ck.values) return;
    // a page with a level table (null count not known to be zero: a v1 page without statistics) is decoded
    // from its scratch body by k_page_null / k_lvl + k_flat_null, which would overwrite values written direct
    if (pg.lvltab != nullptr) return;
    const uint32_t ne = uint32_t(pg.num_values);
    uint32_t L = 0;
    if (ck.max_def > 0) {
        const int bw = bit_width(uint32_t(ck.max_def));
        if (pg.flags & PG_V2) {
            if (!all_present(pg.lvl + pg.rep_len, pg.def_len, bw, ne, uint32_t(ck.max_def))) return;
        } else {
            if (pg.def_enc != 3 || t.ol < 4) return;
            const uint32_t lv = ld32le(in + data, 0, 4);
            if (lv > 60u || 4u + lv > t.ol) return;   // the level section must sit in the first literal
            if (!all_present(in + data + 4, lv, bw, ne, uint32_t(ck.max_def))) return;
            L = 4u + lv;
        }
    }
    if (uint64_t(J.dst_len) != uint64_t(L) + uint64_t(ne) * uint64_t(w)) return;
    uint8_t* dd = ck.values + uint64_t(pg.entry_start) * uint64_t(w) - L;
    const uintptr_t al = reinterpret_cast<uintptr_t>(dd);
    const uint32_t gran = (al & 15u) == 0 ? 16u : ((al & 7u) == 0 ? 8u : ((al & 3u) == 0 ? 4u : 0u));
    if (gran == 0) return;
    J.ddst = dd;
    J.dlo = L;
    J.dgran = gran;
    pg.direct = DIRECT_VALUES;
}

// Dictionary pages that are one Snappy literal (k_snappy_head: FB_LITCOPY): the literal's bytes to
// the page's 16-byte aligned scratch body, 16 bytes per thread per step (aligned dword loads +
// v_alignbyte), LC_SPLIT workgroups per page. The job's literals (k_snappy_head's table in its token
// bitmap: {data offset, output offset} per literal) are found by a binary search per 16-byte chunk;
// a chunk spanning two literals is copied byte by byte.
constexpr int LC_SPLIT = 16;
__global__ __launch_bounds__(NT) void k_snappy_litcopy(const SnappyJob* __restrict__ jobs, const int* __restrict__ list,
                                                       const int* __restrict__ fb) {
    __shared__ uint32_t tab[2 * LC_MAX];
    const int j = list[blockIdx.x];
    if (fb[j] != FB_LITCOPY) return;
    const SnappyJob& J = jobs[j];
    const uint32_t cnt = J.lit;
    if (threadIdx.x < 2 * cnt) tab[threadIdx.x] = J.tokmap[threadIdx.x];
    __syncthreads();
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(J.src);
    const uintptr_t send = s0 + J.src_len;   // aligned dwords below it are readable
    PF_GLOBAL uint8_t* d = gptr(J.dst);
    const uint32_t n = J.dst_len;
    for (uint32_t c = (blockIdx.y * NT + threadIdx.x) * 16u; c < n; c += LC_SPLIT * NT * 16u) {
        uint32_t lo = 0, hi = cnt;   // last literal whose output starts at or before c
        while (hi - lo > 1) {
            const uint32_t m = (lo + hi) >> 1;
            if (tab[2 * m + 1] <= c) lo = m; else hi = m;
        }
        const uint32_t oend = lo + 1 < cnt ? tab[2 * lo + 3] : n;
        if (c + 16u <= oend) {
            const uintptr_t sa = s0 + tab[2 * lo] + (c - tab[2 * lo + 1]);
            const uint32_t sh = uint32_t(sa & 3u);
            const PF_GLOBAL uint32_t* q = (const PF_GLOBAL uint32_t*)(sa & ~uintptr_t(3));
            uint32_t w[5];
            #pragma unroll
            for (int k = 0; k < 5; k++) w[k] = (sa & ~uintptr_t(3)) + 4u * uint32_t(k) < send ? q[k] : 0u;
            const u32x4 v = {__builtin_amdgcn_alignbyte(w[1], w[0], sh), __builtin_amdgcn_alignbyte(w[2], w[1], sh),
                             __builtin_amdgcn_alignbyte(w[3], w[2], sh), __builtin_amdgcn_alignbyte(w[4], w[3], sh)};
            *(PF_GLOBAL u32x4*)(d + c) = v;
        } else {   // the chunk ends the page or spans literals
            const PF_GLOBAL uint8_t* g = (const PF_GLOBAL uint8_t*)(J.src);
            uint32_t k = lo;
            for (uint32_t b = c; b < c + 16u && b < n; b++) {
                while (k + 1 < cnt && tab[2 * k + 3] <= b) k++;
                d[b] = g[tab[2 * k] + (b - tab[2 * k + 1])];
            }
        }
    }
}
void launch_snappy_litcopy(const SnappyJob* d_jobs, const int* d_list, int n, const int* d_fb, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_snappy_litcopy, dim3(n, LC_SPLIT), dim3(NT), 0, st, d_jobs, d_list, d_fb);
}
void launch_snappy_head(SnappyJob* d_jobs, int n_jobs, DevPage* d_pages, const DevChunk* d_chunks, int* d_fb,
                        const DevChunkResult* d_res, hipStream_t st) {
    if (n_jobs > 0)
        hipLaunchKernelGGL(k_snappy_head, dim3((n_jobs + 63) / 64), dim3(64), 0, st, d_jobs, n_jobs, d_pages, d_chunks, d_fb,
                           d_res);
}

}  // namespace pf
