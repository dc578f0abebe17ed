// pf_enc_pgindex.hip — the ColumnIndex lists of one chunk (PF_ENCODE_PAGE_INDEX), gfx950.
//
//   k_enc_pgindex   one workgroup of 256 threads, behind k_enc_stats_combine, whose page results (StatArgs::out)
//                   are all it reads besides the pages' row / value counts and, for BYTE_ARRAY, the winners'
//                   bytes at chars + dsrc[mni / mxi] (never StatArgs::bytes: a value past ST_LIMIT is still
//                   truncated here, and no long value crosses to the host).
//     1  per page (strided): null_page, null_count, the lengths of its min and max entry. A BYTE_ARRAY min
//        longer than T is its first T bytes; a longer max is its first T bytes less trailing 0xFF bytes with
//        the last byte left incremented -- the shortest upper bound under the unsigned bytewise order -- and
//        when nothing is left the chunk gets no ColumnIndex. A page with values but no min / max (all NaN)
//        clears the flag too; so does an entry over ST_LIMIT when nothing is truncated.
//     2  exclusive scan of the 2 x n_pages entry lengths (shuffles inside a wave, LDS across the four).
//     3  the bytes: every thread takes bytes of the value block, finds their entry by bisecting the offsets,
//        and loads from the page result (fixed width: the PLAIN bits) or from chars.
//     4  boundary order over the written entries: the pages that are not null pages are compacted (ballot and
//        popcount), one thread per adjacent pair compares mins and maxes under the type's order (signed
//        integers; FLOAT / DOUBLE by value; bytes unsigned, a proper prefix first), and "never decreasing" /
//        "never increasing" are reduced through two LDS words that only ever go from 0 to 1.
// Plain loads, stores, LDS and wave intrinsics: no atomics, nothing depends on scheduling. No lane walks the pages.
#include <hip/hip_runtime.h>

#include "pf_encode.h"

namespace pf {

namespace {
constexpr int PX_NT = 256;

// Exclusive prefix of v over the workgroup, and the workgroup's total. sh: PX_NT / 64 words.
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* sh, uint32_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = uint32_t(__shfl_up(int(inc), d, 64));
        if (lane >= d) inc += o;
    }
    __syncthreads();   // sh may still be read from an earlier call
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
    #pragma unroll
    for (int i = 0; i < PX_NT / 64; i++) {
        if (i < w) base += sh[i];
        total += sh[i];
    }
    return base + inc - v;
}

// The same for one flag per thread: a ballot and two popcounts instead of the shuffles.
__device__ __forceinline__ uint32_t block_exclusive_flag(bool f, uint32_t* sh, uint32_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    __syncthreads();
    if (lane == 0) sh[w] = uint32_t(__popcll(b));
    __syncthreads();
    uint32_t base = 0;
    total = 0;
    #pragma unroll
    for (int i = 0; i < PX_NT / 64; i++) {
        if (i < w) base += sh[i];
        total += sh[i];
    }
    return base + uint32_t(__popcll(b & ((1ull << lane) - 1ull)));
}

// Written entry e1 against e2: < 0, 0, > 0 under the type's order.
__device__ int entry_cmp(const EncArgs& a, const PgIndexArgs& x, uint32_t e1, uint32_t e2) {
    const uint32_t o1 = x.off[e1], l1 = x.off[e1 + 1] - o1, o2 = x.off[e2], l2 = x.off[e2 + 1] - o2;
    const uint8_t* p1 = x.values + o1;
    const uint8_t* p2 = x.values + o2;
    if (a.ptype == PF_BYTE_ARRAY) {
        const uint32_t n = min(l1, l2);
        for (uint32_t i = 0; i < n; i++)
            if (p1[i] != p2[i]) return p1[i] < p2[i] ? -1 : 1;
        return l1 < l2 ? -1 : (l1 > l2 ? 1 : 0);
    }
    uint64_t b1 = 0, b2 = 0;   // little-endian PLAIN bits (l1 == l2 == width)
    for (uint32_t i = 0; i < l1 && i < 8; i++) { b1 |= uint64_t(p1[i]) << (8u * i); b2 |= uint64_t(p2[i]) << (8u * i); }
    switch (a.ptype) {
    case PF_INT32: { const int32_t v1 = int32_t(uint32_t(b1)), v2 = int32_t(uint32_t(b2)); return v1 < v2 ? -1 : (v1 > v2 ? 1 : 0); }
    case PF_INT64: { const int64_t v1 = int64_t(b1), v2 = int64_t(b2); return v1 < v2 ? -1 : (v1 > v2 ? 1 : 0); }
    case PF_FLOAT: { const float v1 = __uint_as_float(uint32_t(b1)), v2 = __uint_as_float(uint32_t(b2)); return v1 < v2 ? -1 : (v1 > v2 ? 1 : 0); }
    case PF_DOUBLE: { const double v1 = __longlong_as_double((long long)b1), v2 = __longlong_as_double((long long)b2); return v1 < v2 ? -1 : (v1 > v2 ? 1 : 0); }
    default: return b1 < b2 ? -1 : (b1 > b2 ? 1 : 0);   // BOOLEAN
    }
}
}  // namespace

__global__ __launch_bounds__(PX_NT) void k_enc_pgindex(EncArgs a, PgIndexArgs x) {
    __shared__ uint32_t sh[PX_NT / 64];
    __shared__ uint32_t bad, not_asc, not_desc;
    const bool str = a.ptype == PF_BYTE_ARRAY;
    const uint32_t tid = threadIdx.x, np = x.n_pages, E = 2u * np, T = x.trunc;
    if (tid == 0) { bad = 0; not_asc = 0; not_desc = 0; }
    __syncthreads();
    // 1: null pages, null counts, entry lengths
    for (uint32_t p = tid; p < np; p += PX_NT) {
        const uint32_t cnt = x.cnt[p];
        x.null_pages[p] = cnt == 0;
        x.null_counts[p] = (long long)x.rows[p] - (long long)cnt;
        uint32_t lmin = 0, lmax = 0;
        if (cnt) {
            const StatPart r = x.pages[p];
            if (r.any == 0) {
                bad = 1;
            } else if (!str) {
                lmin = lmax = uint32_t(a.width);
            } else if (T == PX_NO_TRUNC) {
                if (r.any == 2) bad = 1;
                else { lmin = r.mnl; lmax = r.mxl; }
            } else {
                lmin = min(r.mnl, T);
                lmax = r.mxl;
                if (r.mxl > T) {
                    const uint8_t* q = a.chars + a.dsrc[r.mxi];
                    lmax = T;
                    while (lmax && q[lmax - 1] == 0xffu) lmax--;
                    if (!lmax) { bad = 1; lmin = 0; }
                }
            }
        }
        x.off[2 * p] = lmin;
        x.off[2 * p + 1] = lmax;
    }
    __syncthreads();
    // 2: lengths -> offsets
    uint32_t carry = 0;
    for (uint32_t base = 0; base < E; base += PX_NT) {
        const uint32_t i = base + tid, v = i < E ? x.off[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive(v, sh, total);
        if (i < E) x.off[i] = carry + ex;
        carry += total;
    }
    if (tid == 0) x.off[E] = carry;
    if (carry > x.value_cap) bad = 1;   // cannot happen: the host reserves the worst case
    __syncthreads();
    // 3: the bytes
    const uint32_t nbytes = min(carry, x.value_cap);
    for (uint32_t b = tid; b < nbytes; b += PX_NT) {
        uint32_t lo = 0, hi = E;   // the entry with off[e] <= b < off[e + 1]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (x.off[mid] <= b) lo = mid; else hi = mid;
        }
        const uint32_t e = lo, p = e >> 1, i = b - x.off[e];
        const bool is_max = (e & 1u) != 0;
        const StatPart& r = x.pages[p];
        uint8_t v;
        if (!str) {
            v = uint8_t((is_max ? r.mx : r.mn) >> (8u * i));
        } else {
            const uint32_t d = is_max ? r.mxi : r.mni, len = x.off[e + 1] - x.off[e];
            v = a.chars[a.dsrc[d] + i];
            if (is_max && len < a.dlen[d] && i == len - 1) v = uint8_t(v + 1u);   // truncated: not 0xFF, so no carry
        }
        x.values[b] = v;
    }
    // 4: boundary order over the pages that are not null pages
    uint32_t nnz = 0;
    for (uint32_t base = 0; base < np; base += PX_NT) {
        const uint32_t p = base + tid;
        const bool f = p < np && x.cnt[p] != 0;
        uint32_t total;
        const uint32_t ex = block_exclusive_flag(f, sh, total);
        if (f) x.nn[nnz + ex] = p;
        nnz += total;
    }
    __syncthreads();   // the values and nn are written
    if (!bad) {
        for (uint32_t j = tid; j + 1 < nnz; j += PX_NT) {
            const uint32_t pa = x.nn[j], pb = x.nn[j + 1];
            const int cmin = entry_cmp(a, x, 2 * pa, 2 * pb), cmax = entry_cmp(a, x, 2 * pa + 1, 2 * pb + 1);
            if (cmin > 0 || cmax > 0) not_asc = 1;
            if (cmin < 0 || cmax < 0) not_desc = 1;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t order = (bad || nnz == 0) ? 0u : (!not_asc ? 1u : (!not_desc ? 2u : 0u));
        *x.head = PgIndexHead{bad ? 0u : 1u, order, carry, nnz};
    }
}

void enc_pgindex(const EncArgs& a, const PgIndexArgs& x, hipStream_t st) {
    hipLaunchKernelGGL(k_enc_pgindex, dim3(1), dim3(PX_NT), 0, st, a, x);
}

}  // namespace pf
