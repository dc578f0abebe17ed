// pf_enc_stats.hip — min / max of a chunk's data pages and of the chunk (PF_ENCODE_STATISTICS),
// gfx950. Reductions over the dense values pf_encode_chunk already holds in HBM (EncArgs::dense, or
// dsrc / dlen + chars): null rows are not among them, so they never count.
//
//   k_enc_stats          one workgroup per (page, tile of ST_TILE dense values): every lane maps its values to
//                        an order-preserving unsigned key -- integers: sign bit flipped; FLOAT / DOUBLE: the
//                        total-order transform, NaN lanes contribute nothing; BOOLEAN: the byte; BYTE_ARRAY: the
//                        first 8 bytes big-endian, zero-padded, with min(len, 8) as the tie-break, so a proper
//                        prefix sorts first -- and the tile's {min, max, any} is reduced with shuffles, then LDS.
//   k_enc_stats_ties     BYTE_ARRAY only, same grid: the workgroup reduces its page's tile partials to the page's
//                        extreme keys, and only the values that carry such a key are compared byte by byte
//                        (a key of fewer than 8 bytes is the whole value: no compare). Each tile names its winners.
//   k_enc_stats_combine  one workgroup: tile partials -> page results -> chunk result; keys back to PLAIN
//                        bits (a zero min is -0.0, a zero max +0.0); the winning strings' bytes into the stat
//                        buffer unless len(min) + len(max) >= ST_LIMIT.
// Plain loads, stores and LDS: no atomics, and the result does not depend on the order workgroups run in.
#include <hip/hip_runtime.h>

#include "pf_encode.h"

namespace pf {

namespace {
constexpr int ST_NT = 256;
constexpr uint32_t ST_NONE = 0xffffffffu;

__device__ __forceinline__ bool kl_less(uint64_t k1, uint32_t l1, uint64_t k2, uint32_t l2) {
    return k1 < k2 || (k1 == k2 && l1 < l2);
}
__device__ __forceinline__ uint32_t shx32(uint32_t v, int d) { return uint32_t(__shfl_xor(int(v), d, 64)); }
__device__ __forceinline__ uint64_t shx64(uint64_t v, int d) {
    return uint64_t(shx32(uint32_t(v >> 32), d)) << 32 | shx32(uint32_t(v), d);
}

// Key of dense value d; false when the value takes no part (NaN).
__device__ __forceinline__ bool stat_key(const EncArgs& a, uint32_t d, uint64_t& k, uint32_t& l) {
    l = 0;
    if (a.ptype == PF_BYTE_ARRAY) {
        const uint32_t len = a.dlen[d];
        const uint8_t* p = a.chars + a.dsrc[d];
        l = min(len, 8u);
        k = 0;
        for (uint32_t i = 0; i < l; i++) k |= uint64_t(p[i]) << (56u - 8u * i);
        return true;
    }
    if (a.ptype == PF_BOOLEAN) { k = a.dense[d] & 1u; return true; }
    if (a.width == 4) {
        const uint32_t b = reinterpret_cast<const uint32_t*>(a.dense)[d];
        if (a.ptype == PF_INT32) { k = b ^ 0x80000000u; return true; }
        if ((b & 0x7fffffffu) > 0x7f800000u) return false;
        k = (b & 0x80000000u) ? uint32_t(~b) : (b | 0x80000000u);
        return true;
    }
    const uint64_t b = reinterpret_cast<const uint64_t*>(a.dense)[d];
    if (a.ptype == PF_INT64) { k = b ^ (1ull << 63); return true; }
    if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return false;
    k = (b >> 63) ? ~b : (b | (1ull << 63));
    return true;
}

// PLAIN bits of a key; a zero of either sign becomes -0.0 as a min and +0.0 as a max.
__device__ __forceinline__ uint64_t stat_bits(const EncArgs& a, uint64_t k, bool is_min) {
    if (a.ptype == PF_BOOLEAN) return k;
    if (a.width == 4) {
        const uint32_t k32 = uint32_t(k);
        if (a.ptype == PF_INT32) return k32 ^ 0x80000000u;
        const uint32_t b = (k32 & 0x80000000u) ? (k32 ^ 0x80000000u) : ~k32;
        return (b & 0x7fffffffu) ? b : (is_min ? 0x80000000u : 0u);
    }
    if (a.ptype == PF_INT64) return k ^ (1ull << 63);
    const uint64_t b = (k >> 63) ? (k ^ (1ull << 63)) : ~k;
    return (b & 0x7fffffffffffffffull) ? b : (is_min ? (1ull << 63) : 0ull);
}

// bytes of dense value x < bytes of dense value y: unsigned, a proper prefix first. The two carry the same
// key, so their first `from` = min(len, 8) bytes are known to be equal and the compare starts behind them.
__device__ bool str_less(const EncArgs& a, uint32_t x, uint32_t y, uint32_t from) {
    const uint32_t lx = a.dlen[x], ly = a.dlen[y], n = min(lx, ly);
    const uint8_t* px = a.chars + a.dsrc[x];
    const uint8_t* py = a.chars + a.dsrc[y];
    for (uint32_t i = from; i < n; i++)
        if (px[i] != py[i]) return px[i] < py[i];
    return lx < ly;
}
__device__ __forceinline__ uint32_t pick_min(const EncArgs& a, uint32_t x, uint32_t y, uint32_t from) {
    if (x == ST_NONE) return y;
    if (y == ST_NONE) return x;
    return str_less(a, y, x, from) ? y : x;
}
__device__ __forceinline__ uint32_t pick_max(const EncArgs& a, uint32_t x, uint32_t y, uint32_t from) {
    if (x == ST_NONE) return y;
    if (y == ST_NONE) return x;
    return str_less(a, x, y, from) ? y : x;
}

struct Ext {   // extreme keys seen so far (any == 0: none; the other fields then never win a compare)
    uint64_t mn = ~0ull, mx = 0;
    uint32_t mnl = ~0u, mxl = 0, any = 0;
    __device__ __forceinline__ void add(uint64_t k, uint32_t l) {
        if (!any || kl_less(k, l, mn, mnl)) { mn = k; mnl = l; }
        if (!any || kl_less(mx, mxl, k, l)) { mx = k; mxl = l; }
        any = 1;
    }
    __device__ __forceinline__ void merge(uint64_t omn, uint32_t omnl, uint64_t omx, uint32_t omxl, uint32_t oany) {
        if (!oany) return;
        if (!any || kl_less(omn, omnl, mn, mnl)) { mn = omn; mnl = omnl; }
        if (!any || kl_less(mx, mxl, omx, omxl)) { mx = omx; mxl = omxl; }
        any = 1;
    }
};

// The workgroup's extremes: across the wave with shuffles, across waves through LDS; the result in sh[0],
// visible to every thread on return.
__device__ __forceinline__ void block_extremes(Ext r, StatPart* sh) {
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t omn = shx64(r.mn, d), omx = shx64(r.mx, d);
        const uint32_t omnl = shx32(r.mnl, d), omxl = shx32(r.mxl, d), oany = shx32(r.any, d);
        r.merge(omn, omnl, omx, omxl, oany);
    }
    const int tid = threadIdx.x;
    __syncthreads();   // sh may still be read from an earlier call
    if ((tid & 63) == 0) sh[tid >> 6] = StatPart{r.mn, r.mx, r.mnl, r.mxl, ST_NONE, ST_NONE, r.any, 0u};
    __syncthreads();
    if (tid == 0) {
        Ext t;
        for (int w = 0; w < ST_NT / 64; w++) t.merge(sh[w].mn, sh[w].mnl, sh[w].mx, sh[w].mxl, sh[w].any);
        sh[0] = StatPart{t.mn, t.mx, t.mnl, t.mxl, ST_NONE, ST_NONE, t.any, 0u};
    }
    __syncthreads();
}
}  // namespace

__global__ __launch_bounds__(ST_NT) void k_enc_stats(EncArgs a, StatArgs s) {
    __shared__ StatPart sh[ST_NT / 64];
    const StatTile t = s.tiles[blockIdx.x];
    Ext r;
    for (uint32_t e = threadIdx.x; e < t.cnt; e += ST_NT) {
        uint64_t k;
        uint32_t l;
        if (stat_key(a, t.d0 + e, k, l)) r.add(k, l);
    }
    block_extremes(r, sh);
    if (threadIdx.x == 0) s.part[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(ST_NT) void k_enc_stats_ties(EncArgs a, StatArgs s) {
    __shared__ StatPart sh[ST_NT / 64];
    __shared__ uint32_t wmin[ST_NT / 64], wmax[ST_NT / 64];
    const StatTile t = s.tiles[blockIdx.x];
    const int tid = threadIdx.x;
    Ext r;   // the page's extreme keys, from its tiles' partials
    for (uint32_t i = s.ptile[t.page] + tid; i < s.ptile[t.page + 1]; i += ST_NT) {
        const StatPart q = s.part[i];
        r.merge(q.mn, q.mnl, q.mx, q.mxl, q.any);
    }
    block_extremes(r, sh);
    const StatPart pg = sh[0];
    uint32_t bmin = ST_NONE, bmax = ST_NONE;
    for (uint32_t e = tid; e < t.cnt && pg.any; e += ST_NT) {
        const uint32_t d = t.d0 + e;
        uint64_t k;
        uint32_t l;
        stat_key(a, d, k, l);
        // fewer than 8 bytes: the key is the value, every candidate is the same bytes
        if (k == pg.mn && l == pg.mnl) bmin = (bmin == ST_NONE || l < 8) ? (bmin == ST_NONE ? d : bmin) : pick_min(a, bmin, d, 8);
        if (k == pg.mx && l == pg.mxl) bmax = (bmax == ST_NONE || l < 8) ? (bmax == ST_NONE ? d : bmax) : pick_max(a, bmax, d, 8);
    }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t omin = shx32(bmin, d), omax = shx32(bmax, d);
        bmin = pick_min(a, bmin, omin, pg.mnl);
        bmax = pick_max(a, bmax, omax, pg.mxl);
    }
    if ((tid & 63) == 0) { wmin[tid >> 6] = bmin; wmax[tid >> 6] = bmax; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < ST_NT / 64; w++) { bmin = pick_min(a, bmin, wmin[w], pg.mnl); bmax = pick_max(a, bmax, wmax[w], pg.mxl); }
        s.win[2 * blockIdx.x] = bmin;
        s.win[2 * blockIdx.x + 1] = bmax;
    }
}

__global__ __launch_bounds__(ST_NT) void k_enc_stats_combine(EncArgs a, StatArgs s) {
    const bool str = a.ptype == PF_BYTE_ARRAY;
    const uint32_t tid = threadIdx.x, np = s.n_pages;
    // tile partials -> page results
    for (uint32_t p = tid; p < np; p += ST_NT) {
        const uint32_t t0 = s.ptile[p], t1 = s.ptile[p + 1];
        Ext r;
        for (uint32_t i = t0; i < t1; i++) {
            const StatPart q = s.part[i];
            r.merge(q.mn, q.mnl, q.mx, q.mxl, q.any);
        }
        uint32_t mni = ST_NONE, mxi = ST_NONE;
        for (uint32_t i = t0; i < t1 && str && r.any; i++) {   // the tiles that hold the page's extreme keys name a winner
            const StatPart q = s.part[i];
            if (q.any && q.mn == r.mn && q.mnl == r.mnl) mni = pick_min(a, mni, s.win[2 * i], r.mnl);
            if (q.any && q.mx == r.mx && q.mxl == r.mxl) mxi = pick_max(a, mxi, s.win[2 * i + 1], r.mxl);
        }
        s.out[p] = StatPart{r.mn, r.mx, r.mnl, r.mxl, mni, mxi, r.any, 0u};
    }
    __syncthreads();
    // page results -> chunk result: thread 0 the min, the first thread of the next wave the max
    if (tid == 0 || tid == 64) {
        const bool is_min = tid == 0;
        uint64_t k = 0;
        uint32_t l = 0, idx = ST_NONE, any = 0;
        for (uint32_t p = 0; p < np; p++) {
            const StatPart q = s.out[p];
            if (!q.any) continue;
            const uint64_t qk = is_min ? q.mn : q.mx;
            const uint32_t ql = is_min ? q.mnl : q.mxl, qi = is_min ? q.mni : q.mxi;
            if (!any || (is_min ? kl_less(qk, ql, k, l) : kl_less(k, l, qk, ql))) { k = qk; l = ql; idx = qi; }
            else if (str && qk == k && ql == l && l == 8) idx = is_min ? pick_min(a, idx, qi, 8) : pick_max(a, idx, qi, 8);
            any = 1;
        }
        StatPart* c = s.out + np;
        if (is_min) { c->mn = k; c->mnl = l; c->mni = idx; c->any = any; c->pad = 0; }
        else { c->mx = k; c->mxl = l; c->mxi = idx; }
    }
    __syncthreads();
    // keys -> PLAIN bits; strings: the lengths, and the size limit
    for (uint32_t e = tid; e <= np; e += ST_NT) {
        StatPart r = s.out[e];
        if (!r.any) continue;
        if (str && (r.mni == ST_NONE || r.mxi == ST_NONE)) {   // cannot happen: a tile that holds the key names a value
            r.any = 0;
        } else if (str) {
            r.mnl = a.dlen[r.mni];
            r.mxl = a.dlen[r.mxi];
            if (uint64_t(r.mnl) + r.mxl >= ST_LIMIT) r.any = 2;
        } else {
            r.mn = stat_bits(a, r.mn, true);
            r.mx = stat_bits(a, r.mx, false);
        }
        s.out[e] = r;
    }
    if (!str) return;
    __syncthreads();
    for (uint32_t e = 0; e <= np; e++) {   // min ‖ max of every entry that keeps them: fewer than ST_LIMIT bytes
        const StatPart r = s.out[e];
        if (r.any != 1) continue;
        uint8_t* o = s.bytes + uint64_t(e) * ST_LIMIT;
        const uint8_t* pmin = a.chars + a.dsrc[r.mni];
        const uint8_t* pmax = a.chars + a.dsrc[r.mxi];
        for (uint32_t i = tid; i < r.mnl; i += ST_NT) o[i] = pmin[i];
        for (uint32_t i = tid; i < r.mxl; i += ST_NT) o[r.mnl + i] = pmax[i];
    }
}

void enc_stats(const EncArgs& a, const StatArgs& s, hipStream_t st) {
    if (s.n_tiles) hipLaunchKernelGGL(k_enc_stats, dim3(s.n_tiles), dim3(ST_NT), 0, st, a, s);
    if (s.n_tiles && a.ptype == PF_BYTE_ARRAY) hipLaunchKernelGGL(k_enc_stats_ties, dim3(s.n_tiles), dim3(ST_NT), 0, st, a, s);
    hipLaunchKernelGGL(k_enc_stats_combine, dim3(1), dim3(ST_NT), 0, st, a, s);
}

}  // namespace pf
