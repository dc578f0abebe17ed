// pf_enc_delta.hip — write path: DELTA_BINARY_PACKED and DELTA_BYTE_ARRAY data pages, the encodings
// parquet-mr's PARQUET_2_0 writer uses for a chunk that is not dictionary-encoded (INT32 / INT64 and
// BINARY; DeltaBinaryPackingValuesWriterForInteger / ForLong, DeltaByteArrayWriter), on gfx950.
//
// A page is one stream (integers) or two streams plus its suffix bytes (strings: prefix lengths,
// suffix lengths). A stream of `cnt` values is one header item and ceil((cnt - 1) / 128) block items;
// every item is sized and written by one wave that looks at nothing but its own 128 deltas, and the
// items of a chunk are chained only through an exclusive scan of their byte sizes:
//
//   k_dl_prefix  strings: prefix / suffix length of every dense value against its predecessor in
//                the same page; an exclusive scan of the suffix lengths places the suffix bytes
//   k_dl_size    one wave per item: header bytes, or {min delta, 4 miniblock widths, block bytes}
//                (min-reduction across the wave, OR-reduction per 16 lanes = 32 values)
//   scan         exclusive sum of the item bytes; k_dl_totals sums a page's streams and suffixes
//   k_dl_write   the same grid: header varints, or zigzag(min delta), the width bytes and the
//                miniblocks, bit-packed in LDS (a miniblock of width w is exactly w dwords, so the
//                miniblocks of a block start dword-aligned there) and copied out bytewise: the
//                stream offset of a block has no alignment
//   k_dl_suffix  strings: suffix bytes of every dense value
//
// The last miniblock of a stream is padded to 32 values with zeros.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "pf_encode.h"

namespace pf {

namespace {
constexpr int ENT = 256;
constexpr uint32_t DL_BLOCK = 128;   // values per block; 4 miniblocks of 32

__device__ __forceinline__ uint32_t dl_varlen(uint64_t v) {
    uint32_t n = 1;
    while (v >= 0x80) { v >>= 7; n++; }
    return n;
}
__device__ __forceinline__ uint32_t dl_put_varint(uint8_t* o, uint64_t v) {
    uint32_t n = 0;
    while (v >= 0x80) { o[n++] = uint8_t(v | 0x80); v >>= 7; }
    o[n++] = uint8_t(v);
    return n;
}
__device__ __forceinline__ uint64_t dl_zigzag(int64_t v) { return (uint64_t(v) << 1) ^ uint64_t(v >> 63); }

// element i of a stream, sign-extended
__device__ __forceinline__ int64_t dl_load(const DeltaStream& s, uint32_t i) {
    return s.ew == 8 ? reinterpret_cast<const int64_t*>(s.src)[i] : int64_t(reinterpret_cast<const int32_t*>(s.src)[i]);
}

// the stream an item belongs to: the last one whose first item is <= item (streams[n].item0 = n_items)
__device__ __forceinline__ uint32_t dl_stream_of(const DeltaStream* __restrict__ s, uint32_t n, uint32_t item) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s[mid].item0 <= item) lo = mid; else hi = mid;
    }
    return lo;
}

// the page of dense value d: the last one whose d0 <= d (pages without values share the next one's d0)
__device__ __forceinline__ uint32_t dl_page_of(const DeltaPage* __restrict__ p, uint32_t n, uint32_t d) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p[mid].d0 <= d) lo = mid; else hi = mid;
    }
    return lo;
}

// Lane's two deltas of block `blk` (deltas 128 blk + 2 lane, + 1), wrapped to the element width and
// sign-extended; v0 / v1: the delta exists.
__device__ __forceinline__ void dl_deltas(const DeltaStream& s, uint32_t blk, int lane, int64_t& d0, int64_t& d1, bool& v0, bool& v1) {
    const uint64_t j = uint64_t(blk) * DL_BLOCK + uint32_t(lane) * 2u;
    v0 = j + 1 < s.cnt;
    v1 = j + 2 < s.cnt;
    const uint64_t a = v0 ? uint64_t(dl_load(s, uint32_t(j))) : 0u;
    const uint64_t b = v0 ? uint64_t(dl_load(s, uint32_t(j + 1))) : 0u;
    const uint64_t c = v1 ? uint64_t(dl_load(s, uint32_t(j + 2))) : 0u;
    d0 = int64_t(b - a);
    d1 = int64_t(c - b);
    if (s.ew == 4) { d0 = int64_t(int32_t(uint32_t(d0))); d1 = int64_t(int32_t(uint32_t(d1))); }
}
}  // namespace

// Strings: pfx[d] = common prefix with the previous present value of the same page (0 for a page's
// first value), sfx[d] = the rest; sfx[m] = 0 closes the scan.
__global__ __launch_bounds__(ENT) void k_dl_prefix(EncArgs a, DeltaArgs t, uint32_t m) {
    for (uint32_t d = blockIdx.x * ENT + threadIdx.x; d <= m; d += gridDim.x * ENT) {
        if (d == m) { t.sfx[m] = 0; t.pfx[m] = 0; continue; }
        const uint32_t len = a.dlen[d];
        uint32_t k = 0;
        if (d != t.pages[dl_page_of(t.pages, t.n_pages, d)].d0) {
            const uint32_t plen = a.dlen[d - 1];
            const uint32_t lim = len < plen ? len : plen;
            const uint8_t* x = a.chars + a.dsrc[d];
            const uint8_t* y = a.chars + a.dsrc[d - 1];
            while (k < lim && x[k] == y[k]) k++;
        }
        t.pfx[d] = k;
        t.sfx[d] = len - k;
    }
}

// One wave per item: bytes of a stream header, or a block's {min delta, widths, bytes}.
__global__ __launch_bounds__(64) void k_dl_size(DeltaArgs t) {
    const uint32_t item = blockIdx.x;
    const int lane = threadIdx.x;
    const DeltaStream s = t.streams[dl_stream_of(t.streams, t.n_streams, item)];
    const uint32_t k = item - s.item0;
    if (k == 0) {   // uvarint(128) uvarint(4) uvarint(count) zigzag(first)
        if (lane == 0) t.bytes[item] = 3u + dl_varlen(s.cnt) + dl_varlen(s.cnt ? dl_zigzag(dl_load(s, 0)) : 0u);
        return;
    }
    int64_t d0, d1;
    bool v0, v1;
    dl_deltas(s, k - 1, lane, d0, d1, v0, v1);
    long long mn = v0 ? d0 : 0x7fffffffffffffffll;
    if (v1 && d1 < mn) mn = d1;
    #pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const long long x = __shfl_xor(mn, o);
        mn = x < mn ? x : mn;
    }
    const uint64_t mask = s.ew == 8 ? ~0ull : 0xffffffffull;
    unsigned long long r = (v0 ? (uint64_t(d0) - uint64_t(mn)) & mask : 0ull) | (v1 ? (uint64_t(d1) - uint64_t(mn)) & mask : 0ull);
    #pragma unroll
    for (int o = 8; o >= 1; o >>= 1) r |= __shfl_xor(r, o);   // 16 lanes = one miniblock
    const uint32_t w = r ? 64u - uint32_t(__clzll(r)) : 0u;
    const uint32_t w0 = __shfl(w, 0), w1 = __shfl(w, 16), w2 = __shfl(w, 32), w3 = __shfl(w, 48);
    if (lane == 0) {
        t.minv[item] = mn;
        t.widths[item] = w0 | w1 << 8 | w2 << 16 | w3 << 24;
        t.bytes[item] = dl_varlen(dl_zigzag(mn)) + 4u + 4u * (w0 + w1 + w2 + w3);   // 32 values x w bits = 4 w bytes
    }
}

// totals[p] = bytes of page p's values section: its streams (+ suffix bytes)
__global__ __launch_bounds__(ENT) void k_dl_totals(DeltaArgs t) {
    const uint32_t p = blockIdx.x * ENT + threadIdx.x;
    if (p >= t.n_pages) return;
    const DeltaPage pg = t.pages[p];
    uint32_t b = t.off[t.streams[pg.s0 + pg.ns].item0] - t.off[t.streams[pg.s0].item0];
    if (t.spre) b += t.spre[pg.d0 + pg.cnt] - t.spre[pg.d0];
    t.totals[p] = b;
}

// One wave per item: the bytes k_dl_size measured, at the item's scanned offset in its page.
__global__ __launch_bounds__(64) void k_dl_write(DeltaArgs t) {
    __shared__ uint32_t buf[2 * DL_BLOCK];   // a block of 64-bit wide values: 128 x 8 bytes
    const uint32_t item = blockIdx.x;
    const int lane = threadIdx.x;
    const DeltaStream s = t.streams[dl_stream_of(t.streams, t.n_streams, item)];
    const DeltaPage pg = t.pages[s.page];
    uint8_t* o = t.out + pg.out_off + (t.off[item] - t.off[t.streams[pg.s0].item0]);
    const uint32_t k = item - s.item0;
    if (k == 0) {
        if (lane == 0) {
            o[0] = 0x80; o[1] = 0x01; o[2] = 0x04;
            uint32_t n = 3u + dl_put_varint(o + 3, s.cnt);
            dl_put_varint(o + n, s.cnt ? dl_zigzag(dl_load(s, 0)) : 0u);
        }
        return;
    }
    int64_t d0, d1;
    bool v0, v1;
    dl_deltas(s, k - 1, lane, d0, d1, v0, v1);
    const int64_t mn = t.minv[item];
    const uint32_t wd = t.widths[item];
    const uint64_t mask = s.ew == 8 ? ~0ull : 0xffffffffull;
    const uint64_t r[2] = {v0 ? (uint64_t(d0) - uint64_t(mn)) & mask : 0ull, v1 ? (uint64_t(d1) - uint64_t(mn)) & mask : 0ull};
    for (uint32_t i = lane; i < 2 * DL_BLOCK; i += 64) buf[i] = 0;
    __syncthreads();
    const uint32_t mb = uint32_t(lane) >> 4;
    const uint32_t w = (wd >> (8 * mb)) & 0xffu;
    uint32_t base = 0;   // dwords of the miniblocks before this one
    for (uint32_t q = 0; q < mb; q++) base += (wd >> (8 * q)) & 0xffu;
    #pragma unroll
    for (uint32_t e = 0; e < 2; e++) {
        if (r[e] == 0) continue;   // also every padding value of the last miniblock
        const uint32_t bit = ((uint32_t(lane) & 15u) * 2u + e) * w;
        const uint32_t dw = base + (bit >> 5), sh = bit & 31u;
        const uint64_t lo = r[e] << sh;                                  // a value spans up to three dwords
        const uint32_t hi = sh ? uint32_t(r[e] >> (64u - sh)) : 0u;
        if (uint32_t(lo) && dw < 2 * DL_BLOCK) atomicOr(&buf[dw], uint32_t(lo));
        if (uint32_t(lo >> 32) && dw + 1 < 2 * DL_BLOCK) atomicOr(&buf[dw + 1], uint32_t(lo >> 32));
        if (hi && dw + 2 < 2 * DL_BLOCK) atomicOr(&buf[dw + 2], hi);
    }
    __syncthreads();
    const uint32_t h = dl_varlen(dl_zigzag(mn)) + 4u;
    if (lane == 0) {
        const uint32_t n = dl_put_varint(o, dl_zigzag(mn));
        o[n] = uint8_t(wd); o[n + 1] = uint8_t(wd >> 8); o[n + 2] = uint8_t(wd >> 16); o[n + 3] = uint8_t(wd >> 24);
    }
    const uint32_t nb = 4u * ((wd & 0xffu) + ((wd >> 8) & 0xffu) + ((wd >> 16) & 0xffu) + (wd >> 24));
    for (uint32_t j = lane; j < nb; j += 64) o[h + j] = uint8_t(buf[j >> 2] >> (8u * (j & 3u)));
}

// Strings: the suffix bytes of every dense value, after its page's two streams.
__global__ __launch_bounds__(ENT) void k_dl_suffix(EncArgs a, DeltaArgs t, uint32_t m) {
    for (uint32_t d = blockIdx.x * ENT + threadIdx.x; d < m; d += gridDim.x * ENT) {
        const uint32_t n = t.sfx[d];
        if (!n) continue;
        const DeltaPage pg = t.pages[dl_page_of(t.pages, t.n_pages, d)];
        const uint32_t streams = t.off[t.streams[pg.s0 + pg.ns].item0] - t.off[t.streams[pg.s0].item0];
        uint8_t* q = t.out + pg.out_off + streams + (t.spre[d] - t.spre[pg.d0]);
        const uint8_t* x = a.chars + a.dsrc[d] + t.pfx[d];
        for (uint32_t k = 0; k < n; k++) q[k] = x[k];
    }
}

// ---------------------------------------------------------------- launchers
namespace {
inline unsigned grid_for(int64_t n) {
    const int64_t g = (n + ENT - 1) / ENT;
    return unsigned(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}
}  // namespace

// Strings: prefix / suffix lengths and the suffix byte positions (spre over m + 1).
hipError_t enc_delta_prefix(const EncArgs& a, const DeltaArgs& t, uint32_t m, void* temp, size_t temp_bytes, hipStream_t st) {
    hipLaunchKernelGGL(k_dl_prefix, dim3(grid_for(int64_t(m) + 1)), dim3(ENT), 0, st, a, t, m);
    size_t tb = temp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(temp, tb, t.sfx, t.spre, int(m + 1), st);
}

// Item sizes, their offsets (bytes[n_items] = 0 set by the host) and the pages' totals.
hipError_t enc_delta_sizes(const DeltaArgs& t, void* temp, size_t temp_bytes, hipStream_t st) {
    hipLaunchKernelGGL(k_dl_size, dim3(t.n_items), dim3(64), 0, st, t);
    size_t tb = temp_bytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(temp, tb, t.bytes, t.off, int(t.n_items + 1), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_dl_totals, dim3(grid_for(t.n_pages)), dim3(ENT), 0, st, t);
    return hipGetLastError();
}

void enc_delta_write(const EncArgs& a, const DeltaArgs& t, uint32_t m, hipStream_t st) {
    hipLaunchKernelGGL(k_dl_write, dim3(t.n_items), dim3(64), 0, st, t);
    if (t.spre && m) hipLaunchKernelGGL(k_dl_suffix, dim3(grid_for(m)), dim3(ENT), 0, st, a, t, m);
}

}  // namespace pf
