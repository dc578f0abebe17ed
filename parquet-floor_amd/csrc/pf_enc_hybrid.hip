// pf_enc_hybrid.hip — write path: RLE / bit-packed hybrid streams in the shape parquet-mr's
// RunLengthBitPackingHybridEncoder gives them (PF_ENCODE_HYBRID_RUNS): definition levels from the
// validity bits, dictionary ids, BOOLEAN values, on gfx950.
//
// The encoder is a value-by-value state machine, but its output is fixed by a chain of positions:
// with left[i] = entries from i on that equal v[i], a chain position i with left[i] >= 8 is an RLE run
// (varint(left << 1), the value in ceil(bw / 8) bytes) and the chain goes on at i + left[i]; any other
// chain position is a bit-packed group of v[i .. i + 7] and the chain goes on at i + 8. Consecutive
// groups share a header byte (groups << 1 | 1) per started block of 63.
//
// One workgroup per stream, the same grid for the size pass and the write pass; no lane walks the
// entries. A tile is HY_TILE entries in LDS and starts at a chain position where a packed stretch
// starts (the stream start, the end of an RLE run, or a group that opens a block of 63), so the only
// thing handed from tile to tile is that position:
//
//   run ends     reverse min-scan of the breaks v[i] != v[i + 1] over the tile and 7 entries past it:
//                enough to know left >= 8 for every entry of the tile
//   chain        next(i) = end of the run | i + 8; pointer jumping from entry 0 marks the chain in
//                ceil(log2(entries / 8)) rounds, fewer once 2^r steps leave the tile, none in a tile
//                without a run of 8 (the chain is every 8th entry)
//   stretches    max-scan of the positions where an RLE run ends: a group k groups into its stretch
//                writes a header when k % 63 == 0 and counts the groups of its block ahead of it
//   tile end     an RLE run that leaves the tile looks for its end with the whole workgroup, 1,024
//                entries a step; a packed stretch that leaves the tile is cut at its last header whose
//                block is not whole, and the next tile starts there
//   bytes        exclusive sum of the elements' bytes; the write pass packs groups as k_enc_pages does
//
// Vector stores and plain C++ only.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "pf_encode.h"

namespace pf {

namespace {
constexpr int HT = 256;                      // threads of a workgroup
constexpr uint32_t HY_TILE = 4096;           // entries of a tile (>= 2 blocks of 63 groups, so a cut tile advances)
constexpr uint32_t HY_C = HY_TILE / HT;      // entries of a thread in the scans
constexpr uint32_t HY_NONE = 0xffffffffu;
constexpr uint32_t F_CHAIN = 1, F_RLE = 2, F_START = 4, F_HDR = 8;

using HyScan = hipcub::BlockScan<uint32_t, HT>;

struct HyShared {
    uint32_t val[HY_TILE + 8];               // the tile, 7 entries past it, zeros past the stream
    uint16_t en[HY_TILE];                    // end of the run of equal values from i on (capped at the window)
    uint16_t nx[HY_TILE];                    // chain pointer (>= entries: leaves the tile)
    uint8_t fl[HY_TILE];                     // F_*
    uint32_t lastc, lasth, found;
    typename HyScan::TempStorage scan;
};

__device__ __forceinline__ uint32_t hy_varlen(uint32_t v) {
    uint32_t n = 1;
    while (v >= 0x80) { v >>= 7; n++; }
    return n;
}

__device__ __forceinline__ uint32_t hy_load(const HybridStream& s, uint32_t i) {
    const uint32_t e = s.first + i;
    if (s.kind == HY_IDS) return reinterpret_cast<const uint32_t*>(s.src)[e];
    if (s.kind == HY_BOOL) return s.src[e] & 1u;
    return s.src ? (uint32_t(s.src[e >> 3]) >> (e & 7u)) & 1u : 1u;
}

// One stream: its bytes (WRITE: also written at `o`).
template <bool WRITE>
__device__ uint32_t hy_stream(const HybridStream& s, uint8_t* o, HyShared& sh) {
    const uint32_t tid = threadIdx.x;
    const uint32_t cnt = s.cnt, bw = s.bw, vb = (bw + 7) >> 3;
    uint32_t t0 = 0, obase = 0;
    while (t0 < cnt) {
        const uint32_t W = min(HY_TILE + 7u, cnt - t0);   // window: entries whose value is looked at
        const uint32_t L = min(HY_TILE, cnt - t0);        // entries of the tile
        for (uint32_t i = tid; i < HY_TILE + 8; i += HT) sh.val[i] = i < W ? hy_load(s, t0 + i) : 0u;
        for (uint32_t i = tid; i < L; i += HT) sh.fl[i] = 0;
        if (tid == 0) { sh.lastc = 0; sh.lasth = 0; }
        __syncthreads();

        // ---- run ends: thread t scans chunk HT - 1 - t downwards, so a prefix scan over threads is a suffix scan over chunks
        {
            const uint32_t c = HT - 1 - tid;
            const uint32_t lo = min(c * HY_C, W), hi = c == HT - 1 ? W : min(c * HY_C + HY_C, W);
            uint32_t fb = HY_NONE;   // first break of the chunk
            for (uint32_t i = hi; i-- > lo;)
                if (i + 1 >= W || sh.val[i + 1] != sh.val[i]) fb = i;
            uint32_t later;
            HyScan(sh.scan).ExclusiveScan(fb, later, HY_NONE, hipcub::Min());
            uint32_t cur = later;
            for (uint32_t i = hi; i-- > lo;) {
                if (i + 1 >= W || sh.val[i + 1] != sh.val[i]) cur = i;
                if (i < L) sh.en[i] = uint16_t(cur + 1);
            }
        }
        __syncthreads();

        // ---- chain
        bool any_rle = false;
        for (uint32_t i = tid; i < L; i += HT) {
            const uint32_t e = sh.en[i];
            const bool rle = e - i >= 8;
            any_rle |= rle;
            sh.nx[i] = uint16_t(rle ? e : i + 8);
            sh.fl[i] = uint8_t((rle ? F_RLE : 0u) | (i == 0 ? F_CHAIN | F_START : 0u));
        }
        uint32_t rounds = 0;
        while ((1u << rounds) < (L + 7) / 8) rounds++;
        if (!__syncthreads_or(any_rle)) {   // no entry of the tile can start an RLE run: the chain is every 8th entry
            rounds = 0;
            for (uint32_t i = tid * 8; i < L; i += HT * 8) sh.fl[i] |= F_CHAIN;
            __syncthreads();
        }
        for (uint32_t r = 0; r < rounds; r++) {
            if (sh.nx[0] >= L) break;   // 2^r steps from entry 0 leave the tile: every chain position is marked
            for (uint32_t i = tid; i < L; i += HT)
                if (sh.fl[i] & F_CHAIN) {
                    const uint32_t j = sh.nx[i];
                    if (j < L) sh.fl[j] |= F_CHAIN;   // one writer per byte: jumps of equal length from chain positions differ
                }
            __syncthreads();
            uint16_t jj[HY_C];
            #pragma unroll
            for (uint32_t k = 0; k < HY_C; k++) {
                const uint32_t i = k * HT + tid;
                const uint32_t j = i < L ? sh.nx[i] : L;
                jj[k] = uint16_t(j < L ? sh.nx[j] : j);
            }
            __syncthreads();
            #pragma unroll
            for (uint32_t k = 0; k < HY_C; k++) {
                const uint32_t i = k * HT + tid;
                if (i < L) sh.nx[i] = jj[k];
            }
            __syncthreads();
        }

        // ---- packed stretches start where an RLE run of the chain ends
        for (uint32_t i = tid; i < L; i += HT)
            if ((sh.fl[i] & (F_CHAIN | F_RLE)) == (F_CHAIN | F_RLE) && sh.en[i] < L) sh.fl[sh.en[i]] |= F_START;
        __syncthreads();
        const uint32_t lo = min(tid * HY_C, L), hi = min(tid * HY_C + HY_C, L);
        {
            uint32_t lp = 0;   // last stretch start of the chunk, + 1
            for (uint32_t i = lo; i < hi; i++)
                if (sh.fl[i] & F_START) lp = i + 1;
            uint32_t before;
            HyScan(sh.scan).ExclusiveScan(lp, before, 0u, hipcub::Max());
            uint32_t p = before, lc = HY_NONE, lh = HY_NONE;
            for (uint32_t i = lo; i < hi; i++) {
                const uint32_t f = sh.fl[i];
                if (f & F_START) p = i + 1;
                if (!(f & F_CHAIN)) continue;
                lc = i;
                if (!(f & F_RLE) && ((i - (p - 1)) >> 3) % 63u == 0) { sh.fl[i] = uint8_t(f | F_HDR); lh = i; }
            }
            if (lc != HY_NONE) atomicMax(&sh.lastc, lc);
            if (lh != HY_NONE) atomicMax(&sh.lasth, lh);
        }
        __syncthreads();

        // ---- where the tile ends and the next one starts (uniform)
        const uint32_t lastc = sh.lastc;
        uint32_t cut = L, next, last_run = 0;
        if (sh.fl[lastc] & F_RLE) {
            uint32_t tend = t0 + sh.en[lastc];
            if (sh.en[lastc] == W && t0 + W < cnt) {   // the run leaves the window: its end, 4 HT entries a step
                const uint32_t v = sh.val[lastc];
                for (uint32_t base = t0 + W;; base += 4 * HT) {
                    if (tid == 0) sh.found = HY_NONE;
                    __syncthreads();
                    uint32_t m = HY_NONE;
                    #pragma unroll
                    for (uint32_t q = 0; q < 4; q++) {
                        const uint32_t pos = base + q * HT + tid;
                        if (pos >= cnt) m = min(m, cnt);
                        else if (hy_load(s, pos) != v) m = min(m, pos);
                    }
                    if (m != HY_NONE) atomicMin(&sh.found, m);
                    __syncthreads();
                    const uint32_t f = sh.found;
                    __syncthreads();
                    if (f != HY_NONE) { tend = f; break; }
                }
            }
            next = tend;
            last_run = tend - (t0 + lastc);
        } else if (t0 + lastc + 8 >= cnt) {
            next = cnt;                                           // the last group of the stream
        } else if (((lastc - sh.lasth) >> 3) + 1 == 63) {
            next = t0 + lastc + 8;                                // the last block is whole
        } else {
            cut = sh.lasth;                                       // the next tile starts with that block
            next = t0 + cut;
        }

        // ---- bytes of the elements, their offsets, the bytes
        uint32_t sum = 0;
        for (uint32_t i = lo; i < hi && i < cut; i++) {
            const uint32_t f = sh.fl[i];
            if (!(f & F_CHAIN)) continue;
            if (f & F_RLE) sum += hy_varlen((i == lastc ? last_run : uint32_t(sh.en[i]) - i) << 1) + vb;
            else sum += bw + ((f & F_HDR) ? 1u : 0u);
        }
        uint32_t off, total;
        HyScan(sh.scan).ExclusiveSum(sum, off, total);
        if (WRITE) {
            uint8_t* q = o + obase + off;
            for (uint32_t i = lo; i < hi && i < cut; i++) {
                const uint32_t f = sh.fl[i];
                if (!(f & F_CHAIN)) continue;
                if (f & F_RLE) {
                    uint32_t h = (i == lastc ? last_run : uint32_t(sh.en[i]) - i) << 1;
                    while (h >= 0x80) { *q++ = uint8_t(h | 0x80); h >>= 7; }
                    *q++ = uint8_t(h);
                    const uint32_t v = sh.val[i];
                    for (uint32_t b = 0; b < vb; b++) *q++ = uint8_t(v >> (8 * b));
                    continue;
                }
                if (f & F_HDR) {   // groups of this block: up to 63, up to the next RLE run or the end
                    uint32_t g = 1;
                    while (g < 63 && i + 8 * g < L && !(sh.fl[i + 8 * g] & F_RLE)) g++;
                    *q++ = uint8_t((g << 1) | 1u);
                }
                uint64_t w[5] = {0, 0, 0, 0, 0};   // 8 values x <= 32 bits
                #pragma unroll
                for (uint32_t k = 0; k < 8; k++) {
                    const uint64_t id = sh.val[i + k];
                    const uint32_t bit = k * bw;
                    w[bit >> 6] |= id << (bit & 63);
                    if ((bit & 63) + bw > 64) w[(bit >> 6) + 1] |= id >> (64 - (bit & 63));
                }
                for (uint32_t b = 0; b < bw; b++) *q++ = uint8_t(w[b >> 3] >> (8 * (b & 7)));
            }
        }
        obase += total;
        t0 = next;
        __syncthreads();   // the tile's arrays and the scan storage are reused
    }
    return obase;
}
}  // namespace

// Size pass: bytes[s] = bytes of stream s.
__global__ __launch_bounds__(HT) void k_hy_size(HybridArgs t) {
    __shared__ HyShared sh;
    const HybridStream s = t.streams[blockIdx.x];
    const uint32_t n = hy_stream<false>(s, nullptr, sh);
    if (threadIdx.x == 0) t.bytes[blockIdx.x] = n;
}

// Write pass: the stream at out_off, behind its prefix (the width byte of an id stream, the 4-byte
// length of a BOOLEAN stream).
__global__ __launch_bounds__(HT) void k_hy_write(HybridArgs t) {
    __shared__ HyShared sh;
    const HybridStream s = t.streams[blockIdx.x];
    uint8_t* o = t.out + s.out_off;
    if (threadIdx.x == 0) {
        if (s.prefix == HY_PREFIX_WIDTH) o[-1] = uint8_t(s.bw);
        if (s.prefix == HY_PREFIX_LENGTH) {
            const uint32_t n = t.bytes[blockIdx.x];
            o[-4] = uint8_t(n); o[-3] = uint8_t(n >> 8); o[-2] = uint8_t(n >> 16); o[-1] = uint8_t(n >> 24);
        }
    }
    hy_stream<true>(s, o, sh);
}

hipError_t enc_hybrid_sizes(const HybridArgs& t, hipStream_t st) {
    if (t.n_streams) hipLaunchKernelGGL(k_hy_size, dim3(t.n_streams), dim3(HT), 0, st, t);
    return hipGetLastError();
}

void enc_hybrid_write(const HybridArgs& t, hipStream_t st) {
    if (t.n_streams) hipLaunchKernelGGL(k_hy_write, dim3(t.n_streams), dim3(HT), 0, st, t);
}

}  // namespace pf
