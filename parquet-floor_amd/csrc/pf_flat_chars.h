// pf_flat_chars.h — the chars copiers of the flat string path: a tile's values, given as LDS tables of
// output offsets (coff) and source positions (csrc), copied cooperatively into the chars arena.
//   copy_chars_short   values of a few bytes, one value per thread
//   copy_chars_plain   PLAIN pages: 64-byte output spans from one round of source loads
//   copy_chars_fast    everything else: 16-byte output chunks (copy_chunk16)
// Only pf_flat.hip (flat_block) includes it today; it is a header so that the next string-path kernel can.
#pragma once
#include "pf_pages.h"

namespace pf {

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

}  // namespace pf
