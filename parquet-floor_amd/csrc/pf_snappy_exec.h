// pf_snappy_exec.h — device code the two Snappy executors share: k_snappy_exec5 (pf_snappy_exec.hip) and
// the diagnostics build's k_snappy_exec2 (pf_snappy_exec2.hip). Both decode a piece's tokens into an LDS
// ring of the newest XRING output bytes and flush it to the page's output in whole XSLOT slots.
#pragma once
#include "pf_snappy_par.h"

namespace pf {

#ifndef PF_XRING
#define PF_XRING 4096
#endif
constexpr uint32_t XRING = PF_XRING; // output ring (LDS); copies reaching further back read HBM (far copies)
constexpr uint32_t XRMASK = XRING - 1;
constexpr uint32_t XSLOT = 1024;     // flush granule
constexpr uint32_t XST = XSLOT / 64 / 16;   // 16-byte stores per lane per slot (flush_slots)
constexpr uint32_t XCHUNK = 1024;    // input bytes whose tokens are enumerated at once
constexpr uint32_t XSTAGE = XCHUNK + 64 + 16;
constexpr uint32_t XLIT = 1024;      // long literals are copied in pieces of this many bytes

__device__ __forceinline__ void wait_vmem() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Where a job's output goes: dst + a, or for a direct job (k_snappy_head) ddst + a from output
// offset dlo on (the column's values; dgran-wide stores, ddst's alignment).
struct OutDst {
    PF_GLOBAL uint8_t* dst;
    PF_GLOBAL uint8_t* dd;   // null: not direct
    uint32_t dlo, gran;
};

// Rare: a 16-byte chunk holding the end of the level section (kept out of put16's registers). Called, not
// inlined: each unit's device code links its own copy (the linkage it had in the single file, so
// k_snappy_exec5's call sequence is the one it was).
__device__ __attribute__((noinline)) void put16_split(PF_GLOBAL uint8_t* dst, PF_GLOBAL uint8_t* dd, uint32_t dlo, uint32_t a,
                                                     u32x4 v) {
    for (uint32_t k = 0; k < 16; k++) {
        const uint8_t b = uint8_t(v[k >> 2] >> (8 * (k & 3)));
        (a + k < dlo ? dst : dd)[a + k] = b;
    }
}

// 16 output bytes at the 16-aligned output offset a.
__device__ __forceinline__ void put16(const OutDst& o, uint32_t a, u32x4 v) {
    if (o.dd == nullptr || a + 16u <= o.dlo) {
        *(PF_GLOBAL u32x4*)(o.dst + a) = v;
    } else if (a >= o.dlo) {
        PF_GLOBAL uint8_t* p = o.dd + a;
        if (o.gran == 16u) {
            *(PF_GLOBAL u32x4*)p = v;
        } else if (o.gran == 8u) {
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            reinterpret_cast<PF_GLOBAL u32x2*>(p)[0] = u32x2{v.x, v.y};
            reinterpret_cast<PF_GLOBAL u32x2*>(p)[1] = u32x2{v.z, v.w};
        } else {
            PF_GLOBAL uint32_t* q = reinterpret_cast<PF_GLOBAL uint32_t*>(p);
            q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
        }
    } else {   // straddles dlo (the end of the level section)
        put16_split(o.dst, o.dd, o.dlo, a, v);
    }
}
__device__ __forceinline__ void put1(const OutDst& o, uint32_t a, uint8_t b) {
    (o.dd == nullptr || a < o.dlo ? o.dst : o.dd)[a] = b;
}

// Store ring bytes [F, upto) in whole XSLOT slots (16-byte stores, XSLOT / 64 bytes per lane).
// Returns the number of store instructions issued.
__device__ __forceinline__ uint32_t flush_slots(const uint8_t* ring, const OutDst& o, uint32_t& F, uint32_t upto, int lane) {
    uint32_t nsl = 0;
    while (upto - F >= XSLOT) {
        const uint32_t a0 = F + uint32_t(lane) * (XSLOT / 64);
        #pragma unroll
        for (uint32_t u = 0; u < XST; u++)
            put16(o, a0 + 16 * u, *reinterpret_cast<const u32x4*>(ring + ((a0 + 16 * u) & XRMASK)));
        F += XSLOT;
        nsl += XST;
    }
    return nsl;
}

// ---- wave64 DPP helpers (VALU-speed; __shfl goes through LDS) ----
__device__ __forceinline__ uint32_t dpp_incl_scan(uint32_t v) {
    v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false);   // row_bcast:15
    v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false);   // row_bcast:31
    return v;
}
__device__ __forceinline__ uint32_t dpp_prev(uint32_t v) {               // lane i <- lane i-1
    return __builtin_amdgcn_update_dpp(0u, v, 0x138, 0xf, 0xf, false);  // wave_shr:1
}

}  // namespace pf
