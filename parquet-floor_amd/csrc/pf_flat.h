// pf_flat.h — what more than one unit of the flat fast path uses (pf_flat_count.hip, pf_flat.hip,
// pf_flat_dstr.hip, pf_flat_null.hip): the tile sizes, the test for the dictionary-string pages the
// count stage takes, the fallback queue's append, the all-present validity fill and a 16-byte load that
// stays inside a section.
// Like pf_pages.h it defines no kernel and no __device__ variable.
#pragma once
#include "pf_pages.h"

namespace pf {

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

// Dictionary-string pages k_count_flat takes: flat, levels all present (k_runs), a run table.
__device__ __forceinline__ bool count_dict_page(const DevPage& pg, const DevChunk& ck, const Sections& s) {
    const IdRunTab* T = pg.runtab;
    return T != nullptr && T->all_present == 1u && T->nruns <= uint32_t(RUN_CAP) && T->covered >= uint32_t(pg.num_values) && ck.dict_len &&
           s.val_n > 0 && flat_block_chars(pg) != nullptr;
}

// Fallback queue (device, zeroed with the batch metadata): word 0 counts the (page, block) pairs that
// start at word 4; k_flat_null and k_flat_fixed append the blocks they do not take, the last workgroups of k_flat_all decode them.
__device__ __forceinline__ void null_fallback(int* fbq, int2 pbk) {
    if (threadIdx.x == 0) reinterpret_cast<int2*>(fbq + 4)[atomicAdd(fbq, 1)] = pbk;
}

// "All levels present": the chunk's validity bits [b0, b1), b0 < b1, set to one by the workgroup's NT threads.
// Whole words are stored; a word the range shares with a neighbouring block is or-ed into. The caller tests
// ck.max_def > 0 && ck.validity. Used by flat_fixed_block's direct branch and by k_flat_dstr; flat_present_fixed's
// tile loop (pf_flat.hip) spells the same loop out, because a call there changes k_flat_fixed's and k_flat_all's text.
__device__ __forceinline__ void fill_valid_ones(const DevChunk& ck, uint64_t b0, uint64_t b1) {
    uint32_t* vw = reinterpret_cast<uint32_t*>(ck.validity);
    for (uint64_t wd = (b0 >> 5) + threadIdx.x; wd <= ((b1 - 1) >> 5); wd += NT) {
        const uint64_t lo = max(b0, wd << 5), hi = min(b1, (wd + 1) << 5);
        const uint32_t m = uint32_t((hi - lo >= 32 ? 0xffffffffull : ((1ull << (hi - lo)) - 1ull)) << (lo & 31));
        if (lo == (wd << 5) && hi == ((wd + 1) << 5)) vw[wd] = m;
        else atomicOr(vw + wd, m);
    }
}

// The 16 bytes at the aligned address a; bytes outside [beg, end) are not read and give zero.
__device__ __forceinline__ u32x4 ld16_within(uintptr_t a, uintptr_t beg, uintptr_t end) {
    if (a >= beg && a + 16u <= end) return *reinterpret_cast<const PF_GLOBAL u32x4*>(a);
    uint32_t q[4] = {0, 0, 0, 0};
    #pragma unroll
    for (uint32_t b = 0; b < 16u; b++)
        if (a + b >= beg && a + b < end) q[b >> 2] |= uint32_t(*reinterpret_cast<const PF_GLOBAL uint8_t*>(a + b)) << (8 * (b & 3));
    return u32x4{q[0], q[1], q[2], q[3]};
}

}  // namespace pf
