// pf_flat.hip — the fast path for data pages of flat columns (max_rep == 0) on gfx950.
//
// Replaces, for the pages it takes, the per-value work parquet-mr 1.12.2 does behind ColumnReader
// (called from src/main/java/blue/strategic/parquet/ParquetReader.java:141-168): the hybrid
// expansion of definition levels and dictionary ids (RunLengthBitPackingHybridDecoder,
// DictionaryValuesReader), the dictionary gather (PlainValuesDictionary.decodeToX), the PLAIN
// fixed-width and BYTE_ARRAY readers, and the def == maxDef null test of ParquetReader.java:146.
// A page it does not take keeps done == 0 and is decoded by k_decode (pf_decode.hip).
//
// Kernels (pages are cut into blocks of FBLK entries, pf_page_tables.h). The count side runs first
// (pf_flat_count.hip: k_runs, k_count_dict, k_count_flat), then the levels of nullable pages
// (pf_flat_null.hip: k_lvl), then the flat stage, which launch_flat puts on the stream in this order:
//   k_flat_null<4|8>  (pf_flat_null.hip) per (page, block) with nulls, fixed width
//   k_flat_fixed   per (page, block), fixed width, all present; dictionary pages with a whole-page run table
//                  eight consecutive ids a thread (flat_fixed8, pf_fix_ids.h)
//   k_flat_dstr    (pf_flat_dstr.hip) per (page, block) of dictionary BYTE_ARRAY pages with a small
//                  dictionary of short values, all present
//   k_flat_all     per (page, block): every other flat page (BYTE_ARRAY, booleans, ...), and the
//                  fallback queue of blocks k_flat_null and k_flat_fixed did not take
#include <hip/hip_runtime.h>

#ifdef PF_DIAG
#include <cstdlib>   // getenv (PF_FIX8: diagnostics build only)
#endif

#include "pf_fix_ids.h"
#include "pf_flat.h"
#include "pf_flat_chars.h"
#include "pf_launch.h"
#include "pf_snappy_par.h"   // FB_WHOLE: what the Snappy executor wrote straight into the column

namespace pf {

// Phase stamps of the flat kernels in -DPF_STAMPS builds (tools/probe_flat_all.py): cycle sums per slot.
// A __device__ array belongs to one unit, so only this unit's kernels stamp (k_flat_fixed, k_flat_all);
// the nullable path has a table of its own (pf_nstamps, pf_flat_null.hip).
#ifdef PF_STAMPS
#include "pf_stamps.h"   // (a macro only: nothing of it lands in this namespace)
PF_STAMP_TABLE(pf_pstamps, 16, pf_debug_pstamps)
#define PSTAMP(i, v) atomicAdd(&pf_pstamps[i], (unsigned long long)(v))
#else
#define PSTAMP(i, v) ((void)0)
#endif

// ---- k_flat: data pages of flat columns (max_rep == 0) ------------------------------------------
// The same per-value work as k_decode, organised for throughput. The definition-level and
// dictionary-id run headers of the page are walked ONCE (one lane of wave 0 and one of wave 1,
// concurrently) into LDS run tables; tiles of FT entries then expand them by binary search with no
// serial section, one workgroup scan for the value index (none when the page has no nulls) and one
// for BYTE_ARRAY char offsets. BYTE_ARRAY chars are copied cooperatively, one 16-byte output chunk
// per thread step (coalesced stores), instead of a byte loop per value.
// Pages it does not take (run tables full, BIT_PACKED levels, RLE booleans, BYTE_STREAM_SPLIT,
// corrupt section layout) keep done == 0 and are decoded by k_decode.
struct FlatLds {
    uint32_t dpos[DSTR_CAP], dlen[DSTR_CAP];
    Run drun[RUN_CAP];
    Run vrun[RUN_CAP];
    uint32_t coff[FT];
    uint32_t csrc[FT];
    uint16_t cv[CV_CAP];
    uint32_t vbits[FT / 32 + 2];
    uint32_t scan_tmp[NT / 64];
    RunWalk dst, vst;
    int ndrun, nvrun, dres, vres, allp;
    uint32_t dcover, vcover, vlo;
};

// k_flat, all levels present, fixed-width values: value index = entry index, lane-consecutive
// entries so every load and store of a wave is one contiguous run of memory. Returns err.
#ifndef PF_DICT_LDS
#define PF_DICT_LDS 16384   // 16 KiB: 0.8 % faster SF1 step than 32 KiB (occupancy), 64 KiB 8 % slower (tools/gpu_ab_libs.sh)
#endif
constexpr uint32_t DICT_LDS = PF_DICT_LDS;   // bytes of a fixed-width dictionary staged in LDS (k_flat_fixed)
#ifndef PF_FIX_IDS
#define PF_FIX_IDS 0   // extra LDS bytes behind the dictionary for a block's ids (6144, which fits the date
                       // columns' 10 + 12 KB, costs a workgroup per CU: SF1 2.660-2.663 vs 2.632-2.655 ms)
#endif
struct FixedLds {
    uint64_t dict[(DICT_LDS + PF_FIX_IDS) / 8 + 2];   // the dictionary, then the block's id bytes when they fit
    Run vrun[RUN_CAP];
    uint32_t coff[FTX / 64];
    RunWalk vst;
    int nvrun, vres, allp;
    uint32_t vcover, vlo;
    uint32_t ib[2];                   // the block's id byte range [ib[0], ib[1])
};

template <class Lds>
__device__ __forceinline__ int flat_present_fixed(Lds& S, const DevChunk& ck, const DevPage& pg, const Sections& s, bool dict,
                                  bool boolean, int enc, int w, const uint8_t* ids, uint64_t ids_n, int id_bw,
                                  uint64_t slot_base, uint32_t e_begin, uint32_t e_end, bool direct = false) {
    const int tid = threadIdx.x;
    const uint8_t* vend = s.val + s.val_n;
    const bool dalign = dict && (reinterpret_cast<uintptr_t>(ck.dict_data) & uintptr_t(w - 1)) == 0;
    // dictionary gather from LDS when the whole dictionary fits (north_star: K3 LDS / global)
    const bool dlds = DICT_LDS > 0 && dict && dalign && (w == 4 || w == 8) && ck.dict_data != nullptr &&
                      ck.dict_n > 0 && uint64_t(ck.dict_n) * uint64_t(w) <= DICT_LDS;
    // The block's dictionary ids, when the run table covers the block and their bytes fit behind the
    // dictionary: staged in LDS with the dictionary's loads (round 5), so the tiles read ids from LDS
    // instead of issuing a round of id loads per tile batch. Page id byte k is staged byte k - idd.
    const uint32_t dbytes = dlds ? (uint32_t(ck.dict_n) * uint32_t(w) + 15u) & ~15u : 0u;
    uint8_t* const sid = reinterpret_cast<uint8_t*>(S.dict) + dbytes;
    int64_t idd = 0;
    bool ilds = false;
    if (dict && dalign && (w == 4 || w == 8) && id_bw > 0 && id_bw <= 32 && s.val_n > 0 && S.vres != 2 &&
        S.vlo <= e_begin && e_end <= S.vcover) {
        if (tid == 0) { S.ib[0] = 0xffffffffu; S.ib[1] = 0u; }
        __syncthreads();
        for (int r = tid; r < S.nvrun; r += NT) {
            const Run R = S.vrun[r];
            const uint32_t f = max(R.first, e_begin), l = min(R.first + R.count, e_end);
            if (!R.packed || f >= l) continue;
            atomicMin(&S.ib[0], uint32_t((uint64_t(R.data) + uint64_t(f - R.first) * uint64_t(id_bw)) >> 3));
            atomicMax(&S.ib[1], uint32_t((uint64_t(R.data) + uint64_t(l - R.first) * uint64_t(id_bw) + 7u) >> 3));
        }
        __syncthreads();
        const uint32_t lo = S.ib[0], hi = S.ib[1];
        if (lo < hi && hi <= ids_n) {
            const uintptr_t a0 = (reinterpret_cast<uintptr_t>(ids) + lo) & ~uintptr_t(15);
            const uintptr_t aend = reinterpret_cast<uintptr_t>(ids) + ids_n;     // readable source end
            const uint32_t nb = (uint32_t(reinterpret_cast<uintptr_t>(ids) + hi - a0) + 8u + 15u) & ~15u;
            if (dbytes + nb <= uint32_t(sizeof(S.dict))) {
                ilds = true;
                idd = int64_t(a0) - int64_t(reinterpret_cast<uintptr_t>(ids));
                for (uint32_t c = tid; c < nb / 16u; c += NT) {
                    const uintptr_t a = a0 + 16u * c;
                    u32x4 x;
                    if (a + 16u <= aend) {
                        x = *reinterpret_cast<const PF_GLOBAL u32x4*>(a);
                    } else {   // the section's last bytes: no read past it (ld16_within with no lower bound, spelled out: DESIGN §3)
                        uint32_t q[4] = {0, 0, 0, 0};
                        for (uint32_t b = 0; b < 16u && a + b < aend; b++)
                            q[b >> 2] |= uint32_t(*reinterpret_cast<const PF_GLOBAL uint8_t*>(a + b)) << (8 * (b & 3));
                        x = u32x4{q[0], q[1], q[2], q[3]};
                    }
                    reinterpret_cast<u32x4*>(sid)[c] = x;
                }
            }
        }
    }
    if (dlds) {   // eight loads a thread in flight per round (a 2,526-entry date dictionary: 2 rounds, not 10)
        const uint32_t dn = uint32_t(ck.dict_n);
        if (w == 8) {
            const PF_GLOBAL uint64_t* g = (const PF_GLOBAL uint64_t*)(ck.dict_data);
            for (uint32_t i0 = tid; i0 < dn; i0 += 8u * NT) {
                uint64_t v[8];
                #pragma unroll
                for (uint32_t k = 0; k < 8; k++) v[k] = i0 + k * NT < dn ? g[i0 + k * NT] : 0ull;
                #pragma unroll
                for (uint32_t k = 0; k < 8; k++) if (i0 + k * NT < dn) S.dict[i0 + k * NT] = v[k];
            }
        } else {
            const PF_GLOBAL uint32_t* g = (const PF_GLOBAL uint32_t*)(ck.dict_data);
            uint32_t* d32 = reinterpret_cast<uint32_t*>(S.dict);
            for (uint32_t i0 = tid; i0 < dn; i0 += 8u * NT) {
                uint32_t v[8];
                #pragma unroll
                for (uint32_t k = 0; k < 8; k++) v[k] = i0 + k * NT < dn ? g[i0 + k * NT] : 0u;
                #pragma unroll
                for (uint32_t k = 0; k < 8; k++) if (i0 + k * NT < dn) d32[i0 + k * NT] = v[k];
            }
        }
    }
    if (dlds || ilds) __syncthreads();
    for (uint32_t e0 = e_begin, want = 0; e0 < e_end; e0 += want) {
        want = min(uint32_t(FTX), e_end - e0);
        int bad = 0;
        if (dict) {
            if ((S.vlo > e0 || e0 + want > S.vcover) && S.vres == 2) {
                __syncthreads();
                if (tid < 64) {   // next window of runs (re-walk from the page start), wave 0
                    if (tid == 0) { S.vst = RunWalk{0, 0}; S.vlo = e0; }
                    const int rr = wave_walk_runs(ids, ids_n, id_bw, e0, e_end, S.vrun, RUN_CAP, S.nvrun, S.vcover, S.vst, RunWalk{0, 0});
                    if (tid == 0) S.vres = rr;
                }
                __syncthreads();
                // a tile whose ids need more runs than the table holds (runs shorter than FTX / RUN_CAP
                // values): this tile is the part the table covers, the next window starts after it
                if (S.vres == 2 && S.vcover > e0 && e0 + want > S.vcover) want = S.vcover - e0;
            }
            if (id_bw > 32 || s.val_n == 0 || ck.dict_data == nullptr || e0 + want > S.vcover || S.vlo > e0) bad = 1;
            if (!bad && uint32_t(tid) < (want + 63) / 64) S.coff[tid] = uint32_t(run_find(S.vrun, S.nvrun, e0 + tid * 64));
            __syncthreads();
        }
        const bool wide = w == 4 || w == 8;
        if (direct) {
            // the executor wrote this page's values into the column (k_snappy_head): validity only
        } else if (!bad && wide && ((dict && dalign) || enc == 0 || enc == 5)) {
            // batched: the loads of FB entries per thread are in flight together
#ifndef PF_FB_DIV
#define PF_FB_DIV 2
#endif
            constexpr uint32_t FB = FEPTX / PF_FB_DIV;   // entries per thread per load batch
            for (uint32_t kb = 0; kb < FEPTX; kb += FB) {
            uint64_t v[FB];
            uint32_t id[FB];
            #pragma unroll
            for (uint32_t k = 0; k < FB; k++) {
                const uint32_t e = e0 + (kb + k) * NT + uint32_t(tid);
                id[k] = 0;
                v[k] = 0;
                if (e >= e0 + want) continue;
                if (dict) {
                    int r = int(S.coff[(e - e0) >> 6]);
                    while (e >= S.vrun[r].first + S.vrun[r].count) r++;
                    const Run R = S.vrun[r];
                    id[k] = R.data;
                    if (R.packed) {
                        const uint64_t bit = uint64_t(R.data) + uint64_t(e - R.first) * uint64_t(id_bw);
                        if (ilds) {
                            const uint32_t rb = uint32_t(int64_t(bit) - 8 * idd);
                            const uint32_t* q = reinterpret_cast<const uint32_t*>(sid) + (rb >> 5);
                            const uint64_t x = (uint64_t(q[0]) | (uint64_t(q[1]) << 32)) >> (rb & 31u);
                            id[k] = uint32_t(x & (id_bw == 32 ? 0xffffffffull : ((1ull << id_bw) - 1ull)));
                        } else {
                            id[k] = (bit >> 3) + 12 <= ids_n ? bits_fast(ids + (bit >> 3), uint32_t(bit & 7), id_bw)
                                                             : bits_le(ids, ids_n, bit, id_bw);
                        }
                    }
                } else if (enc == 0) {
                    if ((uint64_t(e) + 1) * uint64_t(w) > s.val_n) { bad = 1; continue; }
                    const uint8_t* src = s.val + uint64_t(e) * uint64_t(w);
                    if (w == 8) v[k] = src + 12 <= vend ? gld_u64_12(src) : ld64_bytes(src);
                    else v[k] = src + 8 <= vend ? gld_u32_8(src) : ld32le(src, 0, 4);
                } else {
                    v[k] = reinterpret_cast<const uint64_t*>(pg.aux)[e];
                }
            }
            if (dict) {   // all FB gathers issued together (entries past the tile / bad ids load element 0)
                const int64_t dn = ck.dict_n;
                #pragma unroll
                for (uint32_t k = 0; k < FB; k++) {
                    const uint32_t e = e0 + (kb + k) * NT + uint32_t(tid);
                    if (e < e0 + want && int64_t(id[k]) >= dn) bad = 1;
                    id[k] = int64_t(id[k]) < dn ? id[k] : 0u;
                }
                if (dlds) {
                    #pragma unroll
                    for (uint32_t k = 0; k < FB; k++)
                        v[k] = w == 8 ? S.dict[id[k]] : reinterpret_cast<const uint32_t*>(S.dict)[id[k]];
                } else if (w == 8) {
                    const PF_GLOBAL uint64_t* g = (const PF_GLOBAL uint64_t*)ck.dict_data;
                    #pragma unroll
                    for (uint32_t k = 0; k < FB; k++) v[k] = g[id[k]];
                } else {
                    const PF_GLOBAL uint32_t* g = (const PF_GLOBAL uint32_t*)ck.dict_data;
                    #pragma unroll
                    for (uint32_t k = 0; k < FB; k++) v[k] = g[id[k]];
                }
            }
            #pragma unroll
            for (uint32_t k = 0; k < FB; k++) {
                const uint32_t e = e0 + (kb + k) * NT + uint32_t(tid);
                if (e >= e0 + want) continue;
                uint8_t* dst = ck.values + (slot_base + e) * uint64_t(w);
                if (w == 8) *reinterpret_cast<uint64_t*>(dst) = v[k];
                else *reinterpret_cast<uint32_t*>(dst) = uint32_t(v[k]);
            }
            }
        } else if (!bad) {
            #pragma unroll 2
            for (uint32_t k = 0; k < FEPTX; k++) {
                const uint32_t e = e0 + k * NT + uint32_t(tid);
                if (e >= e0 + want) break;
                uint8_t* dst = ck.values + (slot_base + e) * uint64_t(w);
                if (dict) {
                    int r = int(S.coff[(e - e0) >> 6]);
                    while (e >= S.vrun[r].first + S.vrun[r].count) r++;
                    const Run R = S.vrun[r];
                    uint32_t id = R.data;
                    if (R.packed) {
                        const uint64_t bit = uint64_t(R.data) + uint64_t(e - R.first) * uint64_t(id_bw);
                        id = (bit >> 3) + 12 <= ids_n ? bits_fast(ids + (bit >> 3), uint32_t(bit & 7), id_bw)
                                                      : bits_le(ids, ids_n, bit, id_bw);
                    }
                    if (int64_t(id) >= ck.dict_n) { bad = 1; continue; }
                    const uint8_t* src = ck.dict_data + uint64_t(id) * uint64_t(w);
                    if (w == 8 && dalign) *reinterpret_cast<uint64_t*>(dst) = *reinterpret_cast<const uint64_t*>(src);
                    else if (w == 4 && dalign) *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src);
                    else copy_value(dst, src, w);
                } else if (boolean) {
                    if ((e >> 3) >= s.val_n) { bad = 1; continue; }
                    dst[0] = uint8_t((s.val[e >> 3] >> (e & 7)) & 1u);
                } else if (enc == 0) {
                    if ((uint64_t(e) + 1) * uint64_t(w) > s.val_n) { bad = 1; continue; }
                    const uint8_t* src = s.val + uint64_t(e) * uint64_t(w);
                    if (w == 8 && src + 12 <= vend) *reinterpret_cast<uint64_t*>(dst) = gld_u64_12(src);
                    else if (w == 4 && src + 8 <= vend) *reinterpret_cast<uint32_t*>(dst) = gld_u32_8(src);
                    else copy_value(dst, src, w);
                } else {   // DELTA_BINARY_PACKED, decoded by k_delta into aux
                    const uint64_t* dv = reinterpret_cast<const uint64_t*>(pg.aux);
                    if (w == 8) *reinterpret_cast<uint64_t*>(dst) = dv[e];
                    else *reinterpret_cast<uint32_t*>(dst) = uint32_t(dv[e]);
                }
            }
        }
        // all present: the tile's validity bits are ones. fill_valid_ones (pf_flat.h) spelled out: as a call of it
        // here, k_flat_fixed is 5,563 instructions for 5,545 and k_flat_all 39,338 for 39,323 (registers unchanged)
        if (ck.max_def > 0 && ck.validity) {
            const uint64_t b0 = slot_base + e0, b1 = b0 + want;
            uint32_t* vw = reinterpret_cast<uint32_t*>(ck.validity);
            for (uint64_t wd = (b0 >> 5) + tid; wd <= ((b1 - 1) >> 5); wd += NT) {
                const uint64_t lo = max(b0, wd << 5), hi = min(b1, (wd + 1) << 5);
                const uint32_t m = uint32_t((hi - lo >= 32 ? 0xffffffffull : ((1ull << (hi - lo)) - 1ull)) << (lo & 31));
                if (lo == (wd << 5) && hi == ((wd + 1) << 5)) vw[wd] = m;
                else atomicOr(vw + wd, m);
            }
        }
        if (__syncthreads_or(bad)) return 1;
    }
    return 0;
}

// ---- k_flat_fixed's body for dictionary pages with a whole-page run table: eight ids a thread ----
// Thread t owns the 8-entry groups t + NT * k of the block (blocks start at multiples of FBLK, so groups are aligned
// from the page's entry 0). A group inside one run is one run lookup and one contiguous load of its id bytes
// (pf_fix_ids.h); the loads of FIX_GR groups a thread are issued together, the dictionary is staged behind them, and
// after the one barrier the ids are unpacked with constant shifts, gathered (LDS, or eight global loads in flight)
// and stored 16 bytes at a time. A group that straddles runs, the block's last partial group in a packed run, or a
// group whose words would reach outside the id section is decoded entry by entry as flat_present_fixed does.
#ifdef PF_DIAG   // diagnostics build: blocks this body decoded, groups it decoded entry by entry, blocks of dictionary
                 // pages k_flat_fixed gave to flat_present_fixed (tests)
__device__ unsigned long long pf_fix8_counts[3];
extern "C" int pf_debug_fix8_counts(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pf_fix8_counts), sizeof(unsigned long long) * 3) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[3] = {0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pf_fix8_counts), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#define FIX8_COUNT(i, n) ((void)atomicAdd(&pf_fix8_counts[i], (unsigned long long)(n)))
#else
#define FIX8_COUNT(i, n) ((void)0)
#endif

// bits_le (pf_device.h), spelled out: a call of it from this body changes k_flat_all's instruction text
__device__ __forceinline__ uint32_t fix_bits_pad(const uint8_t* p, uint64_t n, uint64_t bit, int w) {
    if (w == 0) return 0;
    const uint64_t by = bit >> 3;
    const int sh = int(bit & 7);
    uint64_t acc = 0;
    #pragma unroll
    for (int k = 0; k < 5; k++)
        if (8 * k < sh + w && by + k < n) acc |= uint64_t(p[by + k]) << (8 * k);
    return uint32_t((acc >> sh) & (w == 32 ? 0xffffffffull : ((1ull << w) - 1)));
}

constexpr uint32_t FIX_GR = 4;   // groups a thread holds the id words of at a time (a block of 8192 entries: all of them)

struct FixRowsLds {   // the block's run table (FixedLds::vrun) as pf_fix_ids.h reads rows
    const Run* r;
    __device__ __forceinline__ uint32_t first(uint32_t i) const { return r[i].first; }
    __device__ __forceinline__ uint32_t end(uint32_t i) const { return r[i].first + r[i].count; }
    __device__ __forceinline__ uint32_t packed(uint32_t i) const { return r[i].packed; }
    __device__ __forceinline__ uint32_t data(uint32_t i) const { return r[i].data; }
};
struct FixMemGlobal {   // the frame of aligned words around a page's id section
    const PF_GLOBAL uint8_t* base;
    __device__ __forceinline__ uint32_t operator()(uint32_t o) const { return *reinterpret_cast<const PF_GLOBAL uint32_t*>(base + o); }
};

// A thread's 8 consecutive values at p (aligned to the value): LEAD single values up to the 16-byte boundary, then
// 16-byte stores (store_offs16's pattern, pf_flat_dstr.hip).
template <int LEAD>
__device__ __forceinline__ void store_vals8(PF_GLOBAL uint32_t* p, const uint32_t (&v)[8]) {
    #pragma unroll
    for (int k = 0; k < LEAD; k++) p[k] = v[k];
    #pragma unroll
    for (int k = LEAD; k + 4 <= 8; k += 4) *reinterpret_cast<PF_GLOBAL u32x4*>(p + k) = u32x4{v[k], v[k + 1], v[k + 2], v[k + 3]};
    #pragma unroll
    for (int k = LEAD + (8 - LEAD) / 4 * 4; k < 8; k++) p[k] = v[k];
}
template <int LEAD>
__device__ __forceinline__ void store_vals8(PF_GLOBAL uint64_t* p, const uint64_t (&v)[8]) {
    #pragma unroll
    for (int k = 0; k < LEAD; k++) p[k] = v[k];
    #pragma unroll
    for (int k = LEAD; k + 2 <= 8; k += 2)
        *reinterpret_cast<PF_GLOBAL u32x4*>(p + k) = u32x4{uint32_t(v[k]), uint32_t(v[k] >> 32), uint32_t(v[k + 1]), uint32_t(v[k + 1] >> 32)};
    #pragma unroll
    for (int k = LEAD + (8 - LEAD) / 2 * 2; k < 8; k++) p[k] = v[k];
}

// The dictionary into LDS, eight loads a thread in flight per round (flat_present_fixed's loop)
template <class V>
__device__ __forceinline__ void fixed8_stage_dict(V* sd, const PF_GLOBAL V* gd, uint32_t dn) {
    for (uint32_t i0 = threadIdx.x; i0 < dn; i0 += 8u * NT) {
        V v[8];
        #pragma unroll
        for (uint32_t k = 0; k < 8; k++) v[k] = i0 + k * NT < dn ? gd[i0 + k * NT] : V(0);
        #pragma unroll
        for (uint32_t k = 0; k < 8; k++) if (i0 + k * NT < dn) sd[i0 + k * NT] = v[k];
    }
}

// The eight values of ids id[0 .. 8) from the dictionary (sd: its LDS copy, or null: gd), n of them stored at p
template <class V>
__device__ __forceinline__ void fixed8_gather_store(const V* sd, const PF_GLOBAL V* gd, const uint32_t (&id)[8], PF_GLOBAL V* p,
                                                    uint32_t n) {
    V v[8];
    if (sd != nullptr) {
        #pragma unroll
        for (uint32_t k = 0; k < 8; k++) v[k] = sd[id[k]];
    } else {
        #pragma unroll
        for (uint32_t k = 0; k < 8; k++) v[k] = gd[id[k]];
    }
    if (n == 8) {
        constexpr uint32_t per = 16u / sizeof(V);   // values per 16 bytes: 4 or 2
        const uint32_t lead = (per - uint32_t((reinterpret_cast<uintptr_t>(p) / sizeof(V)) & (per - 1u))) & (per - 1u);
        if constexpr (sizeof(V) == 4) {
            switch (lead) {
                case 0: store_vals8<0>(p, v); break;
                case 1: store_vals8<1>(p, v); break;
                case 2: store_vals8<2>(p, v); break;
                default: store_vals8<3>(p, v); break;
            }
        } else {
            if (lead == 0) store_vals8<0>(p, v);
            else store_vals8<1>(p, v);
        }
    } else {
        #pragma unroll
        for (uint32_t k = 0; k < 8; k++) if (k < n) p[k] = v[k];
    }
}

// w: 4 or 8. The run table covers the page (S.vrun, visible to all threads), the dictionary is aligned to w.
#ifndef PF_FIX8_GLOBAL
#define PF_FIX8_GLOBAL 0   // 1: the run lookup reads k_runs' table in global memory, not its LDS copy (SF1: no faster, §4.40)
#endif
__device__ __forceinline__ int flat_fixed8(FixedLds& S, const DevChunk& ck, [[maybe_unused]] const IdRunTab* T, int w_,
                                           const uint8_t* ids, uint64_t ids_n_, int id_bw_, uint64_t slot_base, uint32_t e_begin,
                                           uint32_t e_end) {
    const uint32_t tid = threadIdx.x;
    // the page's numbers are the same in every lane: kept in scalar registers (a section is under 4 GiB: body_len)
    const int w = __builtin_amdgcn_readfirstlane(w_), id_bw = __builtin_amdgcn_readfirstlane(id_bw_);
    const uint64_t ids_n = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(ids_n_))));
    const uint32_t dn = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(ck.dict_n))));
    const bool dlds = DICT_LDS > 0 && uint64_t(dn) * uint64_t(w) <= DICT_LDS;
    const uint32_t mis = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(reinterpret_cast<uintptr_t>(ids) & 3u))));
    const FixMemGlobal frame{(const PF_GLOBAL uint8_t*)(ids) - mis};
    const uint32_t nr = uint32_t(S.nvrun);
#if PF_FIX8_GLOBAL
    const FixRowsRt rows{T->rows, nr, S.vcover};
#else
    const FixRowsLds rows{S.vrun};
#endif
    int bad = 0;
    [[maybe_unused]] uint32_t nslow = 0;
    for (uint32_t eb = e_begin; eb < e_end; eb += FIX_GR * 8u * NT) {
        // ---- the run lookups and the id loads of this thread's groups, all issued before any is waited for
        uint32_t q[FIX_GR][FIX_NDW];   // a group's id words (FIX_CONST: q[.][0] is the id)
        uint32_t meta[FIX_GR];         // its kind << 8 | the bit of q[.][0] its first id starts at
        #pragma unroll
        for (uint32_t g = 0; g < FIX_GR; g++) {
            #pragma unroll
            for (int i = 0; i < FIX_NDW; i++) q[g][i] = 0;
            meta[g] = FIX_SLOW << 8;
            const uint32_t e0 = eb + 8u * (tid + NT * g);
            if (e0 < e_end) {
                const FixGrp G = fix_locate(rows, nr, e0, min(8u, e_end - e0), id_bw, mis, ids_n);
                if (G.kind == FIX_CONST) q[g][0] = G.val;
                else if (G.kind == FIX_PACKED) fix_load(id_bw, G.off4, frame, q[g]);
                meta[g] = (G.kind << 8) | (G.kind == FIX_PACKED ? G.val : 0u);
            }
        }
        // ---- the dictionary, behind the id loads and without waiting for them; the one barrier
        if (eb == e_begin && dlds) {
            if (w == 8) fixed8_stage_dict(S.dict, (const PF_GLOBAL uint64_t*)(ck.dict_data), dn);
            else fixed8_stage_dict(reinterpret_cast<uint32_t*>(S.dict), (const PF_GLOBAL uint32_t*)(ck.dict_data), dn);
            __syncthreads();
        }
        // ---- group by group: ids, gather, store. One text for the FIX_GR groups: the next group's words move down
        #pragma unroll 1
        for (uint32_t g = 0; g < FIX_GR; g++) {
            const uint32_t e0 = eb + 8u * (tid + NT * g);
            if (e0 < e_end) {
                const uint32_t n = min(8u, e_end - e0), kind = meta[0] >> 8;
                uint32_t id[8];
                if (kind == FIX_PACKED) {
                    fix_unpack(id_bw, q[0], meta[0] & 0xffu, id);
                } else if (kind == FIX_CONST) {
                    #pragma unroll
                    for (uint32_t k = 0; k < 8; k++) id[k] = q[0][0];
                } else {   // entry by entry, as flat_present_fixed
                    nslow++;
                    int r = run_find(S.vrun, S.nvrun, e0);
                    #pragma unroll
                    for (uint32_t k = 0; k < 8; k++) {
                        id[k] = 0;
                        if (k >= n) continue;
                        const uint32_t e = e0 + k;
                        while (e >= S.vrun[r].first + S.vrun[r].count) r++;
                        const Run R = S.vrun[r];
                        id[k] = R.data;
                        if (R.packed) {
                            const uint64_t bit = uint64_t(R.data) + uint64_t(e - R.first) * uint64_t(id_bw);
                            id[k] = (bit >> 3) + 12 <= ids_n ? bits_fast(ids + (bit >> 3), uint32_t(bit & 7), id_bw)
                                                             : fix_bits_pad(ids, ids_n, bit, id_bw);
                        }
                    }
                }
                #pragma unroll
                for (uint32_t k = 0; k < 8; k++) {   // (entries past the block / bad ids load element 0)
                    if (k < n && id[k] >= dn) bad = 1;
                    id[k] = id[k] < dn ? id[k] : 0u;
                }
                if (w == 8)
                    fixed8_gather_store<uint64_t>(dlds ? S.dict : nullptr, (const PF_GLOBAL uint64_t*)(ck.dict_data), id,
                                                  (PF_GLOBAL uint64_t*)(ck.values) + slot_base + e0, n);
                else
                    fixed8_gather_store<uint32_t>(dlds ? reinterpret_cast<const uint32_t*>(S.dict) : nullptr,
                                                  (const PF_GLOBAL uint32_t*)(ck.dict_data), id,
                                                  (PF_GLOBAL uint32_t*)(ck.values) + slot_base + e0, n);
            }
            #pragma unroll
            for (uint32_t h = 0; h + 1 < FIX_GR; h++) {
                meta[h] = meta[h + 1];
                #pragma unroll
                for (int i = 0; i < FIX_NDW; i++) q[h][i] = q[h + 1][i];
            }
        }
    }
    // all present: the block's validity bits are ones
    if (ck.max_def > 0 && ck.validity) fill_valid_ones(ck, slot_base + e_begin, slot_base + e_end);
#ifdef PF_DIAG
    if (nslow) FIX8_COUNT(1, nslow);
    if (tid == 0) FIX8_COUNT(0, 1);
#endif
    return __syncthreads_or(bad) ? 1 : 0;
}

// k_flat for fixed-width pages whose levels are all present (the common case), with a small LDS
// footprint and its own register budget: one workgroup per (page, FBLK block). Marks the page
// done; k_flat decodes everything else (strings, pages with nulls).
// Returns whether the block took its (page, block) (block-uniform); false: k_flat's body decodes it.
// MODE: 0 = k_flat_all's copy (flat_present_fixed for every block, the text it has always had), 1 = k_flat_fixed (the
// eight-a-thread body where it applies), 2 = the diagnostics build's k_flat_fixed under PF_FIX8=0 (as 0, counted).
template <int MODE>
__device__ __forceinline__ bool flat_fixed_block(FixedLds& S, const DevChunk* __restrict__ chunks, DevPage* pages, const int2 pbk,
                                 DevChunkResult* res) {
    if (pbk.x < 0) return true;   // padding of the XCD-grouped block list (runtime)
    // This head (pi / blk / bsz, the take rule, ids / ids_n / id_bw, tab) is flat_block's, line for line: each
    // of the four as a shared __forceinline__ helper changes both kernels' instruction text
    const int pi = pbk.x;
    const uint32_t blk = uint32_t(pbk.y) & 0x0fffffffu;
    const uint32_t bsz = FBLK << (uint32_t(pbk.y) >> 28);   // entries per block (runtime: wide blocks for no-null pages)
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    // the page's, chunk's and result's words are read in one round (bitwise ors: a short-circuit
    // chain puts a wait between each load)
    const int* jfb = pg.jfb;
    const bool dval = pg.direct == DIRECT_VALUES;
    const int jf = jfb != nullptr ? *jfb : FB_WHOLE + 1;
    const int done = pg.done;
    if (done & DONE_DSTR) return true;   // k_flat_dstr decoded the page
    if ((res[pg.chunk].status != 0) | (ck.max_rep != 0) | (ck.ptype == 6) | ((done & DONE_NULL) != 0)) return false;
    if (dval & (jf <= FB_WHOLE)) {
        // the executor wrote the values (k_snappy_head checked the levels): this block's validity bits
        const uint32_t ne = uint32_t(pg.num_values), e_begin = blk * bsz;
        if (e_begin >= ne && blk > 0) return true;
        const uint32_t e_end = min(ne, e_begin + bsz);
        if (ck.max_def > 0 && ck.validity && e_end > e_begin)
            fill_valid_ones(ck, uint64_t(pg.entry_start) + e_begin, uint64_t(pg.entry_start) + e_end);
        if (threadIdx.x == 0) {
            if (ck.needs_count == 0)
                atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values), (unsigned long long)(e_end - e_begin));
            atomicOr(&pg.done, DONE_FIXED);
        }
        return true;
    }
    Sections s;
    if (!page_sections(pg, ck, s)) return false;
    const int enc = pg.encoding;
    const bool boolean = ck.ptype == 0, dict = is_dict_enc(enc);
    const int w = ck.width;
    bool take = ck.max_def == 0 || s.def_rle;
    if (enc == 0) {
    } else if (dict) take = take && !boolean;
    else if (enc == 5) take = take && (ck.ptype == 1 || ck.ptype == 2) && pg.aux != nullptr;
    else take = false;
    if (!take) return false;
    const uint32_t ne = uint32_t(pg.num_values);
    if (blk > 0 && blk * bsz >= ne) return true;
    const int id_bw = (dict && s.val_n > 0) ? int(s.val[0]) : 0;
    const uint8_t* ids = dict && s.val_n > 0 ? s.val + 1 : s.val;
    const uint64_t ids_n = dict && s.val_n > 0 ? s.val_n - 1 : 0;
    const IdRunTab* T = pg.runtab;
    uint32_t t0 = 0, t3 = 0;
    if (T != nullptr) { t0 = T->nruns; t3 = T->all_present; }
    const bool tab = (t3 == 1u) & (t0 <= uint32_t(RUN_CAP));   // k_runs: levels all present
    if (tid == 0)
        S.allp = tab ? 1 : (ck.max_def == 0 ? 1 : all_present(s.def, s.def_n, bit_width(ck.max_def), ne, uint32_t(ck.max_def)));
    __syncthreads();
    if (!S.allp) return false;
    const uint32_t e_begin = blk * bsz;
    const uint32_t e_end = min(ne, e_begin + bsz);
#ifdef PF_STAMPS
    const unsigned long long ft0 = __builtin_amdgcn_s_memtime();
#endif
    if (dict) {
        if (tab) {
            const uint32_t nr = T->nruns, cov = T->covered;
            for (uint32_t i = tid; i < nr; i += NT) S.vrun[i] = id_run(T, i, nr, cov);
            if (tid == 0) { S.nvrun = int(nr); S.vcover = cov; S.vlo = 0; S.vres = cov >= ne ? 0 : 1; }
        } else if (tid < 64) {   // wave 0 walks the id runs of this block
            if (tid == 0) { S.nvrun = 0; S.vcover = 0; S.vres = 0; S.vlo = e_begin; S.vst = RunWalk{0, 0}; }
            if (s.val_n > 0 && id_bw <= 32) {
                const int rr = wave_walk_runs(ids, ids_n, id_bw, e_begin, e_end, S.vrun, RUN_CAP, S.nvrun, S.vcover, S.vst, RunWalk{0, 0});
                if (tid == 0) S.vres = rr;
            }
        }
        __syncthreads();
    }
    // values already in place: the executor decoded the page without falling back (a redo / serial
    // fallback writes the body to scratch instead, and the page is decoded from there)
    const bool direct = dval & (jf <= FB_WHOLE);
    int err;
    if constexpr (MODE == 1) {
        // the eight-a-thread body: a dictionary page of 4- or 8-byte values with an aligned dictionary, a run table
        // that covers the page, ids of at most FIX_BW_MAX bits. Everything else as before.
        const bool fix8 = dict && tab && !direct && (w == 4 || w == 8) && ck.dict_data != nullptr && ck.dict_n > 0 &&
                          (reinterpret_cast<uintptr_t>(ck.dict_data) & uintptr_t(w - 1)) == 0 && S.vres == 0 &&
                          id_bw <= FIX_BW_MAX && s.val_n > 0;
        if (fix8) {
            err = flat_fixed8(S, ck, T, w, ids, ids_n, id_bw, uint64_t(pg.entry_start), e_begin, e_end);
        } else {
            if (dict && tid == 0) FIX8_COUNT(2, 1);
            err = flat_present_fixed(S, ck, pg, s, dict, boolean, enc, w, ids, ids_n, id_bw,
                                     uint64_t(pg.entry_start), e_begin, e_end, direct);
        }
    } else {
        if constexpr (MODE == 2) { if (dict && tid == 0) FIX8_COUNT(2, 1); }
        err = flat_present_fixed(S, ck, pg, s, dict, boolean, enc, w, ids, ids_n, id_bw,
                                 uint64_t(pg.entry_start), e_begin, e_end, direct);
    }
#ifdef PF_STAMPS
    if (tid == 0) { const unsigned long long dt_ = __builtin_amdgcn_s_memtime() - ft0; PSTAMP(1, dt_); PSTAMP(0, 1); atomicMax(&pf_pstamps[9], dt_); }
#endif
    if (tid == 0) {
        if (err) set_status(res, pg.chunk, ST_CORRUPT, pi);
        else if (ck.needs_count == 0)
            atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values), (unsigned long long)(e_end - e_begin));
        atomicOr(&pg.done, DONE_FIXED);
    }
    return true;
}

// k_flat_fixed (round 5): the blocks of flat fixed-width pages, in a list of their own. Its register
// budget is the fixed-width body's (73 VGPRs, 21 KiB LDS: six workgroups per CU, against four of
// k_flat_all's 127-VGPR union of both bodies); blocks it does not take (a page with nulls that
// k_flat_null did not take, levels that are not RLE, ...) go to the fallback queue (k_flat_all's last workgroups).
#ifndef PF_FIXED_OCC
#define PF_FIXED_OCC 6
#endif
__global__ __launch_bounds__(NT, PF_FIXED_OCC) void k_flat_fixed(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                              const int2* __restrict__ blocks, DevChunkResult* res, int* fbq) {
    __shared__ FixedLds S;
    const int2 pbk = blocks[blockIdx.x];
    if (!flat_fixed_block<1>(S, chunks, pages, pbk, res)) null_fallback(fbq, pbk);
}
#ifdef PF_DIAG   // PF_FIX8=0 (diagnostics build): flat_present_fixed for every block, as before the eight-a-thread body
__global__ __launch_bounds__(NT, PF_FIXED_OCC) void k_flat_fixed_old(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                                  const int2* __restrict__ blocks, DevChunkResult* res, int* fbq) {
    __shared__ FixedLds S;
    const int2 pbk = blocks[blockIdx.x];
    if (!flat_fixed_block<2>(S, chunks, pages, pbk, res)) null_fallback(fbq, pbk);
}
#endif

// One workgroup per (page, FBLK block of entries). Pages whose levels are all present (max_def
// == 0 or RLE runs of max_def) are decoded block by block in parallel: value index = entry
// index, each block walks the dictionary-id run headers up to its own range (windowed when a
// block needs more than RUN_CAP runs) and takes its chars base from k_count's block table or,
// for PLAIN BYTE_ARRAY, from the value positions. Pages with nulls are decoded by block 0 alone.
__device__ __forceinline__ void flat_block(FlatLds& S, const DevChunk* __restrict__ chunks, DevPage* pages, const int2 pbk,
                           DevChunkResult* res) {
    if (pbk.x < 0) return;   // padding of the XCD-grouped block list (runtime)
    const int pi = pbk.x;
    const uint32_t blk = uint32_t(pbk.y) & 0x0fffffffu;
    const uint32_t bsz = FBLK << (uint32_t(pbk.y) >> 28);   // (wide blocks: fixed-width pages only)
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    // DONE_FIXED: k_flat_fixed took the page, DONE_DSTR: k_flat_dstr. Never test DONE_FLAT here: this kernel's own
    // blocks of the same page set it when they finish, and a block that starts later must still run.
    if ((res[pg.chunk].status != 0) | (ck.max_rep != 0) | ((pg.done & (DONE_FIXED | DONE_NULL | DONE_DSTR)) != 0)) return;
    Sections s;
    if (!page_sections(pg, ck, s)) return;                 // k_decode reports it
    const int enc = pg.encoding;
    const bool binary = ck.ptype == 6, boolean = ck.ptype == 0, dict = is_dict_enc(enc);
    const int w = ck.width;
    bool take = ck.max_def == 0 || s.def_rle;
    if (enc == 0) {
    } else if (dict) take = take && !boolean;
    else if (enc == 5) take = take && (ck.ptype == 1 || ck.ptype == 2) && pg.aux != nullptr;
    else take = false;
    if (!take) return;

    const int bwd = bit_width(ck.max_def);
    const uint32_t ne = uint32_t(pg.num_values);
    const int id_bw = (dict && s.val_n > 0) ? int(s.val[0]) : 0;
    const uint8_t* ids = dict && s.val_n > 0 ? s.val + 1 : s.val;
    const uint64_t ids_n = dict && s.val_n > 0 ? s.val_n - 1 : 0;
    const bool counted = ck.needs_count != 0;
    const uint64_t slot_base = uint64_t(pg.entry_start);   // flat: slot == entry
    if (blk > 0 && blk * bsz >= ne) return;
    const IdRunTab* T = pg.runtab;
    uint32_t t0 = 0, t3 = 0;
    if (T != nullptr) { t0 = T->nruns; t3 = T->all_present; }
    const bool tab = (t3 == 1u) & (t0 <= uint32_t(RUN_CAP));   // k_runs: levels all present
    if (tid == 0) S.allp = tab ? 1 : (ck.max_def == 0 ? 1 : all_present(s.def, s.def_n, bwd, ne, uint32_t(ck.max_def)));
    __syncthreads();
    const bool split = S.allp;
    if (!split && blk > 0) return;                          // block 0 decodes the whole page
    const uint32_t e_begin = split ? blk * bsz : 0u;
    const uint32_t e_end = split ? min(ne, e_begin + bsz) : ne;
#ifdef PF_STAMPS
    const unsigned long long ft0 = __builtin_amdgcn_s_memtime();
    if (tid == 0) { PSTAMP(0, 1); if (dict) PSTAMP(6, 1); if (binary) PSTAMP(7, 1); }
#endif
    if (tid < 64) {   // wave 0: definition-level runs (pages with nulls)
        if (tid == 0) { S.ndrun = 0; S.dcover = ne; S.dres = 0; S.dst = RunWalk{0, 0}; }
        if (!split && ck.max_def > 0) {
            const int rr = wave_walk_runs(s.def, s.def_n, bwd, 0, ne, S.drun, RUN_CAP, S.ndrun, S.dcover, S.dst, RunWalk{0, 0});
            if (tid == 0) S.dres = rr;
        }
    } else if (tid < 128 && !(split && tab)) {   // wave 1: dictionary-id runs
        if (tid == 64) { S.nvrun = 0; S.vcover = 0; S.vres = 0; S.vlo = e_begin; S.vst = RunWalk{0, 0}; }
        if (dict && s.val_n > 0 && id_bw <= 32) {
            const int rr = wave_walk_runs(ids, ids_n, id_bw, e_begin, split ? e_end : ne, S.vrun, RUN_CAP, S.nvrun,
                                          S.vcover, S.vst, RunWalk{0, 0});
            if (tid == 64) S.vres = rr;
        }
    }
    if (split && tab) {   // the page's run table (k_runs), loaded by all threads
        const uint32_t nr = T->nruns, cov = T->covered;
        for (uint32_t i = tid; i < nr; i += NT) S.vrun[i] = id_run(T, i, nr, cov);
        if (tid == 0) { S.nvrun = int(nr); S.vcover = cov; S.vlo = 0; S.vres = cov >= ne ? 0 : 1; }
    }
    // small string dictionaries: {pos, len} from LDS (visible after the tile loop's first barrier)
    const bool dstage = binary && dict && ck.dict_pos != nullptr && ck.dict_n > 0 && ck.dict_n <= int64_t(DSTR_CAP);
    if (dstage) {
        const PF_GLOBAL uint32_t* gp = gptr(ck.dict_pos);
        const PF_GLOBAL uint32_t* gl = gptr(ck.dict_len);
        for (uint32_t i = uint32_t(tid); i < uint32_t(ck.dict_n); i += NT) { S.dpos[i] = gp[i]; S.dlen[i] = gl[i]; }
    }
    __syncthreads();
#ifdef PF_STAMPS
    unsigned long long ft1 = __builtin_amdgcn_s_memtime();
    if (tid == 0) PSTAMP(2, ft1 - ft0);
#endif
    if (!split && (S.dres == 2 || S.vres == 2)) return;    // too many runs: k_decode takes the page
    bool allp = true, lvl_bad = S.dres != 0;
    if (!split) {
        for (int r = 0; r < S.ndrun; r++) {
            const Run& R = S.drun[r];
            if (R.packed || R.data != uint32_t(ck.max_def)) allp = false;
            if (!R.packed && R.data > uint32_t(ck.max_def)) lvl_bad = true;
        }
    }
    if (lvl_bad) {
        if (tid == 0) { set_status(res, pg.chunk, ST_CORRUPT, pi); atomicOr(&pg.done, DONE_FLAT); }
        return;
    }
    uint64_t char_base = 0;
    if (binary && counted) {
        char_base = uint64_t(pg.char_start);
        if (e_begin > 0) {
            if (dict) char_base += flat_block_chars(pg)[blk];
            else char_base += uint64_t(pg.aux[e_begin]) - 4ull * (uint64_t(e_begin) + 1);
        }
    }
    uint64_t vidx = e_begin;                                // page-relative index of the next present value
    int err = 0;
#ifdef PF_STAMPS   // tile sub-phases (tools/probe_flat_all.py): 11 levels, 12 values, 13 scan, 14 offsets, 15 chars
    unsigned long long fs_ = __builtin_amdgcn_s_memtime();
#define FSTAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (tid == 0) PSTAMP(i, t_ - fs_); fs_ = t_; } while (0)
#else
#define FSTAMP(i) ((void)0)
#endif


    for (uint32_t e0 = e_begin, want = 0; e0 < e_end; e0 += want) {
        want = min(uint32_t(FT), e_end - e0);
        if (split && dict && S.vres == 2 && (uint64_t(S.vlo) > uint64_t(e0) || e0 + want > S.vcover)) {
            // all levels present: value index = entry index. Next window of id runs before the levels,
            // and a tile needing more runs than the table holds shrinks to what it covers
            __syncthreads();
            if (tid < 64) {
                if (tid == 0) { S.vst = RunWalk{0, 0}; S.vlo = e0; }
                const int rr = wave_walk_runs(ids, ids_n, id_bw, e0, e_end, S.vrun, RUN_CAP, S.nvrun, S.vcover, S.vst,
                                              RunWalk{0, 0});
                if (tid == 0) S.vres = rr;
            }
            __syncthreads();
            if (S.vres == 2 && S.vcover > e0 && e0 + want > S.vcover) want = S.vcover - e0;
        }
        const uint32_t eb = uint32_t(tid) * FEPT;
        for (uint32_t i = tid; i < FT / 32 + 2; i += NT) S.vbits[i] = 0;
        // ---- definition levels -> present bits of this thread's entries
        uint32_t fv = 0;
        int bad = 0;
        if (eb < want) {
            const uint32_t m = min(uint32_t(FEPT), want - eb);
            if (allp) {
                fv = m >= 32 ? 0xffffffffu : (1u << m) - 1u;
            } else {
                const uint32_t e = e0 + eb;
                int r = run_find(S.drun, S.ndrun, e);
                for (uint32_t k = 0; k < m; k++) {
                    while (e + k >= S.drun[r].first + S.drun[r].count) r++;
                    const uint32_t d = run_value(S.drun[r], s.def, s.def_n, e + k, bwd);
                    bad |= d > uint32_t(ck.max_def);
                    fv |= uint32_t(d == uint32_t(ck.max_def)) << k;
                }
            }
        }
        uint32_t tv;
        uint32_t vo;
        if (allp) { vo = min(eb, want); tv = want; }
        else vo = block_excl_scan<NT>(__popc(fv), S.scan_tmp, tv);
        // ---- dictionary: this tile's values [vidx, vidx + tv) must be in the run table
        if (tv > 0 && dict) {
            if (split && (uint64_t(S.vlo) > vidx || vidx + tv > uint64_t(S.vcover)) && S.vres == 2) {
                __syncthreads();
                if (tid < 64) {   // next window of runs (re-walk from the page start), wave 0
                    if (tid == 0) { S.vst = RunWalk{0, 0}; S.vlo = uint32_t(vidx); }
                    const int rr = wave_walk_runs(ids, ids_n, id_bw, uint32_t(vidx), e_end, S.vrun, RUN_CAP, S.nvrun,
                                                  S.vcover, S.vst, RunWalk{0, 0});
                    if (tid == 0) S.vres = rr;
                }
                __syncthreads();
            }
            if (id_bw > 32 || s.val_n == 0 || (binary ? ck.dict_pos == nullptr : ck.dict_data == nullptr) ||
                vidx + tv > uint64_t(S.vcover) || uint64_t(S.vlo) > vidx)
                bad = 1;
        }
        if (__syncthreads_or(bad)) { err = 1; break; }
        FSTAMP(11);
        // ---- values
        uint32_t lsum = 0;
        uint32_t my_src[FEPT], my_len[FEPT];   // indexed by entry k (static after unrolling)
        {
            uint32_t j = 0;
            int vr = -1;
            #pragma unroll
            for (uint32_t k = 0; k < FEPT; k++) {
                my_src[k] = 0;
                my_len[k] = 0;
                if (eb + k >= want) continue;
                const uint64_t slot = slot_base + e0 + eb + k;
                const bool present = (fv >> k) & 1u;
                if (!binary) {
                    uint8_t* dst = ck.values + slot * uint64_t(w);
                    if (!present) { zero_value(dst, w); continue; }
                    const uint64_t gv = vidx + vo + j++;
                    if (dict) {
                        if (vr < 0) vr = run_find(S.vrun, S.nvrun, uint32_t(gv));
                        while (gv >= uint64_t(S.vrun[vr].first) + S.vrun[vr].count) vr++;
                        const uint32_t id = run_value(S.vrun[vr], ids, ids_n, uint32_t(gv), id_bw);
                        if (int64_t(id) >= ck.dict_n) { bad = 1; continue; }
                        copy_value(dst, ck.dict_data + uint64_t(id) * uint64_t(w), w);
                    } else if (boolean) {
                        if ((gv >> 3) >= s.val_n) { bad = 1; continue; }
                        dst[0] = uint8_t((s.val[gv >> 3] >> (gv & 7)) & 1u);
                    } else if (enc == 0) {
                        if ((gv + 1) * uint64_t(w) > s.val_n) { bad = 1; continue; }
                        copy_value(dst, s.val + gv * uint64_t(w), w);
                    } else {   // DELTA_BINARY_PACKED, decoded by k_delta into aux
                        const uint64_t* dv = reinterpret_cast<const uint64_t*>(pg.aux);
                        if (w == 8) *reinterpret_cast<uint64_t*>(dst) = dv[gv];
                        else *reinterpret_cast<uint32_t*>(dst) = uint32_t(dv[gv]);
                    }
                } else if (present) {
                    // strings: ids / positions of all FEPT entries first (their loads in flight
                    // together), the dictionary {pos, len} gathers in a second pass
                    const uint64_t gv = vidx + vo + j;
                    if (dict) {
                        if (vr < 0) vr = run_find(S.vrun, S.nvrun, uint32_t(gv));
                        while (gv >= uint64_t(S.vrun[vr].first) + S.vrun[vr].count) vr++;
                        const Run R = S.vrun[vr];
                        uint32_t id = R.data;
                        if (R.packed) {
                            const uint64_t bit = uint64_t(R.data) + uint64_t(uint32_t(gv) - R.first) * uint64_t(id_bw);
                            id = (bit >> 3) + 12 <= ids_n ? bits_fast(ids + (bit >> 3), uint32_t(bit & 7), id_bw)
                                                          : bits_le(ids, ids_n, bit, id_bw);
                        }
                        my_src[k] = id;
                        my_len[k] = 1;   // present (the length comes from the dictionary)
                    } else {   // PLAIN: value positions from the k_ba walk; a value's length is the
                               // distance to the next position (the walk checked the chain), the
                               // page's last value reads its length prefix
                        const PF_GLOBAL uint32_t* ax = gptr(pg.aux);
                        const uint32_t p = ax[gv];
                        uint32_t ln;
                        if (split && gv + 1 < uint64_t(ne)) {
                            const uint32_t nx = ax[gv + 1];
                            ln = nx >= p + 4 ? nx - p - 4 : 0xffffffffu;
                        } else {
                            ln = (p >= 4 && p <= s.val_n) ? ld32le(s.val, p - 4, s.val_n) : 0xffffffffu;
                        }
                        if (p >= 4 && p <= s.val_n && ln <= s.val_n - p) { my_src[k] = p; my_len[k] = ln; lsum += ln; }
                        else bad = 1;
                    }
                    j++;
                }
            }
            if (binary && dict) {
                const PF_GLOBAL uint32_t* gp = gptr(ck.dict_pos);
                const PF_GLOBAL uint32_t* gl = gptr(ck.dict_len);
                #pragma unroll
                for (uint32_t k = 0; k < FEPT; k++) {
                    if (!my_len[k]) continue;
                    const uint32_t id = my_src[k];
                    uint32_t src = 0, l = 0;
                    if (int64_t(id) >= ck.dict_n) bad = 1;
                    else if (dstage) { src = S.dpos[id]; l = S.dlen[id]; }
                    else { src = gp[id]; l = gl[id]; }
                    my_src[k] = src;
                    my_len[k] = l;
                    lsum += l;
                }
            }
        }
        FSTAMP(12);
        uint32_t tchars = 0;
        const uint32_t lo = binary ? block_excl_scan<NT>(lsum, S.scan_tmp, tchars) : 0;
        if (binary && char_base + tchars > uint64_t(pg.char_start + pg.n_chars)) bad = 1;   // k_count disagrees
        if (__syncthreads_or(bad)) { err = 1; break; }
        FSTAMP(13);
        if (binary) {
            uint32_t c = lo, j = 0;
            #pragma unroll
            for (uint32_t k = 0; k < FEPT; k++) {
                if (eb + k >= want) continue;
                if ((fv >> k) & 1u) {
                    S.coff[vo + j] = c;
                    S.csrc[vo + j] = my_src[k];
                    c += my_len[k];
                    j++;
                }
                ck.offsets[slot_base + e0 + eb + k + 1] = int32_t(char_base + c);
            }
        }
        // validity bits of this thread's entries
        if (ck.max_def > 0 && fv) {
            const uint64_t abase = (slot_base + e0) & ~uint64_t(31);
            const uint64_t rb = slot_base + e0 + eb - abase;
            const uint32_t sh = uint32_t(rb & 31);
            atomicOr(&S.vbits[rb >> 5], fv << sh);
            if (sh + FEPT > 32 && sh) atomicOr(&S.vbits[(rb >> 5) + 1], fv >> (32 - sh));
        }
        __syncthreads();
#ifdef PF_STAMPS
        { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (tid == 0) { PSTAMP(4, t_ - ft1); PSTAMP(3, 1); PSTAMP(14, t_ - fs_); } ft1 = t_; fs_ = t_; }
#endif
        if (binary) {
            const uint8_t* sb = dict ? ck.dict_data : s.val;
            const uint8_t* se = dict ? pages[ck.dict_page].body + pages[ck.dict_page].body_len : s.val + s.val_n;
            if (tchars <= SHORT_AVG * tv) copy_chars_short(S.coff, S.csrc, tv, tchars, sb, ck.chars + char_base);
            else if (!dict) copy_chars_plain(S.coff, S.csrc, tv, tchars, sb, se, ck.chars + char_base, S.cv);
            else copy_chars_fast(S.coff, S.csrc, tv, tchars, sb, se, ck.chars + char_base, S.cv);
        }
        FSTAMP(15);
        if (ck.max_def > 0 && ck.validity) flush_bits(S.vbits, slot_base + e0, want, ck.validity);
        vidx += tv;
        char_base += tchars;
        __syncthreads();
#ifdef PF_STAMPS
        { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (tid == 0) PSTAMP(5, t_ - ft1); ft1 = t_; }
#endif
    }
#ifdef PF_STAMPS
    if (tid == 0) {
        const unsigned long long dt_ = __builtin_amdgcn_s_memtime() - ft0;
        PSTAMP(1, dt_);
        atomicMax(&pf_pstamps[binary ? 8 : 9], dt_);
        if (!split) PSTAMP(10, 1);
    }
#endif
    if (tid == 0) {
        if (err) set_status(res, pg.chunk, ST_CORRUPT, pi);
        else if (!counted) atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values),
                                     (unsigned long long)(vidx - e_begin));
        atomicOr(&pg.done, DONE_FLAT);
    }
}

// k_flat_fixed and k_flat in one launch over the same (page, block) list: a block decodes its page
// with the fixed-width body when that applies, else with the general body. One stage instead of
// two in stream order (the fixed-width columns' blocks no longer wait for the string blocks or the
// other way round); the LDS of the two bodies is shared (they never run in one block together).
#ifndef PF_FLAT_OCC
#define PF_FLAT_OCC 5   // round 5 (with CV_CAP 2048 and the chars copies inlined): SF1 2.74 -> 2.69 ms; 4 before
#endif
// Workgroups n.. of the grid take the fallback queue (round 6: k_flat_fb's launch folded in; the producers
// of the queue, k_flat_fixed and k_flat_null, are earlier in stream order): a grid stride over the queued
// blocks, nearly always none.
__global__ __launch_bounds__(NT, PF_FLAT_OCC) void k_flat_all(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                 const int2* __restrict__ blocks, int n, const int* __restrict__ fbq,
                                                 DevChunkResult* res) {
    __shared__ union FlatAllLds {
        FixedLds f;
        FlatLds g;
    } S;
    if (int(blockIdx.x) >= n) {
        const int nq = fbq[0], g = int(gridDim.x) - n;
        for (int i = int(blockIdx.x) - n; i < nq; i += g) {
            const int2 pq = reinterpret_cast<const int2*>(fbq + 4)[i];
            if (!flat_fixed_block<0>(S.f, chunks, pages, pq, res)) {
                __syncthreads();
                flat_block(S.g, chunks, pages, pq, res);
            }
            __syncthreads();   // the block's LDS reads are done before the next one reuses it
        }
        return;
    }
    const int2 pbk = blocks[blockIdx.x];
    if (flat_fixed_block<0>(S.f, chunks, pages, pbk, res)) return;
    __syncthreads();   // the fixed body's LDS reads are done before the general body reuses it
    flat_block(S.g, chunks, pages, pbk, res);
}

// ---- launcher: the flat stage ------------------------------------------------------------------
void launch_flat(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int nfix, int n, int n4, int n8, int* d_fbq,
                 const int2* d_dblk, int n_dblk, DevChunkResult* d_res, hipStream_t st, NullCaps nc, int stagger) {
    // d_list: nfix (page, block) pairs of flat fixed-width pages (k_flat_fixed), then n of every other
    // flat page (k_flat_all), then n4 / n8 of nullable 4 / 8-byte pages (k_flat_null<4> / <8>; they mark
    // their pages DONE_NULL). Blocks k_flat_null and k_flat_fixed do not take are queued in d_fbq for
    // k_flat_all's last workgroups. nc: k_flat_null's LDS stages (dictionary: nc.dlds bytes); stagger (diagnostics build,
    // tests): k_flat_null's blocks > 0 of a page wait that many sleep rounds (~3 us each) for block 0
    // The stream order is k_flat_null<4>, <8>, k_flat_fixed, k_flat_dstr, k_flat_all: the first two and the
    // fourth through the launchers of the units that define them.
    const int2* blocks = reinterpret_cast<const int2*>(d_list);
    launch_flat_null(d_chunks, d_pages, blocks + nfix + n, n4, n8, d_fbq, d_res, st, nc, stagger);
#ifdef PF_DIAG
    // PF_FIX8=0: k_flat_fixed without the eight-a-thread body. Read here and not with the other PfOpts switches at
    // pf_ctx_create, because this launcher's signature is the runtime's; the product library has no such read.
    const char* fix8_env = std::getenv("PF_FIX8");
    if (nfix > 0 && fix8_env && fix8_env[0] == '0')
        hipLaunchKernelGGL(k_flat_fixed_old, dim3(nfix), dim3(NT), 0, st, d_chunks, d_pages, blocks, d_res, d_fbq);
    else
#endif
    if (nfix > 0) hipLaunchKernelGGL(k_flat_fixed, dim3(nfix), dim3(NT), 0, st, d_chunks, d_pages, blocks, d_res, d_fbq);
    // d_dblk: k_count_dict's (page, block) pairs, the blocks of flat dictionary BYTE_ARRAY pages: k_flat_dstr takes
    // the pages with a small dictionary of short values, k_flat_all's blocks of those then return at once
    launch_flat_dstr(d_chunks, d_pages, d_dblk, n_dblk, d_res, st);
    // k_flat_all last, with min(nq, 32) more workgroups for the fallback queue (nearly always empty; each
    // needs a CU with room for a k_flat_all workgroup: a grid of min(nq, 1024) waited ~0.1 ms under load,
    // and a launch of its own added one more wait per batch)
    const int nq = nfix + n4 + n8;
    const int nqw = nq < 32 ? nq : 32;
    if (n + nqw > 0)
        hipLaunchKernelGGL(k_flat_all, dim3(n + nqw), dim3(NT), 0, st, d_chunks, d_pages, blocks + nfix, n, d_fbq, d_res);
}

}  // namespace pf
