// pf_flat_null.hip — the flat fast path's nullable pages (fixed width 4 / 8, max_rep == 0).
//   k_lvl             per nullable fixed-width page: level run table and values before each block
//   k_flat_null<4|8>  per (page, block) with nulls: null scatter from k_lvl's tables; a block it does
//                     not take goes to the fallback queue (null_fallback, pf_flat.h) for k_flat_all
//   k_page_null       (diagnostics build, opt-in) k_lvl + k_flat_null for a whole page in one workgroup
// launch_lvl is the levels stage; launch_flat (pf_flat.hip) starts the flat stage with launch_flat_null.
#include <hip/hip_runtime.h>

#include "pf_flat.h"
#include "pf_launch.h"

namespace pf {

// Phase stamps of k_lvl and k_flat_null in -DPF_STAMPS builds (tools/probe_wide.py): this unit's own
// table, so a batch that also has all-present pages (pf_pstamps, pf_flat.hip) does not sum into its slots.
#ifdef PF_STAMPS
#include "pf_stamps.h"   // (a macro only: nothing of it lands in this namespace)
PF_STAMP_TABLE(pf_nstamps, 16, pf_debug_nstamps)
#define PSTAMP(i, v) atomicAdd(&pf_nstamps[i], (unsigned long long)(v))
#else
#define PSTAMP(i, v) ((void)0)
#endif

// ---- nullable flat pages: definition-level run table + block-parallel decode ------------------
//
// north_star K2/K6: "RLE/bit-packed-hybrid expansion of definition levels ... using prefix scans to
// find run boundaries" and null scatter. k_lvl walks a page's level run headers once (they are few:
// ~300 per 20,000 entries at 30 % random nulls), counts the present values of every run in parallel
// and scans them, so that every 4096-entry block of the page knows the value index of its first
// present entry. k_flat_null then decodes the blocks in parallel: levels -> present bits -> block
// scan -> value index -> dictionary gather / PLAIN load; null slots are zero.
constexpr uint32_t LVL_STAGE = 4096;   // level sections up to this size are decoded from LDS (k_lvl)

// Bits [bit, bit + k) (k <= 32) of an LDS byte array (LSB-first), from the two aligned dwords around it.
__device__ __forceinline__ uint32_t lds_bits(const uint8_t* st, uint32_t bit, uint32_t k) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(st);
    const uint32_t wi = bit >> 5, sh = bit & 31u;
    const uint64_t v = uint64_t(w[wi]) | (uint64_t(w[wi + 1]) << 32);
    return uint32_t(v >> sh) & (k >= 32 ? 0xffffffffu : ((1u << k) - 1u));
}

// Last level run with first entry <= e (runs: k_lvl's run rows, runs[0].first == 0).
__device__ __forceinline__ uint32_t lvl_run_at(const LvlRun* runs, uint32_t nr, uint32_t e) {
    return last_row_le(nr, e, [runs](uint32_t r) { return lvl_run(runs, r).first; });
}
// Present values before entry e, which lies in run r (its present-before count plus the present
// levels of the run before e, from the staged level section).
__device__ inline uint32_t lvl_values_before(const LvlRun* runs, uint32_t r, uint32_t e, const uint8_t* stage,
                                             uint32_t woff, int bw, uint32_t maxd) {
    const uint32_t first = lvl_run(runs, r).first, data = lvl_run(runs, r).data;
    const uint32_t before = e - first;
    uint32_t vb = lvl_run(runs, r).before;
    if (!lvl_run(runs, r).packed()) return vb + (data == maxd ? before : 0u);
    if (bw == 1) {
        for (uint32_t i = 0; i < before; i += 32) {
            const uint32_t k = min(32u, before - i), bb = woff * 8u + data + i;
            if (bb + k <= LVL_STAGE * 8u) vb += __popc(lds_bits(stage, bb, k));
        }
    } else {
        for (uint32_t i = 0; i < before; i++) {
            const uint32_t bb = woff * 8u + data + i * uint32_t(bw);
            if (bb + uint32_t(bw) <= LVL_STAGE * 8u) vb += lds_bits(stage, bb, uint32_t(bw)) == maxd;
        }
    }
    return vb;
}
// Dictionary-id run (k_runs table T) holding value v.
__device__ __forceinline__ uint32_t id_run_at(const IdRunTab* T, uint32_t nr, uint32_t v) {
    return last_row_le(nr, v, [T](uint32_t r) { return T->first(r); });
}

constexpr int LT_NT = 256;                // k_lvl: four waves per page
constexpr uint32_t LVL_RUNS_LDS = 512;    // level runs k_lvl keeps in LDS (pages with more read them from HBM)
constexpr uint32_t LVL_NXT = 4096;        // = LVL_STAGE: k_lvl's all-positions header tables cover its sections
constexpr uint32_t LVL_JUMP = 8;          // runs per step of k_lvl's chain walk (jump table: 3 doubling passes)
constexpr uint32_t LVL_S8 = LVL_NXT / LVL_JUMP;   // walk steps (a run is at least one byte)
constexpr uint32_t LVL_PPT = LVL_NXT / LT_NT;     // section positions per thread in the table passes
static_assert(LVL_PPT == 16, "k_lvl's mark words: two threads per 32 positions");
#ifndef PF_LVL_OCC
#define PF_LVL_OCC 1   // k_lvl workgroups per CU the register budget must allow (1: the compiler's choice, 114 VGPRs;
                       // 5: 96 VGPRs + 80 B scratch, config 4 3.70-3.75 vs 3.68-3.74 ms, not kept)
#endif
__global__ __launch_bounds__(LT_NT, PF_LVL_OCC) void k_lvl(const DevChunk* __restrict__ chunks, DevPage* pages, const int* __restrict__ list,
                                               DevChunkResult* res, uint32_t dcap, uint32_t icap) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[LVL_STAGE + 48];
    __shared__ uint32_t scan_tmp[LT_NT / 64];
    __shared__ uint32_t s_ns8;
    // next-header positions of every byte position (0xffff: not a header, or its run passes the
    // section end; dn: the chain ends there), then the page's dictionary-id runs (k_runs) for the
    // block table
    __shared__ union { uint16_t nxt[LVL_NXT]; IdRunTab T; } s_u;
    // the 8-run jump table during the chain walk, then the LDS copy of the level runs
    __shared__ union { uint16_t jmp[LVL_NXT]; LvlRun runs[LVL_RUNS_LDS]; } s_a;
    __shared__ uint16_t s_s8[LVL_S8];         // chain positions of runs 0, 8, 16, ...
    __shared__ uint32_t s_mark[LVL_NXT / 32];  // chain positions (run headers)
    static_assert(sizeof(uint16_t) * LVL_NXT >= sizeof(IdRunTab), "s_u sized by the header table");
    uint16_t* const s_nxt = s_u.nxt;
    IdRunTab* const s_T = &s_u.T;
    uint16_t* const s_jmp = s_a.jmp;
    LvlRun* const s_runs = s_a.runs;
    const int pi = list[blockIdx.x];
    DevPage& pg = pages[pi];
    LvlHead* LT = pg.lvltab;
    if (!LT) return;
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    Sections s;
    if (pg.done & DONE_PAGE) {   // k_page_null decoded the page
        if (tid == 0) LT->fit = 0;
        return;
    }
    if (res[pg.chunk].status != 0 || ck.max_rep != 0 || ck.max_def <= 0 || !page_sections(pg, ck, s) || !s.def_rle ||
        s.def_n > LVL_STAGE) {   // (longer level sections: k_flat / k_decode)
        if (tid == 0) LT->fit = 0;
        return;
    }
    const uint32_t ne = uint32_t(pg.num_values);
    const int bw = bit_width(uint32_t(ck.max_def));
    const uint32_t maxd = uint32_t(ck.max_def);
    const uint32_t dn = uint32_t(s.def_n);
#ifdef PF_STAMPS   // phase cycles per page (tools/probe_wide.py): 8 pages, 9 stage, 10 header table, 11 chain,
                   // 12 run decode, 13 present counts, 14 block table, 15 total; 6 runs, 7 level bytes
    unsigned long long lt_ = __builtin_amdgcn_s_memtime(), lt0_ = lt_;
#define LTS(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (tid == 0) PSTAMP(i, t_ - lt_); lt_ = t_; } while (0)
    if (tid == 0) { PSTAMP(8, 1); PSTAMP(7, dn); }
#else
#define LTS(i) ((void)0)
#endif
    // stage the level section with aligned 16-byte loads: section byte i is stage[woff + i]; bytes
    // past the section read as zero (parquet-mr zero-pads a truncated bit-packed run)
    const uintptr_t sa = reinterpret_cast<uintptr_t>(s.def);
    const uint32_t woff = uint32_t(sa & 15u);
    if (woff + dn > LVL_STAGE) {
        if (tid == 0) LT->fit = 0;
        return;
    }
    {
        const PF_GLOBAL u32x4* src = (const PF_GLOBAL u32x4*)(sa - woff);
        const uint32_t nchunk = (woff + dn + 15u) / 16u;
        for (uint32_t c = tid; c < nchunk; c += LT_NT) reinterpret_cast<u32x4*>(stage)[c] = src[c];
        if (uint32_t(tid) < LVL_NXT / 32) s_mark[tid] = 0;
        __syncthreads();
        for (uint32_t i = woff + dn + uint32_t(tid); i < nchunk * 16u + 16u; i += LT_NT) stage[i] = 0;
        __syncthreads();
    }
    LTS(9);
    LvlRun* runs = lvl_runs(LT);
    const uint32_t cap = pg.lvl_cap;
    const uint8_t* const stw = stage + woff;
    // (1) every byte position decoded as a run header: the position of the next header
    for (uint32_t p = tid; p < dn; p += LT_NT) {
        uint32_t h = 0, hl = 0, nx = 0xffffu;
        #pragma unroll
        for (uint32_t k = 0; k < 3; k++) {   // headers over 2^21 are no runs of a <= 4 KiB section
            const uint32_t c = p + k < dn ? uint32_t(stw[p + k]) : 0x80u;
            h |= (c & 0x7fu) << (7 * k);
            if (!(c & 0x80u)) { hl = k + 1; break; }
        }
        if (hl) {
            const uint32_t pay = (h & 1u) ? (h >> 1) * uint32_t(bw) : (uint32_t(bw) + 7u) >> 3;
            if (p + hl + pay <= dn) nx = p + hl + pay;   // a truncated run ends the chain
        }
        s_nxt[p] = uint16_t(nx);
    }
    __syncthreads();
    LTS(10);
    // (2) the chain from position 0 (north_star K2: run boundaries by wavefront passes). The 8-run jump
    // table by three doubling passes, one thread walks it eight runs a step, then one thread per
    // 8-run stretch walks the runs in between and marks their headers. Terminal values stay put:
    // 0xffff (broken chain) and positions >= dn (the section end).
    {
        uint32_t J[LVL_PPT];
        #pragma unroll
        for (uint32_t k = 0; k < LVL_PPT; k++) {
            const uint32_t p = uint32_t(tid) + k * LT_NT;
            const uint32_t q = p < dn ? uint32_t(s_nxt[p]) : 0xffffu;
            J[k] = q < dn ? uint32_t(s_nxt[q]) : q;
        }
        #pragma unroll
        for (uint32_t k = 0; k < LVL_PPT; k++) s_jmp[uint32_t(tid) + k * LT_NT] = uint16_t(J[k]);
        __syncthreads();
        for (int pass = 0; pass < 2; pass++) {   // 2 -> 4 -> 8 runs
            #pragma unroll
            for (uint32_t k = 0; k < LVL_PPT; k++) J[k] = J[k] < dn ? uint32_t(s_jmp[J[k]]) : J[k];
            __syncthreads();
            #pragma unroll
            for (uint32_t k = 0; k < LVL_PPT; k++) s_jmp[uint32_t(tid) + k * LT_NT] = uint16_t(J[k]);
            __syncthreads();
        }
    }
    if (tid == 0) {
        uint32_t p = 0, k = 0;
        while (p < dn && k < LVL_S8) {
            s_s8[k++] = uint16_t(p);
            const uint32_t q = s_jmp[p];
            if (q >= dn) break;   // the chain ends (or breaks) within the next 8 runs
            p = q;
        }
        s_ns8 = k;
    }
    __syncthreads();
    const uint32_t ns8 = s_ns8;
    for (uint32_t j = tid; j < ns8; j += LT_NT) {
        uint32_t p = s_s8[j];
        for (uint32_t i = 0; i < LVL_JUMP && p < dn; i++) {
            const uint32_t q = s_nxt[p];
            if (q == 0xffffu) break;   // no run header here: the chain is broken
            atomicOr(&s_mark[p >> 5], 1u << (p & 31u));
            p = q;
        }
    }
    __syncthreads();
    LTS(11);
    // (3) the marked headers in position order: runs decoded at their headers in parallel, their
    // first entries an exclusive scan of the counts, runs with entries at or past the page's dropped
    const uint32_t mw = s_mark[tid >> 1];   // a thread's 16 positions: half a mark word
    const uint32_t mbits = (mw >> (16u * (uint32_t(tid) & 1u))) & 0xffffu;
    const uint32_t p0 = 16u * uint32_t(tid);
    uint32_t hcnt[LVL_PPT], hdat[LVL_PPT], hpk = 0;
    uint64_t csum = 0;
    #pragma unroll
    for (uint32_t k = 0; k < LVL_PPT; k++) {
        hcnt[k] = 0;
        hdat[k] = 0;
        if (!((mbits >> k) & 1u)) continue;
        const uint32_t P = p0 + k;
        uint32_t h = 0, hl = 0;
        for (uint32_t b = 0; b < 3; b++) {
            const uint32_t c = stw[P + b];
            h |= (c & 0x7fu) << (7 * b);
            if (!(c & 0x80u)) { hl = b + 1; break; }
        }
        const uint32_t packed = h & 1u;
        hcnt[k] = packed ? (h >> 1) * 8u : (h >> 1);
        if (packed) hdat[k] = (P + hl) * 8u;
        else for (uint32_t b = 0; b < ((uint32_t(bw) + 7u) >> 3); b++) hdat[k] |= uint32_t(stw[P + hl + b]) << (8 * b);
        hpk |= packed << k;
        csum += hcnt[k];
    }
    __shared__ unsigned long long scan64[LT_NT / 64];
    uint64_t ctot;
    const uint64_t cbase = block_excl_scan64<LT_NT>(csum, scan64, ctot);
    uint32_t emask = 0, bad = 0;
    {
        uint64_t f = cbase;
        #pragma unroll
        for (uint32_t k = 0; k < LVL_PPT; k++) {
            if (hcnt[k] > 0 && f < ne) {
                emask |= 1u << k;
                if (!((hpk >> k) & 1u) && hdat[k] > maxd) bad = 1;
            }
            f += hcnt[k];
        }
    }
    __syncthreads();   // scan_tmp is reused
    uint32_t nr;
    const uint32_t rbase = block_excl_scan<LT_NT>(__popc(emask), scan_tmp, nr);
    {
        uint64_t f = cbase;
        uint32_t rank = rbase;
        #pragma unroll
        for (uint32_t k = 0; k < LVL_PPT; k++) {
            if ((emask >> k) & 1u && nr <= cap) {   // (emitted: f < ne)
                const uint32_t c = uint32_t(min<uint64_t>(hcnt[k], uint64_t(ne) - f));
                const uint32_t cw = c | (((hpk >> k) & 1u) << 31);
                lvl_run(runs, rank).first = uint32_t(f);
                lvl_run(runs, rank).data = hdat[k];
                lvl_run(runs, rank).cw = cw;
                if (rank < LVL_RUNS_LDS) {
                    lvl_run(s_runs, rank).first = uint32_t(f);
                    lvl_run(s_runs, rank).data = hdat[k];
                    lvl_run(s_runs, rank).cw = cw;
                }
                rank++;
            }
            f += hcnt[k];
        }
    }
    __threadfence_block();   // the run records (HBM and LDS) before the other waves read them
    const bool ok = __syncthreads_or(bad) == 0 && nr <= cap && ctot >= ne;   // (a broken chain covers too few)
    LTS(12);
    if (!ok) {
        if (tid == 0) LT->fit = 0;
        return;
    }
    LvlRun* const R = nr <= LVL_RUNS_LDS ? s_runs : runs;   // the scans below read this copy
    uint32_t carry = 0;
    for (uint32_t r0 = 0; r0 < nr; r0 += LT_NT) {
        const uint32_t r = r0 + uint32_t(tid);
        uint32_t pc = 0;
        if (r < nr) {
            const uint32_t data = lvl_run(R, r).data, cnt = lvl_run(R, r).count();
            if (!lvl_run(R, r).packed()) pc = data == maxd ? cnt : 0u;
            else {
                // packed levels [data, data + cnt * bw) bits (the stage is zero past the section)
                const uint32_t nbits = cnt * uint32_t(bw);
                const uint32_t b0 = woff * 8u + data;
                if (bw == 1) {
                    for (uint32_t i = 0; i < nbits; i += 32) {
                        const uint32_t k = min(32u, nbits - i);
                        if (b0 + i + k <= LVL_STAGE * 8u) pc += __popc(lds_bits(stage, b0 + i, k));
                    }
                } else {
                    for (uint32_t i = 0; i < cnt; i++) {
                        const uint32_t b = b0 + i * uint32_t(bw);
                        if (b + uint32_t(bw) <= LVL_STAGE * 8u) pc += lds_bits(stage, b, uint32_t(bw)) == maxd;
                    }
                }
            }
        }
        uint32_t tot;
        const uint32_t ex = block_excl_scan<LT_NT>(pc, scan_tmp, tot);
        if (r < nr) {
            lvl_run(runs, r).before = carry + ex;
            if (R != runs) lvl_run(R, r).before = carry + ex;
        }
        carry += tot;
        __syncthreads();   // scan_tmp is reused
    }
    LTS(13);
    // per FBLK block (k_flat_null): the runs it overlaps [r0, r1), the value indices of its first and
    // end entries, the level bytes its packed runs read and the dictionary-id bytes of its values
    __threadfence_block();
    const uint32_t nblk = (ne + FBLK - 1) / FBLK;
    // dictionary id runs (k_runs, same stream): value index -> bit offset in the id stream
    const IdRunTab* TG = pg.runtab;
    const bool dict = is_dict_enc(pg.encoding) && TG != nullptr && TG->valid == 1u && TG->nruns <= uint32_t(RUN_CAP) && s.val_n > 0;
    const uint32_t tnr = dict ? TG->nruns : 0u, tcov = dict ? TG->covered : 0u;
    if (dict)
        for (uint32_t i = tid; i < id_tab_words(tnr); i += LT_NT)
            reinterpret_cast<uint32_t*>(s_T)[i] = reinterpret_cast<const uint32_t*>(TG)[i];
    __syncthreads();
    const IdRunTab* T = s_T;
    const uint32_t id_bw = dict ? uint32_t(s.val[0]) : 0u;
    uint32_t fit = 1;
    for (uint32_t b = tid; b < nblk; b += LT_NT) {
        const uint32_t eb = b * FBLK, ee = min(ne, eb + FBLK);
        const uint32_t lo = lvl_run_at(R, nr, eb);
        uint32_t a = lo, z = nr;    // first run with first >= ee
        while (a < z) {
            const uint32_t m = (a + z) >> 1;
            if (lvl_run(R, m).first < ee) a = m + 1; else z = m;
        }
        const uint32_t vb = lvl_values_before(R, lo, eb, stage, woff, bw, maxd);
        const uint32_t ve = ee == ne ? carry : lvl_values_before(R, lvl_run_at(R, nr, ee), ee, stage, woff, bw, maxd);
        // level bytes: from the first packed run's first bit to the last packed run's end
        uint32_t d0 = 0, d1 = 0;
        for (uint32_t r = lo; r < a; r++) {
            if (!lvl_run(R, r).packed()) continue;
            const uint32_t f = lvl_run(R, r).first;
            d0 = (lvl_run(R, r).data + (max(eb, f) - f) * uint32_t(bw)) >> 3;
            break;
        }
        for (uint32_t r = a; r > lo; r--) {
            if (!lvl_run(R, r - 1).packed()) continue;
            const uint32_t f = lvl_run(R, r - 1).first, end = min(ee, f + lvl_run(R, r - 1).count());
            d1 = (lvl_run(R, r - 1).data + (end - f) * uint32_t(bw) + 7u) >> 3;
            break;
        }
        // dictionary-id bytes of values [vb, ve)
        uint32_t i0 = 0, i1 = 0;
        if (dict && ve > vb) {
            if (ve > tcov) fit = 0;
            else {
                const uint32_t q0 = id_run_at(T, tnr, vb), q1 = id_run_at(T, tnr, ve - 1);
                for (uint32_t q = q0; q <= q1; q++) {
                    if (!T->packed(q)) continue;
                    const uint32_t f = T->first(q);
                    i0 = uint32_t((uint64_t(T->data(q)) + uint64_t(max(vb, f) - f) * id_bw) >> 3);
                    break;
                }
                for (uint32_t q = q1 + 1; q > q0; q--) {
                    if (!T->packed(q - 1)) continue;
                    const uint32_t f = T->first(q - 1);
                    const uint32_t nf = q < tnr ? T->first(q) : tcov;
                    i1 = uint32_t((uint64_t(T->data(q - 1)) + uint64_t(min(ve, nf) - f) * id_bw + 7u) >> 3);
                    break;
                }
            }
        }
        if (a - lo > LT_BLOCK_RUNS || d1 - d0 + 16u > dcap || i1 - i0 + 16u > icap || ve < vb) fit = 0;
        *lvl_block(LT, cap, b) = LvlBlock{lo, a, vb, ve, d0, d1, i0, i1};
    }
    fit = __syncthreads_and(fit) ? 1u : 0u;
    if (tid == 0) { LT->nruns = nr; LT->present = carry; LT->fit = fit; }
    LTS(14);
#ifdef PF_STAMPS
    if (tid == 0) PSTAMP(15, __builtin_amdgcn_s_memtime() - lt0_);
    if (tid == 0) PSTAMP(6, nr);
#endif
#undef LTS
}

// k_flat_null<W>: one 256-thread workgroup per 4096-entry block of a nullable W-byte page, 16
// consecutive entries per thread. The block's level runs, the page's id runs and the level / id bytes
// the block reads (k_lvl's block table) are all fetched at once into LDS, so the workgroup waits on one
// round of loads, then on the dictionary gather; no spread step: entry k of a thread takes the value of
// rank popc(fv & (2^k - 1)). The stage is latency-bound (Σ block latency / resident blocks), so what
// sets it is the entries in flight per CU: 16 per lane (round 5; 8 per lane at 512 threads: config 4's
// flat launch 0.97 -> 0.81 ms, gpurun_out/ntn). The runtime gives the kernel only nullable pages of its
// width (its own block lists); a page it does not take goes to the fallback queue (k_flat_all's last workgroups).
#ifndef PF_NTN
#define PF_NTN 256
#endif
constexpr int NTN = PF_NTN;
constexpr int NEPT = FBLK / NTN;   // 8 (512 threads) or 16 (256)
static_assert(NEPT % 4 == 0 && NEPT <= 16, "k_flat_null's stores and present masks");
// Runs in LDS as {first | packed << 31, data}: a run ends where the next begins (k_lvl's level runs
// and k_runs' id runs are contiguous), and one sentinel row after the last holds its end.
struct NullLds {
    uint2 drun[LT_BLOCK_RUNS + 1];
    uint2 vrun[RUN_CAP + 1];
    uint32_t vbits[FBLK / 32 + 2];
    uint32_t scan_tmp[NTN / 64];
};
__device__ __forceinline__ uint32_t rl_first(uint2 r) { return r.x & 0x7fffffffu; }
__device__ __forceinline__ int rl_find(const uint2* runs, int nr, uint32_t i) {   // run holding i (runs[0] first <= i)
    return last_row_le(nr, i, [runs](int r) { return rl_first(runs[r]); });
}

// Dynamic LDS, sized by the host per batch (NullCaps): the block's level bytes (dcap + 32), its
// dictionary-id bytes (icap + 32) -- caps from the batch's level and id bit widths, which k_lvl's
// block table was checked against -- and dictionaries of at most dlds bytes (the batch's largest
// fitting one, <= NULL_DICT_LDS; 0 when it has none), gathered from LDS (north_star K3: "dictionary
// staged in LDS when it fits"); larger ones are gathered from L2 / HBM. Config 4 (1-bit levels,
// 17-bit ids): ~16.6 KiB a workgroup, eight resident per CU (the VGPR limit) instead of five.

template <int W> struct WidthType { using type = uint64_t; };
template <> struct WidthType<4> { using type = uint32_t; };

template <int W>
__global__ __launch_bounds__(NTN) void k_flat_null(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                   const int2* __restrict__ blocks, DevChunkResult* res, NullCaps nc,
                                                   int stagger, int* fbq) {
    using VT = typename WidthType<W>::type;
    __shared__ __attribute__((aligned(16))) NullLds S;
    extern __shared__ __attribute__((aligned(16))) uint64_t DYN[];
    uint32_t* const s_dst = reinterpret_cast<uint32_t*>(DYN);
    uint32_t* const s_ist = s_dst + (nc.dcap + 32u) / 4u;
    uint64_t* const DL = reinterpret_cast<uint64_t*>(s_ist + (nc.icap + 32u) / 4u);
    const uint32_t dlds = nc.dlds;
    const int2 pbk = blocks[blockIdx.x];
#ifdef PF_DIAG   // diagnostics build (tests): blocks after a page's first start late, after it has finished
    if (stagger && pbk.y > 0)
        for (int i = 0; i < stagger; i++) __builtin_amdgcn_s_sleep(127);
#else
    (void)stagger;
#endif
    if (pbk.x < 0) return;   // padding of the XCD-grouped block list (runtime)
#ifdef PF_STAMPS   // phase cycles per block: 0 blocks, 1 tables, 2 LDS stage, 3 levels + scan, 4 gather + store
    unsigned long long t_ph = __builtin_amdgcn_s_memtime(), t_beg = t_ph;
#define NSTAMP(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (threadIdx.x == 0) PSTAMP(i, t_ - t_ph); t_ph = t_; }
#else
#define NSTAMP(i) ((void)0)
#endif
    const int pi = pbk.x;
    const uint32_t blk = uint32_t(pbk.y) & 0x0fffffffu;   // (pages with a level table always have FBLK blocks)
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    LvlHead* const LT = pg.lvltab;
    // pages this kernel does not take (whole pages: the conditions are the page's) go to the fallback queue
    // (not DONE_NULL: blocks of this page that finished first set it, and a block starting later must still run)
    if (!LT || res[pg.chunk].status != 0 || ck.max_rep != 0 || ck.width != W ||
        (pg.done & (DONE_FIXED | DONE_PAGE)) || LT->fit != 1u) {   // (k_page_null took it, or no block table)
        null_fallback(fbq, pbk);
        return;
    }
    Sections s;
    const int enc = pg.encoding;
    const bool dict = is_dict_enc(enc);
    const IdRunTab* T = pg.runtab;
    if (!page_sections(pg, ck, s) || (!dict && enc != 0) ||
        (dict && !(T != nullptr && T->valid == 1u && T->nruns <= uint32_t(RUN_CAP) && s.val_n > 0 && ck.dict_data != nullptr))) {
        null_fallback(fbq, pbk);
        return;
    }
    const uint32_t ne = uint32_t(pg.num_values);
    const uint32_t e_begin = blk * FBLK;
    if (blk > 0 && e_begin >= ne) return;
    const uint32_t e_end = min(ne, e_begin + FBLK);
    constexpr int w = W;
    const int bw = bit_width(uint32_t(ck.max_def));
    const uint32_t maxd = uint32_t(ck.max_def);
    const uint32_t nr = LT->nruns;
    const LvlRun* runs = lvl_runs(LT);
    const LvlBlock& bt = *lvl_block(LT, pg.lvl_cap, blk);
    const uint32_t r0 = bt.r0, r1 = bt.r1, vb = bt.vb, ve = bt.ve, d0 = bt.d0, d1 = bt.d1, i0 = bt.i0, i1 = bt.i1;
    const uint32_t id_bw = dict ? uint32_t(s.val[0]) : 0u;
    const uint32_t vnr = dict ? T->nruns : 0u;
    const uint32_t idcov = dict ? T->covered : 0u;
    const uint8_t* ids = dict ? s.val + 1 : nullptr;
    const uint64_t ids_n = dict ? s.val_n - 1 : 0;
    if (r1 < r0 || (r1 == r0 && e_end > e_begin) || r1 - r0 > LT_BLOCK_RUNS || r1 > nr || id_bw > 32 || ve < vb || d1 < d0 || d1 - d0 + 16u > nc.dcap ||
        i1 < i0 || i1 - i0 + 16u > nc.icap || (dict && ve > idcov) || (!dict && uint64_t(ve) * uint64_t(w) > s.val_n)) {
        if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi);
        return;
    }
    NSTAMP(1);
    // one round of loads: level runs, id runs, level bytes, id bytes
    const uint32_t nrun = r1 - r0;
    for (uint32_t i = tid; i < nrun; i += NTN) {
        const LvlRun& q = lvl_run(runs, r0 + i);
        const uint32_t f = q.first, d = q.data, c = q.cw;
        S.drun[i] = make_uint2(f | (c & 0x80000000u), d);
        if (i + 1 == nrun) S.drun[nrun] = make_uint2(f + (c & 0x7fffffffu), 0u);
    }
    for (uint32_t i = tid; i <= vnr; i += NTN)
        S.vrun[i] = i < vnr ? make_uint2(T->fp(i), T->data(i)) : make_uint2(idcov, 0u);
    const uint32_t doff = stage_bytes(s_dst, s.def, s.def_n, d0, d1);
    const uint32_t ioff = dict ? stage_bytes(s_ist, ids, ids_n, i0, i1) : 0u;
    for (uint32_t i = tid; i < FBLK / 32 + 2; i += NTN) S.vbits[i] = 0;
    const bool dl = dict && dlds != 0 && ck.dict_n > 0 && uint64_t(ck.dict_n) * uint64_t(w) <= dlds &&
                    (reinterpret_cast<uintptr_t>(ck.dict_data) & 7u) == 0;
    if (dl) {   // the dictionary into LDS (8-byte loads; the page body is 16-byte aligned scratch)
        const uint64_t* g = reinterpret_cast<const uint64_t*>(ck.dict_data);
        const uint32_t nw = uint32_t((uint64_t(ck.dict_n) * uint64_t(w) + 7u) / 8u);
        for (uint32_t i = tid; i < nw; i += NTN) DL[i] = g[i];
    }
    __syncthreads();
    NSTAMP(2);
    const uint8_t* dst8 = reinterpret_cast<const uint8_t*>(s_dst);
    const uint8_t* ist8 = reinterpret_cast<const uint8_t*>(s_ist);
    const uint32_t dbase = d0 * 8u - doff * 8u;   // stream bit of LDS bit 0
    const uint32_t ibase = i0 * 8u - ioff * 8u;
    const uint32_t dlim = (d1 - d0 + doff + 16u) * 8u;   // readable LDS bits
    const uint32_t ilim = (i1 - i0 + ioff + 16u) * 8u;
    int bad = 0;
    // present bits of this thread's entries
    const uint32_t e = e_begin + uint32_t(tid) * NEPT;
    const uint32_t m = e < e_end ? min(uint32_t(NEPT), e_end - e) : 0u;
    uint32_t fv = 0;
    if (m) {
        int r = rl_find(S.drun, int(nrun), e);
        const uint2 R = S.drun[r];
        const uint32_t Rf = rl_first(R), Rp = R.x >> 31;
        if (e + m <= rl_first(S.drun[r + 1]) && (!Rp || bw == 1)) {   // one run
            if (!Rp) fv = R.y == maxd ? ((1u << m) - 1u) : 0u;
            else {
                const uint32_t b = R.y + (e - Rf) - dbase;
                fv = b + m <= dlim ? lds_bits(dst8, b, m) : 0u;
                bad |= b + m > dlim;
            }
        } else {
            for (uint32_t k = 0; k < m; k++) {
                while (r + 1 < int(nrun) && e + k >= rl_first(S.drun[r + 1])) r++;
                const uint2 Rk = S.drun[r];
                uint32_t dl = Rk.y;
                if (Rk.x >> 31) {
                    const uint32_t b = Rk.y + (e + k - rl_first(Rk)) * uint32_t(bw) - dbase;
                    bad |= b + uint32_t(bw) > dlim;
                    dl = b + uint32_t(bw) <= dlim ? lds_bits(dst8, b, uint32_t(bw)) : 0u;
                }
                bad |= dl > maxd;
                fv |= uint32_t(dl == maxd) << k;
            }
        }
    }
    uint32_t tv;
    const uint32_t vo = block_excl_scan<NTN>(__popc(fv), S.scan_tmp, tv);
    if (tv != ve - vb) bad = 1;   // the block table disagrees with the levels
    NSTAMP(3);
    const uint32_t gv0 = vb + vo;   // value index of this thread's first present entry
    VT v[NEPT];
    #pragma unroll
    for (int k = 0; k < NEPT; k++) v[k] = 0;
    if (fv && !bad) {
        // Two phases: the ids of the present entries (LDS only), then ALL of the thread's gathers
        // issued back to back through global-address-space loads (absent entries load element 0 and
        // are zeroed after), so the wave waits on one round of L2 / HBM latency instead of one per
        // entry (flat loads under per-entry branches each ended in a vmcnt(0) wait).
        if (dict) {
            uint32_t idv[NEPT];
            #pragma unroll
            for (int k = 0; k < NEPT; k++) idv[k] = 0;
            int vr = rl_find(S.vrun, int(vnr), gv0);
            const uint2 V0 = S.vrun[vr];
            // the thread's present values are gv0, gv0 + 1, ...: when one id run holds them all, their
            // ids are consecutive fields of that run (no run search per value)
            const bool one_run = gv0 + uint32_t(__popc(fv)) <= rl_first(S.vrun[vr + 1]);
            const uint32_t b0 = (V0.x >> 31) ? uint32_t(uint64_t(V0.y) + uint64_t(gv0 - rl_first(V0)) * id_bw - ibase) : 0u;
            const int64_t dn = ck.dict_n;
            uint32_t r = 0;
            #pragma unroll
            for (int k = 0; k < NEPT; k++) {
                if (!((fv >> k) & 1u)) continue;
                uint32_t id;
                if (one_run) {
                    id = V0.y;
                    if (V0.x >> 31) {
                        const uint32_t b = b0 + r * id_bw;
                        bad |= b + id_bw > ilim;
                        id = b + id_bw <= ilim ? lds_bits(ist8, b, id_bw) : 0u;
                    }
                } else {
                    const uint32_t gv = gv0 + r;
                    while (vr + 1 < int(vnr) && gv >= rl_first(S.vrun[vr + 1])) vr++;
                    const uint2 V = S.vrun[vr];
                    id = V.y;
                    if (V.x >> 31) {
                        const uint32_t b = uint32_t(uint64_t(V.y) + uint64_t(gv - rl_first(V)) * id_bw - ibase);
                        bad |= b + id_bw > ilim;
                        id = b + id_bw <= ilim ? lds_bits(ist8, b, id_bw) : 0u;
                    }
                }
                r++;
                bad |= int64_t(id) >= dn;
                idv[k] = int64_t(id) < dn ? id : 0u;
            }
            const uintptr_t da = reinterpret_cast<uintptr_t>(ck.dict_data);
            if (dl) {
                #pragma unroll
                for (int k = 0; k < NEPT; k++) v[k] = reinterpret_cast<const VT*>(DL)[idv[k]];
            } else if ((da & uintptr_t(w - 1)) == 0) {   // (dictionary pages start 16-byte aligned in scratch)
                const PF_GLOBAL VT* g = (const PF_GLOBAL VT*)ck.dict_data;
                #pragma unroll
                for (int k = 0; k < NEPT; k++) v[k] = g[idv[k]];
            } else {
                #pragma unroll
                for (int k = 0; k < NEPT; k++) {
                    const uint8_t* src = ck.dict_data + uint64_t(idv[k]) * uint64_t(w);
                    if constexpr (W == 4) v[k] = ld_u32_any(src); else v[k] = ld_u64_any(src);
                }
            }
        } else {
            // value of entry k: gv0 + present entries before k (absent entries load their successor's,
            // clamped to the thread's last present value)
            const uint32_t last = gv0 + uint32_t(__popc(fv)) - 1u;
            uint32_t vi[NEPT];
            #pragma unroll
            for (int k = 0; k < NEPT; k++) vi[k] = min(gv0 + uint32_t(__popc(fv & ((1u << k) - 1u))), last);
            if ((reinterpret_cast<uintptr_t>(s.val) & uintptr_t(w - 1)) == 0) {
                const PF_GLOBAL VT* g = (const PF_GLOBAL VT*)s.val;
                #pragma unroll
                for (int k = 0; k < NEPT; k++) v[k] = g[vi[k]];
            } else {
                #pragma unroll
                for (int k = 0; k < NEPT; k++) {
                    const uint8_t* src = s.val + uint64_t(vi[k]) * uint64_t(w);
                    if constexpr (W == 4) v[k] = ld_u32_any(src); else v[k] = ld_u64_any(src);
                }
            }
        }
        #pragma unroll
        for (int k = 0; k < NEPT; k++)
            if (!((fv >> k) & 1u)) v[k] = 0;
    }
    const uint64_t slot_base = uint64_t(pg.entry_start);
    if (m && !bad) {
        uint8_t* dst0 = ck.values + (slot_base + e) * uint64_t(w);
        if (m == NEPT && (reinterpret_cast<uintptr_t>(dst0) & 15u) == 0) {
            u32x4* d4 = reinterpret_cast<u32x4*>(dst0);
            if constexpr (W == 4) {
                #pragma unroll
                for (int q = 0; q < NEPT / 4; q++) d4[q] = u32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
            } else {
                #pragma unroll
                for (int q = 0; q < NEPT / 2; q++)
                    d4[q] = u32x4{uint32_t(v[2 * q]), uint32_t(v[2 * q] >> 32), uint32_t(v[2 * q + 1]), uint32_t(v[2 * q + 1] >> 32)};
            }
        } else {
            for (uint32_t k = 0; k < m; k++) {
                uint32_t* d = reinterpret_cast<uint32_t*>(dst0 + uint64_t(k) * uint64_t(w));   // 4-byte aligned
                d[0] = uint32_t(v[k]);
                if constexpr (W == 8) d[1] = uint32_t(uint64_t(v[k]) >> 32);
            }
        }
    }
    if (ck.validity && fv) {
        const uint64_t abase = (slot_base + e_begin) & ~uint64_t(31);
        const uint64_t rb = slot_base + e - abase;
        const uint32_t sh = uint32_t(rb & 31);
        atomicOr(&S.vbits[rb >> 5], fv << sh);
        if (sh + NEPT > 32 && sh) atomicOr(&S.vbits[(rb >> 5) + 1], fv >> (32 - sh));
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0) set_status(res, pg.chunk, ST_CORRUPT, pi);
        return;
    }
    if (ck.validity) flush_bits(S.vbits, slot_base + e_begin, e_end - e_begin, ck.validity);
    if (tid == 0) {
        if (ck.needs_count == 0) atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values), (unsigned long long)tv);
        atomicOr(&pg.done, DONE_NULL);
    }
#ifdef PF_STAMPS
    NSTAMP(4);
    if (tid == 0) { PSTAMP(0, 1); PSTAMP(5, t_ph - t_beg); }
#endif
#undef NSTAMP
}

#ifdef PF_DIAG   // diagnostics build only (VERDICT r05 hygiene)
// k_page_null: one 512-thread workgroup per nullable flat page (fixed width 4 / 8, dictionary or
// PLAIN), for pages whose level section (<= LVL_STAGE bytes), level runs (<= PN_RUNS) and
// dictionary-id bytes (<= PN_IST) fit its LDS. It runs before k_lvl in the levels stage and does
// k_lvl's and k_flat_null's work for the page in one launch: the level and id sections are staged
// once, the level run headers are found by the all-positions chain (every byte decoded as a
// header, the chain from 0 followed in LDS), decoded in parallel and prefix-summed, and the page's
// 4096-entry blocks are then decoded in a loop (8 consecutive entries per thread, present bits ->
// block scan -> value index -> id from LDS -> gathers issued together -> 16-byte stores). The
// page's metadata chain, its section staging and the level parse are paid once per page instead of
// once per block, and k_lvl's one-wave block-table pass is gone. Anything it cannot decode
// exactly (a broken chain, an id past the dictionary, too many runs) leaves the page unmarked:
// k_lvl / k_flat_null / k_decode then take it and report it as before.
constexpr int PN_NT = 512;
constexpr uint32_t PN_RUNS = 512;        // level runs held in LDS
constexpr uint32_t PN_IST = 32768;       // dictionary-id bytes staged in LDS
constexpr uint32_t PN_MAX_BLOCKS = 16;   // entries <= 16 * FBLK
constexpr int PN_NEPT = FBLK / PN_NT;    // 8 consecutive entries per thread
struct PageNullLds {
    uint32_t lv[(LVL_STAGE + 64) / 4];
    uint16_t nxt[LVL_STAGE];
    Run drun[PN_RUNS];
    Run vrun[RUN_CAP];
    uint32_t ist[PN_IST / 4 + 8];
    uint32_t vbits[FBLK / 32 + 2];
    uint32_t scan_tmp[PN_NT / 64];
    uint32_t nh, ok, take;
};
__global__ __launch_bounds__(PN_NT) void k_page_null(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                    const int* __restrict__ list, DevChunkResult* res) {
    __shared__ __attribute__((aligned(16))) PageNullLds S;
    const int pi = list[blockIdx.x];
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    const IdRunTab* T = pg.runtab;
    Sections s;
    const int w = ck.width;
    const bool dict = is_dict_enc(pg.encoding);
    const uint32_t ne = uint32_t(pg.num_values);
    // (uniform: every thread evaluates the same loads)
    bool take = pg.lvltab != nullptr && res[pg.chunk].status == 0 && ck.max_rep == 0 && ck.max_def > 0 &&
                (w == 4 || w == 8) && ck.values != nullptr && !(pg.done & (DONE_FIXED | DONE_NULL)) &&
                (dict || pg.encoding == 0) && ne > 0 && ne <= PN_MAX_BLOCKS * FBLK && page_sections(pg, ck, s) &&
                s.def_rle && s.def_n > 0 && s.def_n <= LVL_STAGE;
    uint32_t id_bw = 0, idn = 0, vnr = 0, idcov = 0;
    if (take && dict) {
        take = T != nullptr && T->valid == 1u && T->nruns <= uint32_t(RUN_CAP) && T->nruns > 0 && s.val_n > 1 && s.val[0] <= 32 &&
               s.val_n - 1 <= PN_IST && ck.dict_data != nullptr && ck.dict_n > 0;
        if (take) { id_bw = s.val[0]; idn = uint32_t(s.val_n - 1); vnr = T->nruns; idcov = T->covered; }
    }
    if (!take) return;
    const int bw = bit_width(uint32_t(ck.max_def));
    const uint32_t maxd = uint32_t(ck.max_def);
    const uint32_t dn = uint32_t(s.def_n);
    // ---- stage: level bytes, id bytes, id runs (one round of loads)
    const uint32_t doff = stage_bytes(S.lv, s.def, dn, 0, dn);
    const uint32_t ioff = dict ? stage_bytes(S.ist, s.val + 1, idn, 0, idn) : 0u;
    for (uint32_t i = tid; i < vnr; i += PN_NT) S.vrun[i] = id_run(T, i, vnr, idcov);
    __syncthreads();
    const uint8_t* lv8 = reinterpret_cast<const uint8_t*>(S.lv);
    const uint8_t* stw = lv8 + doff;   // stw[i] = level section byte i (zero past the section)
    // ---- level run headers: every byte position as a header (position of the next one)
    for (uint32_t p = tid; p < dn; p += PN_NT) {
        uint32_t h = 0, hl = 0, nx = 0xffffu;
        #pragma unroll
        for (uint32_t k = 0; k < 3; k++) {   // (a header of > 3 bytes counts > 2^20 entries: no run here)
            const uint32_t c = p + k < dn ? uint32_t(stw[p + k]) : 0x80u;
            h |= (c & 0x7fu) << (7 * k);
            if (!(c & 0x80u)) { hl = k + 1; break; }
        }
        if (hl) {
            const uint32_t pay = (h & 1u) ? (h >> 1) * uint32_t(bw) : (uint32_t(bw) + 7u) >> 3;
            if (p + hl + pay <= dn) nx = p + hl + pay;
        }
        S.nxt[p] = uint16_t(nx);
    }
    __syncthreads();
    if (tid == 0) {   // the chain from position 0 (one LDS load per run)
        uint32_t p = 0, nh = 0;
        bool ok = true;
        while (p < dn) {
            if (nh == PN_RUNS) { ok = false; break; }
            S.drun[nh++].data = p;   // header position (decoded below)
            const uint32_t q = S.nxt[p];
            if (q == 0xffffu) { ok = false; break; }   // no valid run at p
            p = q;
        }
        S.nh = nh;
        S.ok = ok ? 1u : 0u;
    }
    __syncthreads();
    if (!S.ok) return;   // k_lvl / k_decode take the page (and report what is wrong with it)
    const uint32_t nh = S.nh;
    {   // decode the headers in parallel; first entries by a block scan of the counts
        uint32_t cnt = 0, data = 0, packed = 0;
        bool bad = false;
        const uint32_t k = uint32_t(tid);
        if (k < nh) {
            const uint32_t P = S.drun[k].data;
            uint32_t h = 0, hl = 0;
            for (uint32_t b = 0; b < 3; b++) {
                const uint32_t c = stw[P + b];
                h |= (c & 0x7fu) << (7 * b);
                if (!(c & 0x80u)) { hl = b + 1; break; }
            }
            packed = h & 1u;
            cnt = packed ? (h >> 1) * 8u : (h >> 1);
            if (packed) data = (doff + P + hl) * 8u;   // LDS bit offset of the run's first level
            else {
                for (uint32_t b = 0; b < ((uint32_t(bw) + 7u) >> 3); b++) data |= uint32_t(stw[P + hl + b]) << (8 * b);
                bad = data > maxd;
            }
        }
        uint32_t tot;
        const uint32_t first = block_excl_scan<PN_NT>(cnt, S.scan_tmp, tot);
        if (k < nh) {
            Run r;
            r.first = first;
            r.count = cnt;
            r.data = data;
            r.packed = packed;
            S.drun[k] = r;
        }
        if (__syncthreads_or(bad || (tid == 0 && tot < ne))) return;
    }
    // ---- the page's blocks
    const uint64_t slot_base = uint64_t(pg.entry_start);
    const uint8_t* ist8 = reinterpret_cast<const uint8_t*>(S.ist);
    const uint32_t ilim = (ioff + idn) * 8u;   // staged id bits
    const uint32_t nblk = (ne + FBLK - 1) / FBLK;
    const uintptr_t da = reinterpret_cast<uintptr_t>(dict ? ck.dict_data : s.val);
    const bool galign = (da & uintptr_t(w - 1)) == 0;
    const int64_t dnn = dict ? ck.dict_n : 0;
    uint32_t vbase = 0;   // page-relative index of the block's first present value
    for (uint32_t b = 0; b < nblk; b++) {
        const uint32_t e_begin = b * FBLK, e_end = min(ne, e_begin + FBLK);
        for (uint32_t i = tid; i < FBLK / 32 + 2; i += PN_NT) S.vbits[i] = 0;
        const uint32_t e = e_begin + uint32_t(tid) * PN_NEPT;
        const uint32_t m = e < e_end ? min(uint32_t(PN_NEPT), e_end - e) : 0u;
        uint32_t fv = 0;
        int bad = 0;
        if (m) {
            int r = run_find(S.drun, int(nh), e);
            const Run R = S.drun[r];
            if (e + m <= R.first + R.count && (!R.packed || bw == 1)) {   // one run
                if (!R.packed) fv = R.data == maxd ? ((1u << m) - 1u) : 0u;
                else fv = lds_bits(lv8, R.data + (e - R.first), m);
            } else {
                for (uint32_t k = 0; k < m; k++) {
                    while (r + 1 < int(nh) && e + k >= S.drun[r].first + S.drun[r].count) r++;
                    const Run& Rk = S.drun[r];
                    uint32_t dl = Rk.data;
                    if (Rk.packed) dl = lds_bits(lv8, Rk.data + (e + k - Rk.first) * uint32_t(bw), uint32_t(bw));
                    bad |= dl > maxd;
                    fv |= uint32_t(dl == maxd) << k;
                }
            }
        }
        uint32_t tv;
        const uint32_t vo = block_excl_scan<PN_NT>(__popc(fv), S.scan_tmp, tv);
        const uint32_t gv0 = vbase + vo;
        uint32_t idv[PN_NEPT];
        #pragma unroll
        for (int k = 0; k < PN_NEPT; k++) idv[k] = 0;
        if (fv) {
            if (dict) {
                if (gv0 + uint32_t(__popc(fv)) > idcov) bad = 1;
                int vr = run_find(S.vrun, int(vnr), gv0);
                uint32_t j = 0;
                #pragma unroll
                for (int k = 0; k < PN_NEPT; k++) {
                    if (!((fv >> k) & 1u)) continue;
                    const uint32_t gv = gv0 + j++;
                    while (vr + 1 < int(vnr) && gv >= S.vrun[vr].first + S.vrun[vr].count) vr++;
                    const Run& V = S.vrun[vr];
                    uint32_t id = V.data;
                    if (V.packed) {
                        const uint64_t bb = uint64_t(V.data) + uint64_t(ioff) * 8u + uint64_t(gv - V.first) * id_bw;
                        bad |= bb + id_bw > ilim;
                        id = bb + id_bw <= ilim ? lds_bits(ist8, uint32_t(bb), id_bw) : 0u;
                    }
                    bad |= int64_t(id) >= dnn;
                    idv[k] = int64_t(id) < dnn ? id : 0u;
                }
            } else {
                const uint32_t last = gv0 + uint32_t(__popc(fv)) - 1u;
                if (uint64_t(last + 1) * uint64_t(w) > s.val_n) bad = 1;
                #pragma unroll
                for (int k = 0; k < PN_NEPT; k++) idv[k] = bad ? 0u : min(gv0 + uint32_t(__popc(fv & ((1u << k) - 1u))), last);
            }
        }
        if (__syncthreads_or(bad)) return;   // (nothing counted or marked: the fallback redoes the page)
        uint64_t v[PN_NEPT];
        #pragma unroll
        for (int k = 0; k < PN_NEPT; k++) v[k] = 0;
        if (!fv) {
        } else if (galign) {
            if (w == 4) {
                const PF_GLOBAL uint32_t* g = (const PF_GLOBAL uint32_t*)da;
                #pragma unroll
                for (int k = 0; k < PN_NEPT; k++) v[k] = g[idv[k]];
            } else {
                const PF_GLOBAL uint64_t* g = (const PF_GLOBAL uint64_t*)da;
                #pragma unroll
                for (int k = 0; k < PN_NEPT; k++) v[k] = g[idv[k]];
            }
        } else {
            #pragma unroll
            for (int k = 0; k < PN_NEPT; k++) {
                const uint8_t* src = reinterpret_cast<const uint8_t*>(da) + uint64_t(idv[k]) * uint64_t(w);
                v[k] = w == 4 ? uint64_t(ld_u32_any(src)) : ld_u64_any(src);
            }
        }
        #pragma unroll
        for (int k = 0; k < PN_NEPT; k++)
            if (!((fv >> k) & 1u)) v[k] = 0;
        if (m) {
            uint8_t* dst0 = ck.values + (slot_base + e) * uint64_t(w);
            if (m == PN_NEPT && (reinterpret_cast<uintptr_t>(dst0) & 15u) == 0) {
                u32x4* d4 = reinterpret_cast<u32x4*>(dst0);
                if (w == 4) {
                    d4[0] = u32x4{uint32_t(v[0]), uint32_t(v[1]), uint32_t(v[2]), uint32_t(v[3])};
                    d4[1] = u32x4{uint32_t(v[4]), uint32_t(v[5]), uint32_t(v[6]), uint32_t(v[7])};
                } else {
                    #pragma unroll
                    for (int q = 0; q < 4; q++)
                        d4[q] = u32x4{uint32_t(v[2 * q]), uint32_t(v[2 * q] >> 32), uint32_t(v[2 * q + 1]), uint32_t(v[2 * q + 1] >> 32)};
                }
            } else {
                for (uint32_t k = 0; k < m; k++) {
                    uint32_t* d = reinterpret_cast<uint32_t*>(dst0 + uint64_t(k) * uint64_t(w));   // 4-byte aligned
                    d[0] = uint32_t(v[k]);
                    if (w == 8) d[1] = uint32_t(v[k] >> 32);
                }
            }
        }
        if (ck.validity && fv) {
            const uint64_t abase = (slot_base + e_begin) & ~uint64_t(31);
            const uint64_t rb = slot_base + e - abase;
            const uint32_t sh = uint32_t(rb & 31);
            atomicOr(&S.vbits[rb >> 5], fv << sh);
            if (sh + PN_NEPT > 32 && sh) atomicOr(&S.vbits[(rb >> 5) + 1], fv >> (32 - sh));
        }
        __syncthreads();
        if (ck.validity) flush_bits(S.vbits, slot_base + e_begin, e_end - e_begin, ck.validity);
        vbase += tv;
        __syncthreads();   // (vbits / scan_tmp reused by the next block)
    }
    if (tid == 0) {
        if (ck.needs_count == 0) atomicAdd(reinterpret_cast<unsigned long long*>(&res[pg.chunk].num_values), (unsigned long long)vbase);
        atomicOr(&pg.done, DONE_NULL | DONE_PAGE);
    }
}
#endif  // PF_DIAG

// ---- launchers -------------------------------------------------------------------------------
void launch_lvl(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res,
                hipStream_t st, bool page_null, NullCaps nc) {
    if (n <= 0) return;
    // page_null (diagnostics option): k_page_null first (one 512-thread workgroup and ~57 KiB of LDS per
    // page; under the bench's four streams its workgroups wait for whole CUs: config 4 5.57 ms with it, 4.47 without)
#ifdef PF_DIAG
    if (page_null) hipLaunchKernelGGL(k_page_null, dim3(n), dim3(PN_NT), 0, st, d_chunks, d_pages, d_list, d_res);
#else
    (void)page_null;
#endif
    hipLaunchKernelGGL(k_lvl, dim3(n), dim3(LT_NT), 0, st, d_chunks, d_pages, d_list, d_res, nc.dcap, nc.icap);
}
// blocks: n4 (page, block) pairs of nullable 4-byte pages, then n8 of 8-byte pages. nc: the LDS stages
// (dictionary: nc.dlds bytes); stagger: launch_flat's
void launch_flat_null(const DevChunk* d_chunks, DevPage* d_pages, const int2* blocks, int n4, int n8, int* d_fbq,
                      DevChunkResult* d_res, hipStream_t st, NullCaps nc, int stagger) {
    const size_t dyn = size_t(nc.dcap) + 32u + nc.icap + 32u + nc.dlds;
    if (n4 > 0) hipLaunchKernelGGL(k_flat_null<4>, dim3(n4), dim3(NTN), dyn, st, d_chunks, d_pages, blocks, d_res, nc, stagger, d_fbq);
    if (n8 > 0)
        hipLaunchKernelGGL(k_flat_null<8>, dim3(n8), dim3(NTN), dyn, st, d_chunks, d_pages, blocks + n4, d_res, nc, stagger, d_fbq);
}

}  // namespace pf
