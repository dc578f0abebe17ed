// pf_snappy_exec.hip — K1, execute stage of the block-parallel Snappy decompressor: k_snappy_exec5.
//
// The parse stage (pf_snappy_parse.hip) leaves a token-start bitmap over every page's input and the
// input position of the token at each 64 KiB output boundary. Google Snappy compresses in
// independent 64 KiB blocks, so each such piece of a page decodes on its own:
//
//   k_snappy_exec5  one two-wave workgroup per 64 KiB piece (mode 0), or per page whose pieces turned
//                   out not to be independent and which is redone as a whole (mode 1, FB_REDO). A producer
//                   wave decodes the tokens into batches, a consumer wave resolves their bytes into a
//                   4 KiB LDS ring (pf_snappy_exec.h) and flushes it in 1 KiB slots; a copy that reaches
//                   further back reads the flushed output from HBM. "executor v5" below describes it.
//   k_snappy_exec2  (pf_snappy_exec2.hip, diagnostics build, PfOpts::exec == 2) the one-wave executor
//                   it is tested against.
//   k_snappy_serial (pf_snappy.hip) re-decodes serially any page the executor rejects (FB_SERIAL).
//
// launch_snappy_exec runs the pieces, the redo and the serial kernel in stream order; launch_snappy
// is the parse stage followed by it.
#include <hip/hip_runtime.h>

#include "pf_launch.h"
#include "pf_snappy_exec.h"
#include "pf_stamps.h"

namespace pf {

// Phase stamps of k_snappy_exec5 (its X5T marks; tools/probe_exec5.py).
#ifdef PF_STAMPS
PF_STAMP_TABLE(pf_stamps, 16, pf_debug_stamps)
#define STAMP_ADD(i, v) atomicAdd(&pf_stamps[i], (unsigned long long)(v))
#else
#define STAMP_ADD(i, v) ((void)0)
#endif

// ======================================================================== executor v5
//
// One wave (k_snappy_exec2) runs each 64-token batch as one serial instruction stream, and a dense piece
// (16 K tokens per 64 KiB: l_partkey, l_extendedprice; sorted l_orderkey) is issue-bound at one
// wave's rate — a wave alone on its SIMD issues a VALU instruction every 4 cycles — at ~600-700 K
// cycles; the slowest piece sets the executor launch. k_snappy_exec5 splits that stream over the
// two waves of one workgroup (two SIMDs), pipelined by one batch:
//   wave 0 (producer): stages input, enumerates token starts, decodes batch i's tokens (output
//     offsets, chain checks, cuts), loads its far-copy sources from HBM into LDS and writes the
//     packed descriptors and token-start words into LDS buffer i & 1;
//   wave 1 (consumer): meanwhile resolves batch i-1's bytes (exec2's windows, descriptors read from
//     LDS instead of permuted from the token lanes) into the ring and flushes whole ring slots.
// One workgroup barrier per batch. A far copy's source was flushed by the consumer: before every
// barrier the consumer waits until all but its newest store have landed (all of them after a long
// literal or an empty batch), the producer derives from the batch history the frontier below which
// that guarantees the bytes (and their cache line) are in HBM, and a far copy above it cuts the batch
// (one empty batch when it is the first token, which only follows a long literal).
#ifndef PF_X5_BATCH
#define PF_X5_BATCH 764
#endif
constexpr uint32_t X5_BATCH = PF_X5_BATCH;                     // output bytes of one batch (ring: + XSLOT + far margin)
constexpr uint32_t X5_STG = (XSTAGE + 15u) & ~15u;     // one staged input chunk
// Far-copy sources of a batch, packed by 16-byte chunk. A far copy of ol bytes whose source's global address
// has the low four bits fsh takes the nch = (fsh + ol + 15) >> 4 aligned chunks that cover it (1..5: ol <= 64,
// fsh < 16), at chunks [cb, cb + nch) of the batch's buffer, cb the sum of nch over the batch's earlier far
// copies in token order. Chunk cb + i holds the 16 bytes at (source address - fsh) + 16 i, so source byte j is
// buffer byte 16 cb + fsh + j. The consumer reads a far copy's byte j < ol only, through descriptor word 1
// (below), and fsh + j < fsh + ol <= 16 nch: every byte it reads lies in a chunk this copy loaded. Chunks past
// the batch's total are not loaded and keep stale bytes; no descriptor points at them. A batch is cut before the
// far copy whose chunks would pass X5_FCH.
#ifndef PF_X5_FCH
#define PF_X5_FCH 64
#endif
constexpr uint32_t X5_FCH = PF_X5_FCH;                 // far-copy source chunks of one batch
constexpr uint32_t X5_FSL = X5_FCH * 16u;              // their bytes (first the chunk address table, then the chunks)
constexpr uint32_t X5_STAGE0 = XRING;                  // [ring | stage x2 | far chunks x2]: one byte address
constexpr uint32_t X5_LDS = XRING + 2u * X5_STG;       // selects any byte source (the far chunks: their own array)
constexpr uint32_t X5_W = 768u / 32u;                  // token-start words of a batch (+ its alignment bytes)
constexpr uint32_t X5_LINE = 128u;                     // a far source's cache line must be wholly landed
#ifndef PF_X5_TPL
#define PF_X5_TPL 2
#endif
constexpr int X5_TPL = PF_X5_TPL;                      // tokens a producer lane decodes per batch
constexpr uint32_t X5_DS = 64u * X5_TPL + 1u;          // descriptor table: entry t at [t], its second word at [t + X5_DS]
static_assert(X5_BATCH + 3u <= 768u, "a batch and its alignment bytes are at most three 256-byte windows");
static_assert(X5_FCH <= 128u, "a batch's far-copy chunks are loaded by at most two LDS-DMA wave instructions");
static_assert(X5_FCH >= 32u && (X5_FCH > 64u ? 128u : 64u) * 8u <= X5_FSL && (X5_FCH + 4u) * 8u <= X5_FSL,
              "the chunk address table (an entry per loading lane, and four past the last chunk) lies inside one batch's chunk bytes");
enum : uint32_t { R5_NORMAL = 0, R5_LONG = 1, R5_NOP = 2, R5_END = 3, R5_BAD = 4 };
// Descriptor word 0: the token's first output byte relative to the batch's 4-byte aligned base S
// (bits 0-15); a copy whose source is read through the ring / the window: its offset (< 4 KiB) in bits
// 16-30 and bit 31 set. Word 1: a literal or far copy: the LDS address of its byte at base position x is
// word1 + x; a ring copy: m = floor(65536 / offset) + 1 (or one more), so that (j * m) >> 16 =
// floor(j / offset) for the byte's index j < 64 in the token: byte x's source is
// x - offset * (1 + floor(j / offset)), the byte an overlapping copy reads as j mod offset. Entry 0 is a
// dummy literal for the batch's alignment bytes (token t of the batch is entry t + 1).
constexpr uint32_t X5_CP = 0x80000000u;
// A ring copy's offset is at most XRING - 1 (near: off <= (otok - op) + XRING - X5_BATCH); the (j * m) >> 16
// identity is checked for offsets below 4096 (tests/test_exec_arith.py) and PF_XRING is a build-time override.
static_assert(XRING <= 4096u, "ring-copy offsets must stay below 4096: tests/test_exec_arith.py checks (j * m) >> 16 up to there");

// Workgroup barrier for LDS hand-over only (no wait on outstanding global stores).
__device__ __forceinline__ void x5_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// Compiler ordering point for one wave's LDS accesses (the hardware runs them in order).
__device__ __forceinline__ void x5_order() { asm volatile("" ::: "memory"); }

// Two 16-bit jump words at once: each half of w still pending (bit 15) takes the half of g
// (v_pk_ashrrev_i16 makes the per-half mask, v_bfi_b32 merges; the compiler otherwise splits the halves).
__device__ __forceinline__ uint32_t x5_pick(uint32_t w, uint32_t g) {
    uint32_t m, r;
    asm("v_pk_ashrrev_i16 %0, 15, %1 op_sel_hi:[0,1]" : "=v"(m) : "v"(w));   // (the shift in both halves)
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(g), "v"(w));
    return r;
}

struct X5Lds {
    __attribute__((aligned(16))) uint8_t L[X5_LDS];
    uint16_t tokpos[XCHUNK / 2];
    uint32_t D[2][2 * X5_DS];            // token descriptors (entry 0: the dummy literal)
    uint32_t SB[2][X5_W], WP[2][X5_W];   // token starts from the batch's aligned base, tokens in earlier words
    uint32_t REC[2][4];                  // kind, output start, output bytes, long literal input position
    __attribute__((aligned(8))) uint16_t jv[256];
#if defined(PF_X5_PAD) && PF_X5_PAD > 0
    uint8_t pad[PF_X5_PAD];   // diagnostics: fewer executor workgroups per CU (room for other streams' kernels)
#endif
};

// 16 input bytes from gin[src] (src + 15 < the stream's end) as four dwords: 16-byte aligned loads only
// (the second chunk only when src is not aligned), so no load passes the chunk holding the last byte.
__device__ __forceinline__ u32x4 x5_load16(const PF_GLOBAL uint8_t* gin, uint32_t src) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(gin) + src;
    const PF_GLOBAL u32x4* p = (const PF_GLOBAL u32x4*)(a & ~uintptr_t(15));
    const uint32_t sh = uint32_t(a & 15u);
    const u32x4 A = p[0];
    u32x4 B = A;
    if (sh) B = p[1];
    const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    const uint32_t k = sh >> 2, s = sh & 3u;
    u32x4 r;
    #pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t lo = k == 0 ? w[i] : (k == 1 ? w[i + 1] : (k == 2 ? w[i + 2] : w[i + 3]));
        const uint32_t hi = k == 0 ? w[i + 1] : (k == 1 ? w[i + 2] : (k == 2 ? w[i + 3] : w[i + 4]));
        r[i] = __builtin_amdgcn_alignbyte(hi, lo, s);
    }
    return r;
}

// 16 bytes a lane from global address g into LDS at m0 + 16 * lane (LDS-DMA). Issued from inline asm: the
// compiler, which cannot tell the destination from the producer's other LDS accesses, would otherwise wait
// for the load before the next of them; the producer waits for it itself before the batch's barrier.
// (m0 is a reserved register the compiler does not take as a clobber; no code it generates for this unit's one
// kernel, k_snappy_exec5, reads m0 -- checked in the assembly, round 6 -- so every m0 value is this function's.
// A kernel added to pf_snappy_exec.hip comes under the same check.)
__device__ __forceinline__ void x5_dma16(uint64_t g, uint32_t lds) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(g), "s"(lds) : "memory");
}

// One input chunk [I - woff, I - woff + XSTAGE) as lane l's 16-byte chunks l and 64 + l (lanes < 5), and its
// token-start bits (16 input bytes a lane): every load issued before any is used. Chunks wholly at or past n
// read as zero (the chunk holding the last byte is read whole, as snap_stage does).
static_assert(XSTAGE == 64u * 16u + 5u * 16u, "a staged chunk is 64 + 5 lane loads");
__device__ __forceinline__ void x5_chunk_load(const PF_GLOBAL uint8_t* gin, const PF_GLOBAL uint16_t* tm16, uint64_t n, uint32_t I,
                                              int lane, u32x4& va, u32x4& vb, uint32_t& bits) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(gin + I);
    const uint32_t woff = uint32_t(a & 15u);
    const PF_GLOBAL u32x4* src = (const PF_GLOBAL u32x4*)(a - woff);
    const int64_t first = int64_t(I) - int64_t(woff);
    va = u32x4{0u, 0u, 0u, 0u};
    vb = u32x4{0u, 0u, 0u, 0u};
    bits = 0u;
    if (first + 16 * int64_t(lane) < int64_t(n)) va = src[lane];
    if (lane < 5 && first + 16 * int64_t(64 + lane) < int64_t(n)) vb = src[64 + lane];
    const uint32_t p16 = I + 16u * uint32_t(lane);
    if (uint64_t(p16) < n) bits = uint32_t(tm16[p16 >> 4]);
}

// One piece (mode 0: pieces[item]) or one whole-page redo (mode 1: job item) by the workgroup's two waves.
__device__ __forceinline__ void exec5_piece(X5Lds& S, uint8_t* FS, const SnappyJob* __restrict__ jobs, const int2* __restrict__ pieces,
                                            const uint32_t* __restrict__ splits, int* __restrict__ fb, int mode, int item) {
    uint8_t* const L = S.L;
    uint16_t* const tokpos = S.tokpos;
    auto& D = S.D;
    auto& SB = S.SB;
    auto& WP = S.WP;
    auto& REC = S.REC;
    uint8_t* const jvb = reinterpret_cast<uint8_t*>(S.jv);
    uint8_t* const ring = L;
    // The far-copy chunks are a separate LDS array, so the compiler can tell the producer's LDS-DMA from its
    // other LDS accesses (one array: it waits for the loads before the first descriptor write); the
    // consumer reaches them through the same byte address as the ring and stage, relative to L.
    const uint32_t Lb = uint32_t(reinterpret_cast<uintptr_t>(L));   // (a flat LDS address's low half: the LDS offset)
    const uint32_t FSB = uint32_t(reinterpret_cast<uintptr_t>(FS)) - Lb;
    const int wv = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int lane = int(threadIdx.x) & 63;
    int j, k;
    if (mode == 0) {
        const int2 pc = pieces[item];
        j = pc.x;
        k = pc.y;
    } else {
        j = item;
        k = 0;
    }
    const int f = fb[j];
    bool whole;
    if (mode == 0) {
        if (f >= FB_REDO || (f == FB_WHOLE && k > 0)) return;
        whole = f == FB_WHOLE;
    } else {
        if (f != FB_REDO) return;
        whole = true;
    }
    const SnappyJob job = jobs[j];
    const uint8_t* in = job.src;
    const uint64_t n = job.src_len;
    const uint32_t* sp = splits + job.split_base;
    uint64_t pos0 = 0, ulen = 0;
    if (!uvarint(in, n, pos0, ulen) || ulen != job.dst_len) {
        if (threadIdx.x == 0) atomicMax(&fb[j], FB_SERIAL);
        return;
    }
    if (mode == 0 && (job.dflags & 1u)) {   // diagnostics: forced redo
        if (threadIdx.x == 0) atomicMax(&fb[j], FB_REDO);
        return;
    }
    uint32_t ip, out_start, out_end = job.dst_len;
    if (whole) {
        ip = uint32_t(pos0);
        out_start = 0;
    } else {
        if (k > 0 && sp[k] == SNAP_INVALID) return;   // no token at this boundary: an earlier piece covers it
        ip = k == 0 ? uint32_t(pos0) : sp[k];
        out_start = uint32_t(k) * SNAP_BLOCK;
        for (uint32_t k2 = k + 1; k2 < job.n_pieces; k2++)
            if (sp[k2] != SNAP_INVALID) { out_end = k2 * SNAP_BLOCK; break; }
    }
    const PF_GLOBAL uint16_t* tm16 = (const PF_GLOBAL uint16_t*)(job.tokmap);
    const PF_GLOBAL uint8_t* gin = gptr(in);
    PF_GLOBAL uint8_t* gdst = gptr(job.dst);
    const OutDst od{gdst, mode == 0 ? gptr(job.ddst) : nullptr, job.dlo, job.dgran};
    if (threadIdx.x < 2) {   // the dummy entry of both descriptor buffers (a literal reading ring bytes)
        D[threadIdx.x][0] = 0u;
        D[threadIdx.x][X5_DS] = 0u;
    }
    // producer state
    uint32_t op = out_start, sb = 0, T = 0, I = 0, woff = 0, cb = 1;
    uint32_t ops_m1 = out_start, k_m1 = R5_NOP, k_m2 = R5_NOP, nops = 0;
    uint32_t pfI = ~0u, pfbits = 0;   // prefetched input chunk (base, token-start bits, data)
    u32x4 pfa = {0u, 0u, 0u, 0u}, pfb = {0u, 0u, 0u, 0u};
    // consumer state
    uint32_t F = out_start, cop = out_start;
    uint32_t last = R5_END;
#ifdef PF_STAMPS   // per phase cycles: producer slots 0-4 (wave 0), consumer 6-9 (wave 1), 12 batches, 13 pieces
    unsigned long long x5t = __builtin_amdgcn_s_memtime();
#define X5T(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (lane == 0) STAMP_ADD(i, t_ - x5t); x5t = t_; } while (0)
    if (threadIdx.x == 0) STAMP_ADD(13, 1);
#else
#define X5T(i) ((void)0)
#endif
    for (uint32_t it = 0;; it++) {
        const uint32_t b = it & 1u;
        if (wv == 0) {
            if (lane == 0) STAMP_ADD(12, 1);
            // ---------------- producer: batch it into buffer b
            uint32_t kind = R5_BAD, b_op = op, b_tot = 0, b_s0 = 0;
            // landed frontier: the consumer finished batch it-2 before the last barrier
            const uint32_t sf = out_start + ((ops_m1 - out_start) & ~(XSLOT - 1u));
            const uint32_t LF = k_m2 == R5_NORMAL ? (sf >= out_start + XSLOT ? sf - XSLOT : out_start) : sf;
            bool ok = true;
            if (op >= out_end) {
                kind = R5_END;
                ok = false;
            } else if (sb >= T) {   // next input chunk (the other stage buffer: the consumer may read this one)
                if (ip >= n) {
                    ok = false;
                } else {
                    I = ip & ~15u;
                    cb ^= 1u;
                    // the chunk from the registers when the last staging prefetched it (the next chunk starts
                    // where the last token of this one ends: past I + XCHUNK, in the same 16 bytes unless that
                    // token is a literal)
                    u32x4 va, vb;
                    uint32_t bits;
                    if (I == pfI) {
                        va = pfa;
                        vb = pfb;
                        bits = pfbits;
                    } else {
                        x5_chunk_load(gin, tm16, n, I, lane, va, vb, bits);
                    }
                    u32x4* stq = reinterpret_cast<u32x4*>(L + X5_STAGE0 + cb * X5_STG);
                    stq[lane] = va;
                    if (lane < 5) stq[64 + lane] = vb;
                    woff = uint32_t(reinterpret_cast<uintptr_t>(gin + I) & 15u);
                    // prefetch the next chunk: its loads land while this chunk's batches are decoded
                    pfI = I + XCHUNK;
                    if (uint64_t(pfI) < n) x5_chunk_load(gin, tm16, n, pfI, lane, pfa, pfb, pfbits);
                    else pfI = ~0u;
                    const uint32_t p16 = I + 16u * uint32_t(lane);
                    if (p16 + 16u <= ip) bits = 0;
                    else if (p16 < ip) bits &= ~((1u << (ip - p16)) - 1u);
                    const uint32_t cnt = __popc(bits);
                    const uint32_t ex = dpp_incl_scan(cnt);
                    T = __builtin_amdgcn_readlane(ex, 63);
                    uint32_t q = ex - cnt;
                    while (bits) {
                        const uint32_t bb = uint32_t(__ffs(bits) - 1);
                        bits &= bits - 1;
                        tokpos[q++] = uint16_t(16u * uint32_t(lane) + bb);
                    }
                    sb = 0;
                    x5_order();
                    if (T == 0) ok = false;
                }
            }
            X5T(0);   // chunk staging + token enumeration
            if (ok) {
                // X5_TPL tokens a lane: token sb + 64 h + lane in half h (batches of up to 64 X5_TPL tokens)
                const uint32_t stg_off = __builtin_amdgcn_readfirstlane(cb) ? X5_STAGE0 + X5_STG : X5_STAGE0;
                const uint8_t* stg = L + stg_off;
                uint32_t pos[X5_TPL], ol[X5_TPL], start[X5_TPL], endp[X5_TPL], inc[X5_TPL], otok[X5_TPL];
                bool v[X5_TPL], take[X5_TPL];
                SnapTok32 tk[X5_TPL];
                #pragma unroll
                for (int h = 0; h < X5_TPL; h++) {
                    const uint32_t t = sb + 64u * uint32_t(h) + uint32_t(lane);
                    v[h] = t < T;
                    pos[h] = uint32_t(tokpos[min(t, XCHUNK / 2u - 1u)]);   // (read unconditionally; v gates the use)
                    if (!v[h]) pos[h] = 0u;
                }
                uint32_t tlo[X5_TPL], thi[X5_TPL];
                #pragma unroll
                for (int h = 0; h < X5_TPL; h++) lds_read8_2(stg, woff + pos[h], tlo[h], thi[h]);
                #pragma unroll
                for (int h = 0; h < X5_TPL; h++) tk[h] = snap_tok32(tlo[h], thi[h]);
                int nt = 0;
                bool wrong = false;
                uint32_t prevlast = ip, incbase = 0;
                #pragma unroll
                for (int h = 0; h < X5_TPL; h++) {
                    ol[h] = v[h] ? tk[h].ol : 0u;
                    start[h] = I + pos[h];
                    endp[h] = __builtin_elementwise_add_sat(start[h], tk[h].tl);
                    const uint32_t pdpp = dpp_prev(endp[h]);   // (every lane runs the DPP move)
                    const uint32_t prev = lane == 0 ? prevlast : pdpp;
                    inc[h] = incbase + dpp_incl_scan(ol[h]);
                    otok[h] = op + inc[h] - ol[h];
                    take[h] = v[h] && otok[h] < out_end;
                    nt += __popcll(__ballot(take[h]));
                    wrong = wrong || (take[h] && (start[h] != prev || endp[h] > n || op + inc[h] > out_end || inc[h] < ol[h] ||
                                                  inc[h] < incbase));
                    prevlast = __builtin_amdgcn_readlane(endp[h], 63);
                    incbase = __builtin_amdgcn_readlane(inc[h], 63);
                }
                if (__any(wrong) || nt == 0) {
                    ok = false;
                } else {
                    uint32_t kd[X5_TPL], off[X5_TPL], srcv[X5_TPL], a[X5_TPL], fsh[X5_TPL], nch[X5_TPL], fce[X5_TPL];
                    bool farc[X5_TPL], fnr[X5_TPL], lstaged[X5_TPL], fdd[X5_TPL];
                    unsigned long long cutm[X5_TPL], farm = 0;
                    unsigned long long wide2 = 0, wide4 = 0;   // far copies of >= 2 / >= 4 chunks among the tokens
                    #pragma unroll
                    for (int h = 0; h < X5_TPL; h++) {
                        kd[h] = tk[h].kind;
                        off[h] = tk[h].arg;
                        srcv[h] = start[h] + tk[h].arg;   // literal data position
                        lstaged[h] = srcv[h] + ol[h] <= I + XCHUNK + 64;
                        a[h] = otok[h] - off[h];          // copy source start
                        farc[h] = take[h] && kd[h] != 0 && a[h] + min(ol[h], off[h]) <= op &&
                                  int32_t(a[h] - (op + X5_BATCH - XRING)) < 0;
                        // Source not yet landed in HBM: every cache line an issued load touches must lie wholly
                        // below the landed frontier LF. The copy's loads read addresses [A - fsh, A - fsh + 16 nch),
                        // A = arena + a the source's address. They end at output offset
                        // a - fsh + 16 nch <= a + ol + 15 (16 nch <= fsh + ol + 15), at a 16-byte aligned address,
                        // so at most X5_LINE - 16 bytes of the last cache line lie behind them: the highest line
                        // touched ends at or below output offset a + ol + 15 + X5_LINE - 16 of the same arena,
                        // whatever the arena's base alignment is (the scratch body and the column arena of a
                        // direct page are aligned differently, and neither as the output offset). Landed when
                        // that is <= LF; lines below the last are older still. (Bytes of a line that lie outside
                        // this piece's output, or in the scratch body past od.dlo, are never a far copy's source.)
                        fnr[h] = farc[h] && a[h] + ol[h] + (X5_LINE - 1u) > LF;
                        farm |= __ballot(farc[h]);
                        fsh[h] = 0u;
                        nch[h] = 0u;
                        fce[h] = 0u;
                        fdd[h] = false;
                    }
                    if (farm) {   // (a batch without far copies skips this)
                        // (the low bits of the two arenas' addresses: a source's alignment to its 16-byte chunks)
                        const uint32_t dst_lo = uint32_t(reinterpret_cast<uintptr_t>(gdst)) & 15u;
                        const uint32_t dd_lo = uint32_t(reinterpret_cast<uintptr_t>(od.dd)) & 15u;
                        uint32_t anyn = 0;
                        #pragma unroll
                        for (int h = 0; h < X5_TPL; h++) {
                            // the address the source is read from: the column arena from od.dlo on, else the scratch body
                            fdd[h] = od.dd != nullptr && a[h] >= od.dlo;
                            fsh[h] = ((fdd[h] ? dd_lo : dst_lo) + a[h]) & 15u;
                            nch[h] = farc[h] ? (fsh[h] + ol[h] + 15u) >> 4 : 0u;
                            anyn |= nch[h];
                        }
                        wide2 = __ballot(anyn > 1u);
                        wide4 = __ballot(anyn > 3u);
                        // chunk base: the exclusive prefix of nch in token order (fce: the inclusive one). One DPP
                        // scan for two halves of the lanes, 16 bits each (a half's sum is at most 5 * 64)
                        uint32_t cbase = 0;
                        #pragma unroll
                        for (int h = 0; h < X5_TPL; h += 2) {
                            const int h1 = h + 1 < X5_TPL ? h + 1 : h;   // (the pair's second half, if there is one)
                            const uint32_t sc = dpp_incl_scan(nch[h] | (h1 != h ? nch[h1] << 16 : 0u));
                            const uint32_t tot = __builtin_amdgcn_readlane(sc, 63);
                            fce[h] = cbase + (sc & 0xffffu);
                            cbase += tot & 0xffffu;
                            if (h1 != h) {
                                fce[h1] = cbase + (sc >> 16);
                                cbase += tot >> 16;
                            }
                        }
                    }
                    #pragma unroll
                    for (int h = 0; h < X5_TPL; h++)
                        cutm[h] = __ballot(take[h] && (ol[h] > 64u || inc[h] > X5_BATCH || (kd[h] == 0 && !lstaged[h]) ||
                                                       (farc[h] && fce[h] > X5_FCH) || fnr[h]));
                    uint32_t cut = uint32_t(nt);
                    #pragma unroll
                    for (int h = X5_TPL - 1; h >= 0; h--)
                        if (cutm[h]) cut = 64u * uint32_t(h) + uint32_t(__ffsll(cutm[h]) - 1);
                    uint32_t used = 0;
                    if (cut == 0) {
                        if (__builtin_amdgcn_readfirstlane(kd[0]) == 0) {   // one long literal: the consumer copies it
                            kind = R5_LONG;
                            b_tot = __builtin_amdgcn_readfirstlane(ol[0]);
                            b_s0 = __builtin_amdgcn_readfirstlane(srcv[0]);
                            used = 1;
                            nops = 0;
                        } else if (__builtin_amdgcn_readfirstlane(uint32_t(fnr[0])) && nops < 3) {
                            kind = R5_NOP;   // wait one batch for the source's stores to land
                            nops++;
                        } else {
                            ok = false;
                        }
                    } else {
                        used = cut;
                        const uint32_t ch = (cut - 1u) >> 6;   // the half holding the batch's last token
                        uint32_t btot = 0, ntot = 0;   // the batch's output bytes and far-copy chunks
                        #pragma unroll
                        for (int h = 0; h < X5_TPL; h++)
                            if (ch == uint32_t(h)) {
                                btot = __builtin_amdgcn_readlane(inc[h], (cut - 1u) & 63u);
                                ntot = __builtin_amdgcn_readlane(fce[h], (cut - 1u) & 63u);
                            }
                        bool inb[X5_TPL], lit[X5_TPL], cp[X5_TPL], far[X5_TPL];
                        bool bad = false;
                        #pragma unroll
                        for (int h = 0; h < X5_TPL; h++) {
                            inb[h] = take[h] && 64u * uint32_t(h) + uint32_t(lane) < cut;
                            lit[h] = inb[h] && kd[h] == 0;
                            cp[h] = inb[h] && kd[h] != 0;
                            far[h] = cp[h] && farc[h];
                            bad = bad || (cp[h] && (off[h] == 0 || off[h] > otok[h] - out_start));
                            // a far source straddling the direct split (level bytes | values) is not one window
                            bad = bad || (od.dd != nullptr && far[h] && a[h] < od.dlo && a[h] + ol[h] > od.dlo);
                        }
                        if (__any(bad)) ok = false;
                        X5T(1);   // token decode, chain checks, cuts
                        if (ok) {
                            // far-copy sources: each copy's lane writes the addresses of its nch aligned chunks
                            // (which end with the chunk holding the source's last byte, inside the arena) into
                            // the batch's chunk address table, at its chunk base on; then lane l loads chunk l
                            // (and 64 + l) straight into the chunk buffer by LDS-DMA, so the lane-linear destination
                            // is the packed layout. The table lies in the bytes the loads overwrite: both table
                            // reads are issued before the first load. The loads are waited for only before the
                            // barrier, after the descriptors (no data registers, latency behind them).
                            if (ntot) {
                                uint64_t* ca = reinterpret_cast<uint64_t*>(FS + b * X5_FSL);
                                uint64_t fb0v[X5_TPL];
                                #pragma unroll
                                for (int h = 0; h < X5_TPL; h++) {
                                    const uint64_t fb0 = reinterpret_cast<uintptr_t>((fdd[h] ? od.dd : gdst) + a[h]) & ~uintptr_t(15);
                                    fb0v[h] = fb0;
                                }
                                // Every far copy writes entries cb0 .. cb0 + 4 (up to cb0 + 2, or cb0 alone, when no copy
                                // among the tokens takes more chunks than that), the highest first: an entry past a copy's own nch belongs to a later copy, which writes it with a
                                // smaller i, so later (one wave's LDS operations run in order), and the right address
                                // stays. cb0 + 4 < X5_FCH + 4 entries: inside the batch's chunk bytes (8 (X5_FCH + 4) <=
                                // 16 X5_FCH); entries at or past the batch's total are not used.
                                #pragma unroll
                                for (int i = 4; i >= 0; i--) {
                                    if ((i >= 3 && !wide4) || (i >= 1 && !wide2)) continue;
                                    #pragma unroll
                                    for (int h = 0; h < X5_TPL; h++)
                                        if (far[h]) ca[fce[h] - nch[h] + uint32_t(i)] = fb0v[h] + 16u * uint32_t(i);
                                }
                                x5_order();
                                const uint32_t l0 = uint32_t(lane);
                                uint64_t s0a = ca[l0];   // (entries at or past ntot: stale, not used)
                                uint64_t s1a = 0;
                                if constexpr (X5_FCH > 64u)
                                    if (ntot > 64u) s1a = ca[64u + l0];
                                asm volatile("" : "+v"(s0a), "+v"(s1a) :: "memory");   // both reads before the first load
                                uint8_t* chunks = FS + b * X5_FSL;
                                const uint32_t sl0 = __builtin_amdgcn_readfirstlane(uint32_t(reinterpret_cast<uintptr_t>(chunks)));
                                if (l0 < ntot) x5_dma16(s0a, sl0);
                                if constexpr (X5_FCH > 64u)
                                    if (ntot > 64u && l0 + 64u < ntot) x5_dma16(s1a, sl0 + 1024u);
                            }
                            X5T(2);   // far-copy source loads (issued)
                            if (lane < int(X5_W)) SB[b][lane] = 0;
                            #pragma unroll
                            for (int h = 0; h < X5_TPL; h++) {
                                const uint32_t relS = otok[h] - (op & ~3u);   // from the batch's aligned base
                                uint32_t d0 = 0, d1 = 0;
                                if (inb[h]) {
                                    const bool near = cp[h] && !far[h];
                                    d0 = relS | (near ? (X5_CP | (off[h] << 16)) : 0u);
                                    d1 = near ? uint32_t(65536.0f * __builtin_amdgcn_rcpf(float(off[h]))) + 1u
                                              : (lit[h] ? stg_off + woff + (srcv[h] - I) - relS
                                                        : FSB + b * X5_FSL + 16u * (fce[h] - nch[h]) + fsh[h] - relS);
                                }
                                D[b][1 + 64 * h + lane] = d0;
                                D[b][1 + X5_DS + 64 * h + lane] = d1;
                                x5_order();
                                if (inb[h]) atomicOr(&SB[b][relS >> 5], 1u << (relS & 31u));
                            }
                            x5_order();
                            const uint32_t c = lane < int(X5_W) ? __popc(SB[b][lane]) : 0u;
                            const uint32_t e2 = dpp_incl_scan(c) - c;
                            if (lane < int(X5_W)) WP[b][lane] = e2;
                            kind = R5_NORMAL;
                            b_tot = btot;
                            nops = 0;
                        }
                    }
                    if (ok && used) {
                        op += b_tot;
                        const uint32_t uh = (used - 1u) >> 6;
                        #pragma unroll
                        for (int h = 0; h < X5_TPL; h++)
                            if (uh == uint32_t(h)) ip = __builtin_amdgcn_readlane(endp[h], (used - 1u) & 63u);
                        sb += used;
                    }
                }
            }
            if (!ok && kind != R5_END) kind = R5_BAD;
            if (lane == 0) {
                REC[b][0] = kind;
                REC[b][1] = b_op;
                REC[b][2] = b_tot;
                REC[b][3] = b_s0;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // far-copy chunks landed in LDS
            X5T(3);   // descriptors, token-start words, far-copy loads landed
            k_m2 = k_m1;
            k_m1 = kind;
            ops_m1 = b_op;
        } else if (it > 0) {
            // ---------------- consumer: batch it-1 from buffer b ^ 1
            const uint32_t pb = b ^ 1u;
            const uint32_t kind = __builtin_amdgcn_readfirstlane(REC[pb][0]);
            const uint32_t s0 = __builtin_amdgcn_readfirstlane(REC[pb][1]);
            const uint32_t btot = __builtin_amdgcn_readfirstlane(REC[pb][2]);
            if (kind == R5_NORMAL) {
                // 256-byte windows from the aligned base Sb = s0 & ~3, four consecutive bytes a lane; the
                // al = s0 & 3 bytes before s0 belong to the previous batch (read, never written)
                const uint32_t al = s0 & 3u;
                const uint32_t Sb = s0 - al;
                const uint32_t btS = btot + al;
                const uint32_t* sbw = SB[pb];
                const uint32_t* wpw = WP[pb];
                const uint32_t* Dp = D[pb];
                for (uint32_t w0 = 0; w0 < btS; w0 += 256) {
                    const uint32_t x0 = w0 + 4u * uint32_t(lane);
                    const uint32_t ws = w0 == 0 ? al : w0;   // sources at or past ws are resolved in the window
                    const uint32_t wd = x0 >> 5, sh = x0 & 31u;
                    const uint32_t sbv = sbw[wd];
                    const uint32_t t0 = wpw[wd] + __popc(sbv & ((2u << sh) - 1u));   // entry of byte x0
                    const uint32_t nb = sbv >> sh;
                    uint32_t tk[4];
                    tk[0] = t0;
                    tk[1] = t0 + ((nb >> 1) & 1u);
                    tk[2] = tk[1] + ((nb >> 2) & 1u);
                    tk[3] = tk[2] + ((nb >> 3) & 1u);
                    uint32_t d0[4], d1[4];
                    #pragma unroll
                    for (int u = 0; u < 4; u++) {
                        d0[u] = Dp[tk[u]];
                        d1[u] = Dp[tk[u] + X5_DS];
                    }
                    uint32_t addr[4], pw[4];
                    bool pend[4];
                    #pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t x = x0 + uint32_t(u);
                        const uint32_t jj = x - (d0[u] & 0xffffu);
                        const bool cp = int32_t(d0[u]) < 0;
                        const uint32_t q = __umul24(jj, d1[u]) >> 16;        // floor(jj / offset) (copies)
                        const uint32_t of = (d0[u] >> 16) & 0x7fffu;
                        uint32_t t;   // of * q + of, kept a 24-bit multiply (the compiler folds it into v_mad_u64_u32)
                        asm("v_mad_u32_u24 %0, %1, %2, %1" : "=v"(t) : "v"(of), "v"(q));
                        const uint32_t y = x - t;                            // a copy's source (from Sb; may wrap)
                        pend[u] = cp && int32_t(y) >= int32_t(ws);
                        addr[u] = cp ? ((Sb + y) & XRMASK) : (d1[u] + x);
                        // (bits above the window's 8 stay in the word: the rounds mask the address with 0x1fe)
                        pw[u] = 0x8000u | (y << 1);
                    }
                    // the four source reads issued together (every addr is inside the workgroup's LDS)
                    uint32_t vv[4];
                    #pragma unroll
                    for (int u = 0; u < 4; u++) vv[u] = uint32_t(*reinterpret_cast<const __attribute__((address_space(3))) uint8_t*>(size_t(Lb + addr[u])));
                    asm volatile("" : "+v"(vv[0]), "+v"(vv[1]), "+v"(vv[2]), "+v"(vv[3]));
                    // jump words, two per dword: (value << 1), or 0x8000 | (window position << 1) while pending
                    uint32_t Wa = (pend[0] ? pw[0] : (vv[0] << 1)) | ((pend[1] ? pw[1] : (vv[1] << 1)) << 16);
                    uint32_t Wb = (pend[2] ? pw[2] : (vv[2] << 1)) | ((pend[3] ? pw[3] : (vv[3] << 1)) << 16);
                    while (__any(((Wa | Wb) & 0x80008000u) != 0u)) {
                        *reinterpret_cast<uint2*>(jvb + 8u * uint32_t(lane)) = make_uint2(Wa, Wb);
                        const uint32_t g0 = *reinterpret_cast<const uint16_t*>(jvb + (Wa & 0x1feu));
                        const uint32_t g1 = *reinterpret_cast<const uint16_t*>(jvb + ((Wa >> 16) & 0x1feu));
                        const uint32_t g2 = *reinterpret_cast<const uint16_t*>(jvb + (Wb & 0x1feu));
                        const uint32_t g3 = *reinterpret_cast<const uint16_t*>(jvb + ((Wb >> 16) & 0x1feu));
                        const uint32_t ga = __builtin_amdgcn_perm(g1, g0, 0x05040100u), gb = __builtin_amdgcn_perm(g3, g2, 0x05040100u);
                        Wa = x5_pick(Wa, ga);
                        Wb = x5_pick(Wb, gb);
                    }
                    const uint32_t o4 = __builtin_amdgcn_perm(Wb >> 1, Wa >> 1, 0x06040200u);
                    if (x0 < btS) {
                        const uint32_t ra = (Sb + x0) & XRMASK;
                        if (x0 >= al) {   // (a dword past the batch end writes <= 3 bytes the next batch rewrites)
                            *reinterpret_cast<uint32_t*>(ring + ra) = o4;
                        } else {          // the batch's first dword: only bytes from s0 on
                            #pragma unroll
                            for (uint32_t u = 1; u < 4; u++)
                                if (u >= al) ring[ra + u] = uint8_t(o4 >> (8u * u));
                        }
                    }
                }
                X5T(6);   // windows
                flush_slots(ring, od, F, s0 + btot, lane);
                cop = s0 + btot;
                X5T(7);   // flush
                asm volatile("s_waitcnt vmcnt(1)" ::: "memory");   // all but the newest store have landed
                X5T(8);   // store drain
            } else if (kind == R5_LONG) {
                // bytes [s0, s0 + btot) = input [sl, sl + btot): whole 16-byte ring blocks from 16-byte loads,
                // the partial first / last block byte by byte
                const uint32_t sl = __builtin_amdgcn_readfirstlane(REC[pb][3]);
                const uint32_t e = s0 + btot;
                for (uint32_t base = s0 & ~15u; base < e; base += XLIT) {
                    const uint32_t p = base + 16u * uint32_t(lane);   // this lane's block
                    if (p < e) {
                        if (p >= s0 && p + 16u <= e) {
                            *reinterpret_cast<u32x4*>(ring + (p & XRMASK)) = x5_load16(gin, sl + (p - s0));
                        } else {
                            for (uint32_t q = max(p, s0); q < min(p + 16u, e); q++) ring[q & XRMASK] = gin[sl + (q - s0)];
                        }
                    }
                    flush_slots(ring, od, F, min(base + XLIT, e), lane);
                }
                cop = e;
                wait_vmem();
            } else {
                wait_vmem();
            }
        }
        X5T(9);   // (long literal / empty batch)
        x5_barrier();
        if (wv == 0) X5T(4); else X5T(10);   // barrier wait
        last = __builtin_amdgcn_readfirstlane(REC[b][0]);
        if (last >= R5_END) break;
    }
    if (last == R5_BAD) {
        if (threadIdx.x == 0) atomicMax(&fb[j], whole ? FB_SERIAL : FB_REDO);
        return;
    }
    if (wv == 1) {   // tail: bytes [F, cop)
        for (uint32_t a = F + uint32_t(lane) * 16u; a + 16u <= cop; a += 1024u)
            put16(od, a, *reinterpret_cast<const u32x4*>(ring + (a & XRMASK)));
        for (uint32_t a = F + ((cop - F) & ~15u) + uint32_t(lane); a < cop; a += 64) put1(od, a, ring[a & XRMASK]);
    }
#undef X5T
}

// One workgroup per item: mode 0 = a 64 KiB piece (pieces[blockIdx.x]), mode 1 = a whole-page redo.
__global__ __launch_bounds__(128) void k_snappy_exec5(const SnappyJob* __restrict__ jobs, const int2* __restrict__ pieces,
                                                      const uint32_t* __restrict__ splits, int* __restrict__ fb, int mode) {
    __shared__ X5Lds S;
    __shared__ __attribute__((aligned(16))) uint8_t FS[2 * X5_FSL];   // far-copy source chunks of two batches
    exec5_piece(S, FS, jobs, pieces, splits, fb, mode, int(blockIdx.x));
}

// Execute stage, after launch_snappy_parse (pf_snappy_parse.hip): the pieces, the whole-page redo, the serial kernel.
void launch_snappy_exec(const SnappyJob* d_jobs, int n_jobs, const int2* d_pieces, int n_pieces, uint32_t* d_splits,
                        int* d_fb, DevChunkResult* d_res, int exec, hipStream_t s) {
    if (n_jobs <= 0) return;
    // exec (PfOpts; the diagnostics build's PF_EXEC): 5 = producer / consumer waves (default), 2 = one wave
    // per piece (pf_snappy_exec2.hip). The whole-page redo is always the same kernel's mode 1.
#ifdef PF_DIAG
    if (exec == 2) {
        launch_snappy_exec2(d_jobs, n_jobs, d_pieces, n_pieces, d_splits, d_fb, s);
    } else
#else
    (void)exec;
#endif
    {
        hipLaunchKernelGGL(k_snappy_exec5, dim3(n_pieces), dim3(128), 0, s, d_jobs, d_pieces, (const uint32_t*)d_splits, d_fb, 0);
        hipLaunchKernelGGL(k_snappy_exec5, dim3(n_jobs), dim3(128), 0, s, d_jobs, d_pieces, (const uint32_t*)d_splits, d_fb, 1);
    }
    launch_snappy_serial(d_jobs, n_jobs, d_fb, d_res, s);
}

// All Snappy work of one batch, in stream order. fb must be zero on entry.
void launch_snappy(const SnappyJob* d_jobs, int n_jobs, const int2* d_wins, int n_wins, SnapWin* d_win,
                   SnapEnt* d_ent, uint32_t* d_lane_out, const int2* d_pieces, int n_pieces, uint32_t* d_splits,
                   int* d_fb, DevChunkResult* d_res, int max_nwin, int exec, hipStream_t s) {
    launch_snappy_parse(d_jobs, n_jobs, d_wins, n_wins, d_win, d_ent, d_lane_out, d_splits, d_fb, max_nwin, s);
    launch_snappy_exec(d_jobs, n_jobs, d_pieces, n_pieces, d_splits, d_fb, d_res, exec, s);
}

}  // namespace pf
