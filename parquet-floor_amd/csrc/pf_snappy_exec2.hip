// pf_snappy_exec2.hip — diagnostics build only: k_snappy_exec2, the one-wave Snappy executor (PF_EXEC=2).
//
// The executor the production one (k_snappy_exec5, pf_snappy_exec.hip) is tested against, with the same
// contract: one launch over the 64 KiB pieces (mode 0), one over the pages to redo as a whole (mode 1,
// FB_REDO); input is the parse stage's token-start bitmap and split points, output goes through OutDst
// (pf_snappy_exec.h), and anything wrong in the stream escalates the job's flag to FB_REDO or FB_SERIAL.
//
// One wave per piece. The token starts of XCHUNK staged input bytes are enumerated from the bitmap, and up
// to 64 tokens, one per lane, are decoded together (output offsets by a DPP scan; each token must start
// where the one before it ends). The step is cut before the first token that is longer than 64 output
// bytes (a long literal: copied from HBM on its own), that passes XBATCH output bytes, that is a literal
// not wholly staged, or that is the step's (XFAR + 1)-th far copy: a copy whose source the ring no longer
// holds, loaded from the already written output into its LDS slot once the flush's stores have landed.
//
// Every output byte of a step is then produced by one byte-lane pass: the step's output is walked in
// windows of 256 bytes, lane x owning bytes w0 + 64u + x (u < 4). A byte's token comes from the step's
// token-start bitmap (word prefix counts + popcount), the token's packed descriptor from the
// token's lane (ds_bpermute, no LDS table), and its source is
//   a literal byte (staged input) or a far-copy byte (prefetched source slot): one LDS read;
//   a copy byte whose source precedes the window: one ring read (earlier windows of the same
//     step are already in the ring: single wave, LDS operations execute in order);
//   a copy byte whose source lies in the same window (dependent copies, self-overlapping runs):
//     resolved across the lanes by pointer jumping on a {pending, window position | value} word
//     (one LDS round trip per round; a source always precedes its reader).
// Self-overlapping copies read source byte (j mod offset), so a run never chains through itself.
// Dependent copies therefore cost a few rounds per window instead of one serial read-then-write
// per token.
#ifdef PF_DIAG
#include <hip/hip_runtime.h>

#include "pf_launch.h"
#include "pf_snappy_exec.h"

namespace pf {

#ifndef PF_XBATCH
#define PF_XBATCH 1024
#endif
constexpr uint32_t XBATCH = PF_XBATCH;   // output bytes of one parallel step (ring: XBATCH + XSLOT <= XRING)
constexpr uint32_t FBUF_W = 17;      // dwords per far copy's source slot (64 bytes + misalignment)
#ifndef PF_XFAR
#define PF_XFAR 24
#endif
constexpr uint32_t XFAR = PF_XFAR;   // far copies per step (the step is cut before the next one)

// x mod d for 0 <= x < 64, 1 <= d <= 64 ((x + 0.5) / d is never within 1/128 of an integer).
__device__ __forceinline__ uint32_t mod_small(uint32_t x, uint32_t d) {
    const uint32_t q = uint32_t((float(x) + 0.5f) * __builtin_amdgcn_rcpf(float(d)));
    return x - q * d;
}

__device__ __forceinline__ uint64_t lane_mask_lt(uint32_t k) { return k >= 64 ? ~0ull : ((1ull << k) - 1ull); }

__device__ __forceinline__ void wait_vmem_last_slot() {   // all but the last flush slot's XST stores
    if constexpr (XST == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
}

constexpr uint32_t X2_STAGE_OFF = XRING;                            // [ring | stage | far slots] in one LDS array,
constexpr uint32_t X2_FBUF_OFF = XRING + ((XSTAGE + 15u) & ~15u);   // so one byte address selects any source
constexpr uint32_t X2_LDS = X2_FBUF_OFF + XFAR * FBUF_W * 4;
enum : uint32_t { X2_LDSADDR = 0, X2_COPY = 1 };

__global__ __launch_bounds__(64) void k_snappy_exec2(const SnappyJob* __restrict__ jobs, const int2* __restrict__ pieces,
                                                     const uint32_t* __restrict__ splits, int* __restrict__ fb, int mode) {
    __shared__ __attribute__((aligned(16))) uint8_t L[X2_LDS];
    __shared__ uint16_t tokpos[XCHUNK / 2];
    __shared__ uint32_t sbits[XBATCH / 32];                               // token starts of the step's output
    __shared__ uint32_t wpre[XBATCH / 32];                                // tokens starting in earlier words
    __shared__ uint16_t jv[256];                                          // pointer-jumping words of a window
    uint8_t* const ring = L;
    uint8_t* const stage = L + X2_STAGE_OFF;
    uint32_t* const fbuf = reinterpret_cast<uint32_t*>(L + X2_FBUF_OFF);
    const int lane = threadIdx.x;
    int j, k;
    if (mode == 0) {
        const int2 pc = pieces[blockIdx.x];
        j = pc.x;
        k = pc.y;
    } else {
        j = blockIdx.x;
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
    uint8_t* dst = job.dst;
    const uint64_t n = job.src_len;
    const uint32_t* sp = splits + job.split_base;
    uint64_t pos0 = 0, ulen = 0;
    if (!uvarint(in, n, pos0, ulen) || ulen != job.dst_len) {
        if (lane == 0) atomicMax(&fb[j], FB_SERIAL);
        return;
    }
    if (mode == 0 && (job.dflags & 1u)) {   // diagnostics: forced redo
        if (lane == 0) atomicMax(&fb[j], FB_REDO);
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
    PF_GLOBAL uint8_t* gdst = gptr(dst);
    const OutDst od{gdst, mode == 0 ? gptr(job.ddst) : nullptr, job.dlo, job.dgran};
    uint32_t op = out_start, F = out_start;
    uint32_t nst = 0;   // store instructions issued by the last flush (still possibly in flight)
    bool bad = false;
    while (op < out_end && !bad) {
        if (ip >= n) { bad = true; break; }
        const uint32_t I = ip & ~15u;
        __syncthreads();
        const uint32_t woff = snap_stage(stage, in, n, I, XSTAGE, lane);
        // token starts in [ip, I + XCHUNK): 16 input bytes per lane
        const uint32_t p16 = I + 16u * uint32_t(lane);
        uint32_t bits = uint64_t(p16) < n ? uint32_t(tm16[p16 >> 4]) : 0u;
        if (p16 + 16u <= ip) bits = 0;
        else if (p16 < ip) bits &= ~((1u << (ip - p16)) - 1u);
        const uint32_t cnt = __popc(bits);
        const uint32_t ex = dpp_incl_scan(cnt);
        const uint32_t T = __builtin_amdgcn_readlane(ex, 63);
        uint32_t q = ex - cnt;
        while (bits) {
            const uint32_t b = uint32_t(__ffs(bits) - 1);
            bits &= bits - 1;
            tokpos[q++] = uint16_t(16u * uint32_t(lane) + b);
        }
        nst = 0;   // the bitmap loads above waited for every earlier store
        __syncthreads();
        if (T == 0) { bad = true; break; }
        uint32_t sb = 0;
        while (sb < T && op < out_end) {
            const uint32_t t = sb + uint32_t(lane);
            const bool v = t < T;
            const uint32_t pos = v ? uint32_t(tokpos[t]) : 0u;
            const SnapTok tk = snap_tok(lds_read8(stage, woff + pos));
            const uint32_t ol = v ? tk.ol : 0u;
            const uint32_t start = I + pos;
            const uint32_t endp = tk.tl > uint64_t(0xffffffffu - start) ? 0xffffffffu : start + uint32_t(tk.tl);
            const uint32_t prev = dpp_prev(endp);
            const uint32_t inc = dpp_incl_scan(ol);
            const uint32_t otok = op + inc - ol;
            const bool take = v && otok < out_end;
            const int nt = __popcll(__ballot(take));
            const bool wrong = take && ((lane == 0 ? start != ip : start != prev) || endp > n || op + inc > out_end ||
                                        inc < ol);
            if (__any(wrong)) { bad = true; break; }
            if (nt == 0) break;   // the previous step ended exactly at out_end
            const uint32_t kd = tk.kind;
            const uint32_t off = tk.arg;
            const uint32_t srcv = start + tk.arg;   // literal data position
            const bool lstaged = srcv + ol <= I + XCHUNK + 64;
            const uint32_t a = otok - off;                       // copy source start
            const bool farc = take && kd != 0 && a + min(ol, off) <= op && int32_t(a - (op + XBATCH - XRING)) < 0;
            const unsigned long long farm = __ballot(farc);
            const uint32_t frank = uint32_t(__popcll(farm & lane_mask_lt(uint32_t(lane))));
            const unsigned long long cutm = __ballot(take && (ol > 64u || inc > XBATCH || (kd == 0 && !lstaged) ||
                                                              (farc && frank >= XFAR)));
            const uint32_t cut = cutm ? uint32_t(__ffsll(cutm) - 1) : uint32_t(nt);
            uint32_t used, btot;
            if (cut == 0) {
                // one literal, from HBM (copies are <= 64 bytes, so only a literal gets here)
                const uint32_t L0 = __builtin_amdgcn_readfirstlane(ol);
                const uint32_t s0 = __builtin_amdgcn_readfirstlane(srcv);
                if (__builtin_amdgcn_readfirstlane(kd) != 0) { bad = true; break; }
                uint32_t fl_slots = 0;
                for (uint32_t d0 = 0; d0 < L0; d0 += XLIT) {
                    const uint32_t c = min(L0 - d0, XLIT);
                    const uint32_t b0 = uint32_t(lane) * 16u;
                    if (b0 < c) {
                        uint8_t by[16];
                        #pragma unroll
                        for (int u = 0; u < 16; u++) by[u] = b0 + u < c ? gin[s0 + d0 + b0 + u] : uint8_t(0);
                        #pragma unroll
                        for (int u = 0; u < 16; u++)
                            if (b0 + u < c) ring[(op + d0 + b0 + u) & XRMASK] = by[u];
                    }
                    fl_slots += flush_slots(ring, od, F, op + d0 + c, lane);
                }
                nst = fl_slots;
                used = 1;
                btot = L0;
            } else {
                used = cut;
                btot = __builtin_amdgcn_readlane(inc, cut - 1);
                const bool inb = take && uint32_t(lane) < cut;
                const bool lit = inb && kd == 0;
                const bool cp = inb && kd != 0;
                if (__any(cp && (off == 0 || off > otok - out_start))) { bad = true; break; }
                const bool far = cp && farc;
                // a far source straddling the direct split (level bytes | values) is not one window
                if (od.dd != nullptr && __any(far && a < od.dlo && a + ol > od.dlo)) { bad = true; break; }
                // far copies: their source (flushed output) into this token's LDS slot
                if (__any(far)) {
                    if (nst == XST) wait_vmem_last_slot();   // all but the last slot's stores have landed
                    else wait_vmem();
                    if (far) {
                        const PF_GLOBAL uint8_t* fb0 = od.dd != nullptr && a >= od.dlo ? od.dd + a : gdst + a;
                        const uintptr_t fa = reinterpret_cast<uintptr_t>(fb0);
                        const PF_GLOBAL uint32_t* fsrc = (const PF_GLOBAL uint32_t*)(fa & ~uintptr_t(3));
                        const uint32_t nwd = (uint32_t(fa & 3u) + ol + 3u) >> 2;
                        uint32_t fw[FBUF_W];
                        #pragma unroll
                        for (int u = 0; u < int(FBUF_W); u++) fw[u] = uint32_t(u) < nwd ? fsrc[u] : 0u;
                        uint32_t* fl = fbuf + frank * FBUF_W;
                        #pragma unroll
                        for (int u = 0; u < int(FBUF_W); u++)
                            if (uint32_t(u) < nwd) fl[u] = fw[u];
                    }
                }
                // packed token descriptor, read by the byte lanes with ds_bpermute:
                //   d0 = rel (11 bits) | kind (1 bit, 11) | self-overlap (bit 12) | offset << 16
                //   d1 = LDS byte address of the token's first source byte (literal / far copy) or the
                //        absolute output position of its source (near copy)
                const uint32_t rel = otok - op;
                uint32_t d0 = 0, d1 = 0;
                if (inb) {
                    const bool near = cp && !far;
                    d0 = rel | ((near ? X2_COPY : X2_LDSADDR) << 11) | ((near && off < ol) ? (1u << 12) : 0u) |
                         (min(off, 0xffffu) << 16);
                    const uint32_t fsh = od.dd != nullptr && a >= od.dlo
                                             ? uint32_t((reinterpret_cast<uintptr_t>(od.dd) + a) & 3u) : (a & 3u);
                    d1 = lit ? X2_STAGE_OFF + woff + (srcv - I)
                             : (far ? X2_FBUF_OFF + frank * (FBUF_W * 4) + fsh : a);
                }
                if (lane < int(XBATCH / 32)) sbits[lane] = 0;
                __syncthreads();
                if (inb) atomicOr(&sbits[rel >> 5], 1u << (rel & 31u));
                __syncthreads();
                {
                    const uint32_t c = lane < int(XBATCH / 32) ? __popc(sbits[lane]) : 0u;
                    const uint32_t e2 = dpp_incl_scan(c) - c;
                    if (lane < int(XBATCH / 32)) wpre[lane] = e2;
                }
                __syncthreads();
                // 256-byte windows: lane L owns bytes w0 + 64u + L (u < 4). A byte's word is its value
                // (< 0x100) or 0x100 | p: "same as window byte p" (p < its own position).
                for (uint32_t w0 = 0; w0 < btot; w0 += 256) {
                    const uint32_t s0 = op + w0;
                    // straight-line phases over the four slots (no branches: the compiler keeps the four
                    // chains of LDS operations in flight together)
                    uint32_t W[4], xw[4], ti[4], i0[4], i1[4], addr[4];
                    bool act[4], pend[4];
                    #pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t x = w0 + 64u * uint32_t(u) + uint32_t(lane);
                        act[u] = x < btot;
                        xw[u] = act[u] ? x : btot - 1u;
                    }
                    #pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t wd = xw[u] >> 5;
                        ti[u] = wpre[wd] + __popc(sbits[wd] & ((2u << (xw[u] & 31u)) - 1u)) - 1u;
                    }
                    #pragma unroll
                    for (int u = 0; u < 4; u++) {
                        i0[u] = uint32_t(__builtin_amdgcn_ds_bpermute(int(ti[u] << 2), int(d0)));
                        i1[u] = uint32_t(__builtin_amdgcn_ds_bpermute(int(ti[u] << 2), int(d1)));
                    }
                    #pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t jj = xw[u] - (i0[u] & 0x7ffu);
                        const bool copy = ((i0[u] >> 11) & 1u) == X2_COPY;
                        const uint32_t offv = max(i0[u] >> 16, 1u);
                        const uint32_t r = (i0[u] & (1u << 12)) ? mod_small(jj & 63u, offv) : jj;
                        const uint32_t y = i1[u] + r;                 // copy: absolute output position of the source byte
                        pend[u] = act[u] && copy && y >= s0;          // produced in this window
                        addr[u] = copy ? (y & XRMASK) : (i1[u] + jj);
                        W[u] = 0x100u | ((y - s0) & 0xffu);
                    }
                    #pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t v = uint32_t(L[addr[u]]);
                        W[u] = pend[u] ? W[u] : (act[u] ? v : 0u);
                    }
                    // pointer jumping over the window's 256 bytes (a source always precedes its reader):
                    // every round publishes the window's words to LDS (byte x of the window at jv[x]) and
                    // each pending byte takes the word it points at. A single wave's LDS operations run in
                    // order, so the reads see this round's writes; one LDS read per byte and round instead
                    // of two permutes plus the half-word selects (~20 instead of ~60 VALU per round).
                    while (__any(((W[0] | W[1] | W[2] | W[3]) & 0x100u) != 0u)) {
                        #pragma unroll
                        for (int u = 0; u < 4; u++) jv[64u * uint32_t(u) + uint32_t(lane)] = uint16_t(W[u]);
                        uint32_t G[4];
                        #pragma unroll
                        for (int u = 0; u < 4; u++) G[u] = jv[W[u] & 0xffu];
                        #pragma unroll
                        for (int u = 0; u < 4; u++) W[u] = (W[u] & 0x100u) ? G[u] : W[u];
                    }
                    #pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (act[u]) ring[(s0 + 64u * uint32_t(u) + uint32_t(lane)) & XRMASK] = uint8_t(W[u]);
                }
                const uint32_t sl = flush_slots(ring, od, F, op + btot, lane);
                if (sl) nst = sl;
            }
            op += btot;
            ip = __builtin_amdgcn_readlane(endp, int(used) - 1);
            sb += used;
        }
    }
    if (bad) {
        if (lane == 0) atomicMax(&fb[j], whole ? FB_SERIAL : FB_REDO);
        return;
    }
    // tail: bytes [F, op)
    for (uint32_t a = F + uint32_t(lane) * 16u; a + 16u <= op; a += 1024u)
        put16(od, a, *reinterpret_cast<const u32x4*>(ring + (a & XRMASK)));
    for (uint32_t a = F + ((op - F) & ~15u) + uint32_t(lane); a < op; a += 64) put1(od, a, ring[a & XRMASK]);
}

// The pieces, then the whole-page redo of pages whose pieces were not independent (launch_snappy_exec, exec == 2).
void launch_snappy_exec2(const SnappyJob* d_jobs, int n_jobs, const int2* d_pieces, int n_pieces, const uint32_t* d_splits,
                         int* d_fb, hipStream_t s) {
    hipLaunchKernelGGL(k_snappy_exec2, dim3(n_pieces), dim3(64), 0, s, d_jobs, d_pieces, d_splits, d_fb, 0);
    hipLaunchKernelGGL(k_snappy_exec2, dim3(n_jobs), dim3(64), 0, s, d_jobs, d_pieces, d_splits, d_fb, 1);
}

}  // namespace pf
#endif  // PF_DIAG
