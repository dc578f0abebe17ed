// pf_snappy_parse.hip — K1, parse stage of the block-parallel Snappy decompressor: where every token starts.
//
// K1 replaces snappy-java's Snappy.uncompress behind the Hadoop codec shim
// (src/main/java/org/apache/hadoop/io/compress/DecompressorStream.java:61-70,101-173).
//
// Google Snappy (what snappy-java wraps) compresses in independent 64 KiB blocks: no copy reaches
// back across a block boundary and a token starts exactly at every multiple of 65536 of the output.
// A page therefore splits into 64 KiB pieces that decode independently, once the token chain is
// known. This unit finds the chain, with four kernels in stream order (launch_snappy_parse); the
// executor (pf_snappy_exec.hip) then decodes the pieces from the bitmap and the split points.
//
//   k_snappy_index  one wave per 8 KiB window of compressed input (all pages). Each lane walks the
//                   token chain of its 128-byte region from the region start (a guess: the true
//                   chain usually enters a little later). A scalar pass then follows the chain
//                   lane to lane from the window entry; a lane whose true entry is not on its
//                   guessed chain re-walks from it, until the chain is consistent (each round
//                   fixes at least the first wrong lane). Output: the token-start bitmap (1 bit per
//                   input byte), per-lane output byte counts, the window exit X, and the
//                   successor record: where the chain from X meets the next window's own chain
//                   (the chain from its start) and the output difference up to there, found by
//                   a two-pointer walk over IDX_EXT staged bytes past the window end.
//   k_snappy_chain  one wave per page. Window w's true entry is window w-1's exit: one record
//                   load per window (a walk in HBM for an entry the record does not answer, an
//                   exact whole-wave parse for windows neither resolves), repeated until the
//                   entries are consistent. Output: each window's true entry, merge point or exit,
//                   output bytes and WM_* mode.
//   k_snappy_repair one wave per window whose true entry is not its own chain's start: the bitmap
//                   and lane counts in front of the merge point (or of the whole window) are parsed
//                   again from the true entry; windows inside a literal are cleared.
//   k_snappy_splits one workgroup per page: the output total is checked against the page header and
//                   the input position of the token at each 64 KiB output boundary is found.
//
// A page whose stream breaks the block structure or is corrupt is flagged FB_SERIAL on the way and
// re-decoded by k_snappy_serial (pf_snappy.hip) — results never depend on the assumption.
#include <hip/hip_runtime.h>

#include "pf_launch.h"
#include "pf_snappy_par.h"
#include "pf_stamps.h"

namespace pf {

// Phase stamps of the parse kernels (tools/probe_parse_sf1.py).
#ifdef PF_STAMPS
PF_STAMP_TABLE(pf_cstamps, 40, pf_debug_cstamps)
#define CSTAMP(i, v) atomicAdd(&pf_cstamps[i], (unsigned long long)(v))
#else
#define CSTAMP(i, v) ((void)0)
#endif

// ======================================================================== index pass

struct WinLane {
    uint32_t b0, b1, b2, b3;   // token starts in the lane's region (bit i = input byte rs + i)
    uint32_t out;              // output bytes of those tokens
    uint32_t x;                // chain exit (first position >= region end), SNAP_INVALID past the stream
    uint32_t c;                // chain start
};

__device__ __forceinline__ void bit_set(WinLane& L, uint32_t i) {
    const uint32_t m = 1u << (i & 31u), w = i >> 5;
    L.b0 |= w == 0 ? m : 0u;
    L.b1 |= w == 1 ? m : 0u;
    L.b2 |= w == 2 ? m : 0u;
    L.b3 |= w == 3 ? m : 0u;
}
__device__ __forceinline__ void bit_clr(WinLane& L, uint32_t i) {
    const uint32_t m = 1u << (i & 31u), w = i >> 5;
    L.b0 &= w == 0 ? ~m : ~0u;
    L.b1 &= w == 1 ? ~m : ~0u;
    L.b2 &= w == 2 ? ~m : ~0u;
    L.b3 &= w == 3 ? ~m : ~0u;
}
__device__ __forceinline__ bool bit_get(const WinLane& L, uint32_t i) {
    const uint32_t w = i >> 5;
    const uint32_t v = w == 0 ? L.b0 : (w == 1 ? L.b1 : (w == 2 ? L.b2 : L.b3));
    return (v >> (i & 31u)) & 1u;
}

// ---- padded window stage: lane region k (input bytes [W0 + 128k, W0 + 128k + 140)) sits at
// sp + 140k, so 64 lanes reading the same offset of their own regions hit 64 different LDS banks
// (140 B = 35 dwords, odd) and an 8-byte token read at any region offset < 128 stays in the copy.
constexpr uint32_t SNAP_PB = 140;
constexpr uint32_t SNAP_PSTAGE = 64 * SNAP_PB;
constexpr uint32_t XS_SAT = 0x7fffu;       // saturated region exit (a literal longer than ~32 KiB)

// n >= 1. Dwords holding no stream byte are never read (zero instead).
__device__ void stage_pad(uint8_t* sp, const uint8_t* in, uint64_t n, uint32_t W0, int lane) {
    const uintptr_t base = reinterpret_cast<uintptr_t>(in);
    const uintptr_t lastw = (base + n - 1) & ~uintptr_t(3);
    constexpr uint32_t PU = 8;   // dwords a lane in flight before their stores (round 6: 35 serial round trips)
    for (uint32_t i0 = uint32_t(lane); i0 < SNAP_PSTAGE / 4; i0 += 64u * PU) {
        uint32_t lo[PU], hi[PU], sh[PU];
        #pragma unroll
        for (uint32_t u = 0; u < PU; u++) {
            const uint32_t idx = i0 + 64u * u;
            const uint32_t k = idx / (SNAP_PB / 4), jd = idx - k * (SNAP_PB / 4);
            const uintptr_t a = base + W0 + k * SNAP_RB + jd * 4;
            const uintptr_t a0 = a & ~uintptr_t(3);
            const bool in_range = idx < SNAP_PSTAGE / 4;
            lo[u] = in_range && a0 <= lastw ? *(const PF_GLOBAL uint32_t*)a0 : 0u;
            hi[u] = in_range && a0 + 4 <= lastw ? *(const PF_GLOBAL uint32_t*)(a0 + 4) : 0u;
            sh[u] = uint32_t(a & 3u);
        }
        #pragma unroll
        for (uint32_t u = 0; u < PU; u++) {
            const uint32_t idx = i0 + 64u * u;
            if (idx < SNAP_PSTAGE / 4) reinterpret_cast<uint32_t*>(sp)[idx] = __builtin_amdgcn_alignbyte(hi[u], lo[u], sh[u]);
        }
    }
}

// 8 stream bytes from window offset r (< 8 KiB) of a padded stage.
__device__ __forceinline__ uint64_t pad_read8(const uint8_t* sp, uint32_t r) {
    return lds_read8(sp, (r >> 7) * SNAP_PB + (r & 127u));
}

// Input / output bytes of the token at window offset r of a padded stage.
__device__ __forceinline__ uint64_t pad_tok(const uint8_t* sp, uint32_t r, uint32_t& ol) {
    const uint32_t a = (r >> 7) * SNAP_PB + (r & 127u);
    const uint32_t tag = (*reinterpret_cast<const uint32_t*>(sp + (a & ~3u)) >> (8u * (a & 3u))) & 0xffu;
    if (!tag_long(tag)) {
        ol = tag_ol(tag);
        return tag_tl(tag);
    }
    const SnapTok t = snap_tok(lds_read8(sp, a));
    ol = t.ol;
    return t.tl;
}

constexpr int WIN_ROUNDS = 66;       // lane-region fixed-point rounds: each fixes at least the first wrong lane,
                                     // so 64 + 1 always converge (seq_parse stays as a guard)

// Input / output bytes of the token at stage offset a (linear stage; tag decode unless a literal
// carries a length field).
__device__ __forceinline__ uint64_t stage_tok(const uint8_t* stage, uint32_t a, uint32_t& ol) {
    const uint32_t tag = stage[a];
    if (!tag_long(tag)) {
        ol = tag_ol(tag);
        return tag_tl(tag);
    }
    const SnapTok t = snap_tok(lds_read8(stage, a));
    ol = t.ol;
    return t.tl;
}

// Output / input bytes of the token whose tag and the 3 bytes after it are v: straight-line lengths (a literal
// length field of 4 bytes, >= 16 MiB, cannot be in a page: tl = 0xffffffff breaks the chain).
__device__ __forceinline__ void tok_lens(uint32_t v, uint32_t& ol, uint32_t& tl) {
    const uint32_t tag = v & 0xffu, kind = tag & 3u, Lv = tag >> 2;
    const uint32_t nb = Lv >= 60u ? Lv - 59u : 0u;
    const uint32_t lit_ol = (Lv < 60u ? Lv : ((v >> 8) & ((1u << (8u * min(nb, 3u))) - 1u))) + 1u;
    const uint32_t lit_tl = nb >= 4u ? 0xffffffffu : 1u + nb + lit_ol;
    // (selects as bit masks: v_bfi, where the compiler would branch on the kind)
    const uint32_t mlit = 0u - uint32_t(kind == 0u), m1 = 0u - uint32_t(kind == 1u);
    const uint32_t cp_ol = ((4u + (Lv & 7u)) & m1) | ((Lv + 1u) & ~m1);
    tl = (lit_tl & mlit) | (((0x05030200u >> (8u * kind)) & 0xffu) & ~mlit);
    ol = (lit_ol & mlit) | (cp_ol & ~mlit);
}

// The token at stream position p of a linear stage (base = stage offset of position 0): the tag and the 3
// bytes after it from one aligned dword pair.
__device__ __forceinline__ void walk_tok(const uint8_t* stage, uint32_t base, uint32_t p, uint32_t& ol, uint32_t& tl) {
    const uint32_t a = base + p;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(stage + (a & ~3u));
    tok_lens(__builtin_amdgcn_alignbyte(w[1], w[0], a & 3u), ol, tl);
}

// Walk the chain from c while positions stay below re (bits relative to rs). The token-start bits are
// OR-ed into the lane's four LDS words lb (one ds_or per token, no register selects; round 6) and read
// back into L at the end.
__device__ void lane_walk(const uint8_t* stage, uint32_t woff, uint32_t W0, uint64_t n, uint32_t rs, uint32_t re,
                          uint32_t c, WinLane& L, uint32_t* lb) {
    *reinterpret_cast<uint4*>(lb) = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t n32 = uint32_t(n);   // (< 2^32 - 1: 0xffffffff marks a broken chain)
    const uint32_t base = woff - W0;    // stage offset of stream position p: base + p
    uint32_t out = 0, p = c;
    L.c = c;
    while (p < re) {
        uint32_t ol, tl;
        walk_tok(stage, base, p, ol, tl);
        const uint32_t i = p - rs;
        atomicOr(lb + (i >> 5), 1u << (i & 31u));
        out = __builtin_elementwise_add_sat(out, ol);
        const uint32_t np = __builtin_elementwise_add_sat(p, tl);
        p = np > n32 ? 0xffffffffu : np;
    }
    const uint4 bv = *reinterpret_cast<const uint4*>(lb);
    L.b0 = bv.x; L.b1 = bv.y; L.b2 = bv.z; L.b3 = bv.w;
    L.out = out;
    L.x = p;   // (SNAP_INVALID when the chain ran past the stream end)
}

// Speculative parse of one window whose chain enters at `entry` (W0 <= entry < min(W0 + SNAP_WIN,
// n)), all 64 lanes, linear stage. Each lane walks the chain of its 128-byte region from the region
// start (a guess: chains started anywhere usually meet the true one within a few tokens); a scalar
// walk then follows the chain lane to lane from the entry, and a lane whose true entry is not on
// its guessed chain re-walks from it, until consistent (each round fixes at least the first wrong
// lane). Returns the window exit; flags = WIN_BROKEN if the chain runs past the stream end,
// WIN_NOCONV if max_rounds did not converge.
__device__ uint32_t win_parse_spec(const uint8_t* stage, uint32_t woff, uint32_t W0, uint64_t n, uint32_t entry,
                                   WinLane& L, uint32_t& flags, uint32_t* lbits, int max_rounds = WIN_ROUNDS) {
    const int lane = threadIdx.x & 63;
    uint32_t* const lb = lbits + 4 * lane;   // the lane's bit words (SNAP_WWORDS words of LDS for the wave)
    const uint32_t rs = W0 + uint32_t(lane) * SNAP_RB;
    const uint32_t re = uint32_t(min(uint64_t(rs) + SNAP_RB, n));
    entry = __builtin_amdgcn_readfirstlane(entry);
    const uint32_t L0 = (entry - W0) / SNAP_RB;
    L.b0 = L.b1 = L.b2 = L.b3 = 0;
    L.out = 0;
    L.c = rs;
    L.x = SNAP_INVALID;
    if (uint32_t(lane) >= L0 && uint64_t(rs) < n) lane_walk(stage, woff, W0, n, rs, re, uint32_t(lane) == L0 ? entry : rs, L, lb);
    uint32_t ent = SNAP_INVALID, X = SNAP_INVALID;
    bool converged = false;
    flags = 0;
    for (int round = 0; round < max_rounds; round++) {
        // follow the chain lane to lane. Fast-forward: while each lane's exit lands in the next lane's
        // region the entries are just the previous lanes' exits (one shuffle); from the first lane
        // where that fails, a uniform scalar walk.
        flags = 0;
        const uint32_t xk = L.x;
        const bool ok = uint32_t(lane) >= L0 && xk != SNAP_INVALID && uint64_t(xk) < n && xk < W0 + SNAP_WIN &&
                        (xk - W0) / SNAP_RB == uint32_t(lane) + 1;
        const uint64_t notok = ~__ballot(ok) & (~0ull << L0);
        const uint32_t la = notok ? uint32_t(__ffsll((unsigned long long)notok) - 1) : 63u;
        const uint32_t xprev = __shfl_up(xk, 1, 64);
        ent = uint32_t(lane) == L0 ? entry : ((uint32_t(lane) > L0 && uint32_t(lane) <= la) ? xprev : SNAP_INVALID);
        uint32_t k = la, e = __builtin_amdgcn_readlane(ent, int(la));
        for (;;) {
            ent = uint32_t(lane) == k ? e : ent;
            const uint32_t x = __builtin_amdgcn_readlane(L.x, int(k));
            if (x == SNAP_INVALID) { flags = WIN_BROKEN; X = SNAP_INVALID; break; }
            if (uint64_t(x) >= n || x >= W0 + SNAP_WIN) { X = x; break; }
            k = (x - W0) / SNAP_RB;
            e = x;
        }
        const bool need = ent != SNAP_INVALID && ent != L.c && !(ent > L.c && bit_get(L, ent - rs));
        if (!__any(need)) { converged = true; break; }
#ifdef PF_STAMPS
        if (lane == 0) { CSTAMP(7, 1); CSTAMP(8, __popcll(__ballot(need))); }
#else
        (void)__ballot(need);
#endif
        if (need) lane_walk(stage, woff, W0, n, rs, re, ent, L, lb);
    }
    if (!converged) flags = WIN_NOCONV;
    // lanes off the chain hold no tokens; drop the guessed prefix before a lane's true entry
    if (ent == SNAP_INVALID) {
        L.b0 = L.b1 = L.b2 = L.b3 = 0;
        L.out = 0;
    } else if (ent > L.c) {
        uint32_t p = L.c;
        while (p < ent) {
            uint32_t ol;
            const uint64_t tl = stage_tok(stage, woff + (p - W0), ol);
            bit_clr(L, p - rs);
            L.out -= ol;
            p += uint32_t(tl);
        }
        L.c = ent;
    }
    return X;
}

// Successor record (index pass -> chain pass). The chain pass asks, for window w + 1, where the chain from
// its true entry e meets the window's own chain (the one from its start W1) and what the two chains' outputs
// differ by up to there. Its first guess for e is window w's own exit X, usually the final answer, so the wave
// of window w, which has X in a register, answers that one question: row w + 1 of the entry arena holds
// {answer, X} in its first two SnapEnts (the rest of the row is never touched). No bitmap of window w + 1 is
// needed: its own chain is by definition the chain from W1, so two pointers p = X and q = W1, the one behind
// stepping one token at a time, meet at the first position of chain(X) that lies on chain(W1).
// The walk reads staged bytes only: the index stage reaches IDX_EXT bytes past the window end.
#ifndef PF_IDX_EXT   // (probe builds measure merge distances past the product's values with other ones)
#define PF_IDX_EXT 512
#endif
#ifndef PF_IDX_STEPS
#define PF_IDX_STEPS 384
#endif
constexpr uint32_t IDX_EXT = PF_IDX_EXT;
constexpr uint32_t IDX_STAGE = SNAP_WIN + IDX_EXT + 32;   // + alignment shift (< 16) + a token read's dword pair
constexpr uint32_t IDX_LDS = IDX_STAGE + SNAP_WWORDS * 4 + 64 * 4;   // k_snappy_index's static LDS
static_assert(IDX_EXT % 16 == 0 && IDX_EXT >= 64, "whole 16-byte chunks; seq_parse looks 64 positions ahead");
static_assert(IDX_EXT > 512 || IDX_LDS <= 10240, "k_snappy_index: 16 waves a CU need <= 10 KiB of LDS each");
constexpr int IDX_STEPS = PF_IDX_STEPS;   // tokens both pointers may take together; longer: ENT_SLOW (exact parse)
constexpr int DEEP_STEPS = 24;       // HBM token walks of the chain pass; longer: exact parse of the window
constexpr uint32_t ENT_POS = 0x3fffffffu;
enum : uint32_t { ENT_MERGE = 0, ENT_NOMERGE = 1, ENT_SLOW = 2, ENT_BAD = 3 };
constexpr uint32_t REC_NONE = SNAP_INVALID;   // record key that answers no entry (the chain pass walks in HBM)

__device__ __forceinline__ SnapEnt mk_ent(uint32_t pos, uint32_t flag, uint32_t out) {
    return SnapEnt{pos | (flag << 30), out};
}

// MERGE: pos = meeting point m, out = (true chain output in [e, m)) - (window chain output in
// [W1, m)), wrapping. NOMERGE (deep_walk only): the chain from e leaves the window first: pos = its exit,
// out = its output. SLOW: not resolved within the step cap. BAD: the chain from e runs past the stream end.
//
// Two-pointer walk for the entry X of the window at W1 (W1 <= X < wend1 = the window's end, X - W1 < IDX_EXT),
// uniform over the wave: every operand is wave-uniform and the token word goes through readfirstlane, so the
// lengths are computed on the scalar unit. key = X when `return` answers X; REC_NONE when the walk would need
// a byte at or past W1 + IDX_EXT or the stream end, or the chains meet outside the window (not classified
// here: deep_walk tells NOMERGE from BAD). A walk that runs out of staged bytes after the chain from X took
// DEEP_STEPS tokens answers SLOW like one that runs out of steps: deep_walk would give up on it too.
__device__ SnapEnt succ_walk(const uint8_t* stage, uint32_t base, uint32_t X, uint32_t W1, uint32_t wend1, uint32_t n32,
                             uint32_t& key, uint32_t& steps, uint32_t& need) {
    const uint32_t lim = min(W1 + IDX_EXT, n32);
    uint32_t p = X, q = W1, ap = 0, aq = 0, kp = 0;
    key = REC_NONE;
    need = 0;
    for (steps = 0;; steps++) {
        if (p == q) {
            if (p >= wend1) break;
            key = X;
            return mk_ent(p, ENT_MERGE, ap - aq);
        }
        const bool pb = p < q;
        const uint32_t lo = pb ? p : q;
        if (lo >= lim) {
            if (kp >= uint32_t(DEEP_STEPS)) key = X;
            break;
        }
        if (steps == uint32_t(IDX_STEPS)) {
            key = X;
            break;
        }
        const uint32_t a = base + lo;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(stage + (a & ~3u));
        const uint32_t w0 = __builtin_amdgcn_readfirstlane(w[0]), w1 = __builtin_amdgcn_readfirstlane(w[1]);
        uint32_t ol, tl;
        tok_lens(uint32_t(((uint64_t(w1) << 32) | w0) >> (8u * (a & 3u))), ol, tl);
        need = lo + 4u - W1;
        const uint32_t np = __builtin_elementwise_add_sat(lo, tl);
        if (np > n32) break;   // past the stream end
        if (pb) { p = np; ap += ol; kp++; } else { q = np; aq += ol; }
    }
    return mk_ent(X, ENT_SLOW, 0);
}

__device__ __forceinline__ uint32_t wave_sum_sat(uint32_t v) {
    uint64_t s = v;
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    return s > 0xffffffffull ? 0xffffffffu : uint32_t(s);
}

// Exact whole-wave parse of the chain from e (a token start, W0 <= e < stop) up to the first chain
// position >= stop, on a staged window. 64 lanes decode the token at cur + lane; the chain through
// those 64 candidates is followed in scalar registers (readlane) and its 64-bit start mask is
// OR-ed into sbits (bit i = W0 + i) by one lane. Afterwards every lane sums the output lengths of
// the tokens in its SNAP_RB region into slo. sbits must be zero on entry. Returns the exit
// (SNAP_INVALID if the chain runs past n) and the output byte total in `out`.
__device__ uint32_t seq_parse(const uint8_t* stage, uint32_t woff, uint32_t W0, uint64_t n, uint32_t e, uint64_t stop,
                              uint32_t* sbits, uint32_t* slo, uint32_t& out) {
    const int lane = threadIdx.x & 63;
    uint64_t cur = e;
    out = 0;
    bool bad = false;
    while (cur < stop) {
        const uint64_t q = cur + uint64_t(lane);
        const SnapTok t = snap_tok(lds_read8(stage, woff + uint32_t(q - W0)));
        const uint32_t tl = t.tl > 0x7fffffffull ? 0x7fffffffu : uint32_t(t.tl);
        const uint32_t lim = uint32_t(min<uint64_t>(64, stop - cur));
        uint32_t k = 0;
        uint64_t mask = 0;
        while (k < lim) {
            mask |= 1ull << k;
            k += __builtin_amdgcn_readlane(tl, k);
        }
        if (lane == 0) {
            const uint32_t r0 = uint32_t(cur - W0), wi = r0 >> 5, sh = r0 & 31u;
            sbits[wi] |= uint32_t(mask << sh);
            const uint32_t m1 = sh ? uint32_t(mask >> (32u - sh)) : uint32_t(mask >> 32);
            const uint32_t m2 = sh ? uint32_t(mask >> (64u - sh)) : 0u;
            if (m1 && wi + 1 < SNAP_WWORDS) sbits[wi + 1] |= m1;
            if (m2 && wi + 2 < SNAP_WWORDS) sbits[wi + 2] |= m2;
        }
        cur += k;
        if (cur > n) { bad = true; break; }
    }
    __syncthreads();
    // output bytes per lane region, from the marked tokens
    uint32_t acc = 0;
    #pragma unroll
    for (int kw = 0; kw < 4; kw++) {
        uint32_t m = sbits[lane * 4 + kw];
        while (m) {
            const uint32_t i = uint32_t(lane) * SNAP_RB + uint32_t(kw) * 32u + uint32_t(__ffs(m) - 1);
            m &= m - 1;
            const uint32_t o = snap_tok(lds_read8(stage, woff + i)).ol;
            acc = acc + o < acc ? 0xffffffffu : acc + o;
        }
    }
    slo[lane] = acc;
    if (bad) return SNAP_INVALID;
    out = wave_sum_sat(acc);
    return uint32_t(cur);
}

// Exact parse of the 8 KiB window at W0 whose chain enters at `entry` (W0 <= entry < min(W0 + 8 KiB,
// n)), all 64 lanes, lane k owning input region k. (1) Every offset i of the region is decoded as
// if a token started there: xs[i][k] = i + token length when that is inside the region, else the
// tagged offset the token ends at. (2) A backward pass turns this into the region exit of the
// chain from every offset (tokens are >= 2 bytes, so offsets i and i-1 never depend on each other:
// two per LDS round trip). Offsets at or past the stream end stop every chain (a chain stepping
// over n is broken). (3) The true chain crosses the regions with one lookup per region (offsets
// < 8 from registers). (4) Each lane walks the true chain through its region: token-start bits and
// output bytes. Returns the window exit (SNAP_INVALID: broken); a saturated exit falls back to the
// exact whole-wave parse on a linear stage (xs reused). sp must be staged (stage_pad) and synced.
__device__ uint32_t win_parse(const uint8_t* in, uint64_t n, uint32_t W0, uint32_t entry, const uint8_t* sp,
                              uint16_t* xs, uint32_t* sbits, uint32_t* slo, WinLane& L) {
    const int lane = threadIdx.x & 63;
    const uint32_t rs = W0 + uint32_t(lane) * SNAP_RB;
    const int64_t nrel = int64_t(n) - int64_t(rs);
    const uint8_t* mine = sp + uint32_t(lane) * SNAP_PB;
#ifdef PF_STAMPS
    unsigned long long pt0 = __builtin_amdgcn_s_memtime();
#define PT(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (lane == 0) CSTAMP(i, t_ - pt0); pt0 = t_; } while (0)
#else
#define PT(i) ((void)0)
#endif
    // (1) + (2), 8 offsets at a time from the region end: their tags (and literal length fields)
    // come from 4 LDS dwords; an exit inside the group is resolved in registers, one beyond it is
    // read from xs (final already)
    uint32_t c[8];
    for (int g = SNAP_RB / 8 - 1; g >= 0; g--) {
        const uint32_t* mw = reinterpret_cast<const uint32_t*>(mine) + 2 * g;
        const uint32_t d[4] = {mw[0], mw[1], mw[2], mw[3]};
        uint32_t tl[8];
        bool any_long = false;
        #pragma unroll
        for (int jj = 0; jj < 8; jj++) {
            const uint32_t tag = (d[jj >> 2] >> (8 * (jj & 3))) & 0xffu;
            tl[jj] = tag_tl(tag);
            any_long |= tag_long(tag);
        }
        if (__any(any_long)) {
            #pragma unroll
            for (int jj = 0; jj < 8; jj++) {
                const uint32_t tag = (d[jj >> 2] >> (8 * (jj & 3))) & 0xffu;
                const int q = (jj + 1) >> 2, sh = (jj + 1) & 3;
                const uint32_t b1 = __builtin_amdgcn_alignbyte(d[q + 1], d[q], uint32_t(sh));
                const uint32_t nb = (tag >> 2) - 59u;
                const uint32_t len = b1 & (nb >= 4u ? 0xffffffffu : (1u << (8u * nb)) - 1u);
                if (tag_long(tag)) tl[jj] = len >= XS_SAT ? XS_SAT : 2u + nb + len;
            }
        }
        uint32_t res[8];   // 0x8000 | exit offset, or an offset beyond the group to take the exit of
        #pragma unroll
        for (int jj = 7; jj >= 0; jj--) {
            const uint32_t i = uint32_t(8 * g + jj);
            const uint32_t nx = i + tl[jj];
            uint32_t r = nx >= SNAP_RB ? (0x8000u | min(nx, XS_SAT)) : nx;
            #pragma unroll
            for (int m = jj + 2; m < 8; m++) r = nx == uint32_t(8 * g + m) ? res[m] : r;
            if (int64_t(i) >= nrel) r = 0x8000u | i;
            res[jj] = r;
        }
        uint32_t rd[8];
        #pragma unroll
        for (int jj = 0; jj < 8; jj++) rd[jj] = xs[((res[jj] & 0x8000u) ? uint32_t(8 * g + jj) : res[jj]) * 64 + lane];
        #pragma unroll
        for (int jj = 0; jj < 8; jj++) {
            c[jj] = (res[jj] & 0x8000u) ? (res[jj] & 0x7fffu) : rd[jj];
            xs[(8 * g + jj) * 64 + lane] = uint16_t(c[jj]);
        }
    }
    PT(21);
    PT(22);
    // (3) region entries by a prefix over the lanes of entry maps: lane k's map sends an entry
    // offset d < 8 to the offset its chain enters region k+1 at (8: not below 8 there, or it
    // leaves otherwise). The chain is exact up to the first lane the maps lose it at; from there a
    // scalar walk follows it region by region.
    uint32_t e = __builtin_amdgcn_readfirstlane(entry);
    const uint32_t L0 = (e - W0) >> 7, d0 = e - W0 - (L0 << 7);
    uint32_t ent = SNAP_INVALID;
    if (d0 < 8) {
        uint32_t P = 0;
        #pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint32_t o = c[q] - SNAP_RB;
            P |= (o < 8u ? o : 8u) << (4 * q);
        }
        if (uint32_t(lane) < L0) P = 0x76543210u;   // identity
        #pragma unroll
        for (int h = 1; h < 64; h <<= 1) {
            uint32_t A = __shfl_up(P, h, 64);
            if (lane < h) A = 0x76543210u;
            uint32_t np = 0;
            #pragma unroll
            for (int q = 0; q < 8; q++) {
                const uint32_t a = (A >> (4 * q)) & 15u;
                np |= (a >= 8u ? 8u : (P >> (4u * a)) & 15u) << (4 * q);
            }
            P = np;
        }
        const uint32_t Pp = __shfl_up(P, 1, 64);
        const uint32_t off = uint32_t(lane) == L0 ? d0 : (uint32_t(lane) > L0 ? (Pp >> (4u * d0)) & 15u : 8u);
        const uint64_t lost = __ballot(uint32_t(lane) > L0 && off == 8u);
        const uint32_t j = lost ? uint32_t(__ffsll((unsigned long long)lost) - 1) : 64u;
        if (uint32_t(lane) >= L0 && uint32_t(lane) < j) ent = rs + off;
        e = __builtin_amdgcn_readlane(ent, int(j - 1));   // the last lane the maps resolved
    }
    uint64_t X;
    bool sat = false;
    for (;;) {   // uniform (scalar) walk
        const uint32_t k = (e - W0) >> 7, d = e - W0 - (k << 7);
        uint32_t x;
        if (d < 8) {
            uint32_t r[8];
            #pragma unroll
            for (int q = 0; q < 8; q++) r[q] = __builtin_amdgcn_readlane(c[q], int(k));
            x = r[0];
            #pragma unroll
            for (int q = 1; q < 8; q++) x = d == uint32_t(q) ? r[q] : x;
        } else {
            x = __builtin_amdgcn_readfirstlane(uint32_t(xs[d * 64 + k]));
        }
        ent = uint32_t(lane) == k ? e : ent;
        if (x == XS_SAT) { sat = true; X = 0; break; }
        const uint64_t ex = uint64_t(W0) + (k << 7) + x;
        if (ex >= n || ex >= uint64_t(W0) + SNAP_WIN) { X = ex; break; }
        e = uint32_t(ex);
    }
    PT(23);
    L.b0 = L.b1 = L.b2 = L.b3 = 0;
    L.out = 0;
    if (sat) {   // exact whole-wave parse on a linear stage
        __syncthreads();
        const uint32_t woff = snap_stage(reinterpret_cast<uint8_t*>(xs), in, n, W0, SNAP_WSTAGE, lane);
        reinterpret_cast<uint4*>(sbits)[lane] = make_uint4(0, 0, 0, 0);
        slo[lane] = 0;
        __syncthreads();
        uint32_t sum;
        const uint64_t wend = min(uint64_t(W0) + SNAP_WIN, n);
        const uint32_t Xs = seq_parse(reinterpret_cast<const uint8_t*>(xs), woff, W0, n, entry, wend, sbits, slo, sum);
        __syncthreads();
        const uint4 v = reinterpret_cast<const uint4*>(sbits)[lane];
        L.b0 = v.x; L.b1 = v.y; L.b2 = v.z; L.b3 = v.w;
        L.out = slo[lane];
        return Xs;
    }
    if (X > n) return SNAP_INVALID;
    // (4)
    if (ent != SNAP_INVALID) {
        const uint32_t re = uint32_t(min<uint64_t>(uint64_t(rs) + SNAP_RB, n));
        uint32_t p = ent;
        while (p < re) {
            const uint32_t o = p - rs;
            const uint32_t tag = (*reinterpret_cast<const uint32_t*>(mine + (o & ~3u)) >> (8u * (o & 3u))) & 0xffu;
            uint32_t tl = tag_tl(tag), ol = tag_ol(tag);
            if (tag_long(tag)) {   // < 2^15 past the region (the exits are not saturated)
                const SnapTok t = snap_tok(lds_read8(mine, o));
                tl = uint32_t(t.tl);
                ol = t.ol;
            }
            bit_set(L, o);
            const uint32_t s2 = L.out + ol;
            L.out = s2 < L.out ? 0xffffffffu : s2;
            p += tl;
        }
    }
    PT(24);
    return uint32_t(X);
#undef PT
}

__device__ __forceinline__ void store_window(uint32_t* tm, uint32_t* lo, const WinLane& L, int lane) {
    reinterpret_cast<uint4*>(tm)[lane] = make_uint4(L.b0, L.b1, L.b2, L.b3);
    lo[lane] = L.out;
}

__global__ __launch_bounds__(64) void k_snappy_index(const SnappyJob* __restrict__ jobs, const int2* __restrict__ wins,
                                                     SnapWin* __restrict__ win, SnapEnt* __restrict__ ent,
                                                     uint32_t* __restrict__ lane_out, int* __restrict__ fb) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[IDX_STAGE];
    __shared__ __attribute__((aligned(16))) uint32_t sbits[SNAP_WWORDS];
    __shared__ uint32_t slo[64];
    const int2 jw = wins[blockIdx.x];
    if (fb[jw.x] >= FB_INPLACE) return;   // one literal: in place, or copied by k_snappy_litcopy
    const SnappyJob job = jobs[jw.x];
    const int lane = threadIdx.x;
    const uint64_t n = job.src_len;
    const uint32_t W0 = uint32_t(jw.y) * SNAP_WIN;
    const uint32_t wi = job.win_base + uint32_t(jw.y);
    uint32_t* tm = job.tokmap + size_t(jw.y) * SNAP_WWORDS;
    uint32_t* lo = lane_out + size_t(wi) * 64;
    uint32_t entry = W0;
    WinLane L{};
    if (jw.y == 0) {
        uint64_t pos = 0, ulen = 0;
        if (!uvarint(job.src, n, pos, ulen) || ulen != job.dst_len) {   // the serial kernel reports it
            store_window(tm, lo, L, lane);
            if (lane == 0) { win[wi] = SnapWin{0, SNAP_INVALID, 0, WIN_BROKEN}; fb[jw.x] = FB_SERIAL; }
            return;
        }
        entry = uint32_t(pos);
    }
    if (entry >= n) {   // empty body
        store_window(tm, lo, L, lane);
        if (lane == 0) win[wi] = SnapWin{entry, entry, 0, 0};
        return;
    }
    const uint64_t wend = min(uint64_t(W0) + SNAP_WIN, n);
#ifdef PF_STAMPS
    unsigned long long it0 = __builtin_amdgcn_s_memtime();
    const unsigned long long itw = it0;
#endif
    const uint32_t woff = snap_stage(stage, job.src, n, W0, IDX_STAGE, lane);
    __syncthreads();
    uint32_t flags;
    uint32_t X = win_parse_spec(stage, woff, W0, n, entry, L, flags, sbits);
#ifdef PF_STAMPS
    // The phase times are kept in registers and added to the table at the wave's end, so that no phase holds
    // lane 0's atomics of the one before (3400 waves add to the same addresses). The spans are wave residency,
    // not work: DESIGN 4.37.
    unsigned long long st_spec, st_sum, st_store;
    { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_spec = t_ - it0; it0 = t_; }
#define IDX_FLUSH(t_end)                                                                               \
    do {                                                                                               \
        if (lane == 0) {                                                                               \
            CSTAMP(0, 1); CSTAMP(1, st_spec); CSTAMP(26, st_sum); CSTAMP(3, st_store);                 \
            CSTAMP(25, (t_end) - itw);                                                                 \
            if (noconv) CSTAMP(2, 1);                                                                  \
        }                                                                                              \
    } while (0)
#endif
    uint32_t sum;
    const bool noconv = flags & WIN_NOCONV;
    if (noconv) {   // chains that do not synchronise: exact whole-wave parse instead
        reinterpret_cast<uint4*>(sbits)[lane] = make_uint4(0, 0, 0, 0);
        slo[lane] = 0;
        __syncthreads();
        X = seq_parse(stage, woff, W0, n, entry, wend, sbits, slo, sum);
        flags = X == SNAP_INVALID ? WIN_BROKEN : 0u;
        __syncthreads();
        const uint4 v = reinterpret_cast<const uint4*>(sbits)[lane];
        L.b0 = v.x; L.b1 = v.y; L.b2 = v.z; L.b3 = v.w;
        L.out = slo[lane];
    } else {
        sum = wave_sum_sat(L.out);
    }
#ifdef PF_STAMPS   // (the wave sum apart from the stores)
    { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_sum = t_ - it0; }
#endif
    store_window(tm, lo, L, lane);
    if (lane == 0) win[wi] = SnapWin{entry, X, sum, flags};
#ifdef PF_STAMPS
    { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_store = t_ - it0; it0 = t_; }
#endif
    if (uint32_t(jw.y) + 1 >= job.n_win) {   // the page's last window: no successor
#ifdef PF_STAMPS
        IDX_FLUSH(it0);
#endif
        return;
    }
    // successor record: the answer for window w + 1's entry X, or none (window broken or parsed exactly, the
    // chain jumps over window w + 1 (WM_SKIP in the chain pass), or X lies past the staged extension)
    const uint32_t W1 = W0 + SNAP_WIN;
    const uint32_t wend1 = uint32_t(min(uint64_t(W1) + SNAP_WIN, n));
    X = __builtin_amdgcn_readfirstlane(X);
    SnapEnt R = mk_ent(0, ENT_SLOW, 0);
    uint32_t key = REC_NONE, steps = 0, need = 0;
    const bool asked = !noconv && !(flags & WIN_BROKEN) && X != SNAP_INVALID && X < wend1;
    if (asked && X - W1 < IDX_EXT) R = succ_walk(stage, woff - W0, X, W1, wend1, uint32_t(n), key, steps, need);
    if (lane == 0) *reinterpret_cast<uint4*>(ent + size_t(wi + 1) * 64) = make_uint4(R.pos, R.out, key, 0u);
#ifdef PF_STAMPS
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();
    IDX_FLUSH(t_);
#undef IDX_FLUSH
    if (lane == 0) {
        CSTAMP(9, t_ - it0);
        CSTAMP(4, steps);
        if (asked) CSTAMP(15, 1);
        if (asked && key == REC_NONE) CSTAMP(10, 1);
        if (key != REC_NONE && (R.pos >> 30) == ENT_SLOW) CSTAMP(5, 1);
        if (key != REC_NONE && (R.pos >> 30) == ENT_MERGE) {   // histogram of the bytes a resolved walk needed
            CSTAMP(6, need);
            uint32_t b = 0;
            while (b < 7 && need > (32u << b)) b++;
            CSTAMP(32 + b, 1);
        }
    }
#endif
}

// ======================================================================== chain pass

constexpr int FIX_MAXW = 1024;       // pages up to 8 MiB compressed (larger: serial fallback)

__device__ __forceinline__ bool tm_get(const uint32_t* tm, uint32_t i) { return (tm[i >> 5] >> (i & 31u)) & 1u; }

// An entry of window w that its record does not answer (deeper than IDX_EXT bytes, after a long
// literal; or not the predecessor's own exit): follow the chain from e in HBM until it meets the
// window's own chain (bitmap) or leaves the window. The window chain's output in [W0, m) is the
// lane-region counts before m's region plus the tokens of m's region below m.
__device__ SnapEnt deep_walk(const SnappyJob& job, uint32_t w, uint32_t e, uint64_t wend, const uint32_t* LOw) {
    const uint64_t n = job.src_len;
    const uint32_t W0 = w * SNAP_WIN;
    const uint32_t* tm = job.tokmap + size_t(w) * SNAP_WWORDS;
    uint64_t q = e;
    uint32_t acc = 0;
    int steps = 0;
    for (;;) {
        if (q >= wend) return mk_ent(uint32_t(q), ENT_NOMERGE, acc);
        if (tm_get(tm, uint32_t(q) - W0)) break;
        if (steps == DEEP_STEPS) return mk_ent(e, ENT_SLOW, 0);
        const SnapTok t = snap_tok(glb_read8(job.src, n, q));
        acc += t.ol;
        q += t.tl;
        steps++;
        if (q > n) return mk_ent(e, ENT_BAD, 0);
    }
    const uint32_t rel = uint32_t(q) - W0, rq = rel / SNAP_RB;
    uint32_t g = 0;
    for (uint32_t r = 0; r < rq; r++) g += LOw[r];
    for (uint32_t b = rq * SNAP_RB; b < rel; b += 32) {
        const uint32_t hi = rel - b >= 32 ? 0xffffffffu : ((1u << (rel - b)) - 1u);
        uint32_t mm = tm[b >> 5] & hi;
        while (mm) {
            const uint32_t i = b + uint32_t(__ffs(mm) - 1);
            mm &= mm - 1;
            g += snap_tok(glb_read8(job.src, n, W0 + i)).ol;
        }
    }
    return mk_ent(uint32_t(q), ENT_MERGE, acc - g);
}

// One wave per page, lanes over windows. Window 0's entry is exact (after the varint); window w's
// true entry is window w-1's true exit. Every window's exit as a function of its entry is known
// from the index pass for entries that merge with the window's own chain (exit = the window's own
// exit) or that leave it first (deep_walk); so all windows are evaluated at once from a
// guessed entry (the previous window's own exit, which the successor record answers) and
// re-evaluated where the previous exit changed, until the entries are consistent: the fixed point
// of e_w = exit_{w-1}(e_{w-1}) with e_1 exact is unique, so a consistent assignment is the true
// chain. Usually two rounds, each one record load per window. A window neither the record nor the
// walk resolves (entry not within IDX_STEPS / DEEP_STEPS tokens of the chain) stops the
// propagation; the first such window is parsed exactly by the whole wave
// once its entry is final, and the rounds continue behind it. The result replaces each window's
// SnapWin: {true entry, merge point / exit, true output bytes, WM_* mode}.
// LDS: the DP stage of the exact window parse (25 KiB) plus five per-window words sized by the host
// to the batch's largest page (dynamic LDS, cap windows; round 3 sized them for FIX_MAXW = 20 KiB).
// (r04: a whole-wave sequential exact parse instead of win_parse needs 9.5 KiB in all, but took the
// isolated chain launch 93 -> 433 us on SF1: dense windows are parsed exactly often.)
__global__ __launch_bounds__(64) void k_snappy_chain(const SnappyJob* __restrict__ jobs, SnapWin* __restrict__ win,
                                                     const SnapEnt* __restrict__ ent, uint32_t* __restrict__ lane_out,
                                                     int* __restrict__ fb, uint32_t cap) {
    __shared__ __attribute__((aligned(16))) uint8_t sp[SNAP_PSTAGE];
    __shared__ __attribute__((aligned(16))) uint16_t xs[SNAP_RB * 64];
    __shared__ __attribute__((aligned(16))) uint32_t sbits[SNAP_WWORDS];
    __shared__ uint32_t slo[64];
    extern __shared__ uint32_t dyn_chain[];
    uint32_t* const s_e = dyn_chain;              // current entry of window w
    uint32_t* const s_x = dyn_chain + cap;        // exit given that entry (unresolved: the window's own exit)
    uint32_t* const s_pos = dyn_chain + 2 * cap;  // merge point / exit (SnapWin.exit)
    uint32_t* const s_out = dyn_chain + 3 * cap;  // true output bytes
    uint32_t* const s_mode = dyn_chain + 4 * cap; // 0 entry changed, 1 unresolved, else WM_* (WM_DONE: final)
    const int j = blockIdx.x;
    const int lane = threadIdx.x;
    const SnappyJob job = jobs[j];
    if (fb[j] >= FB_SERIAL) return;
    const uint32_t nw = job.n_win;
    const uint64_t n = job.src_len;
    SnapWin* Wn = win + job.win_base;
    const SnapEnt* E = ent + size_t(job.win_base) * 64;
    uint32_t* LO = lane_out + size_t(job.win_base) * 64;
    if (nw > cap || nw > uint32_t(FIX_MAXW) || (Wn[0].flags & WIN_BROKEN)) {
        if (lane == 0) fb[j] = FB_SERIAL;
        return;
    }
    const SnapWin w0 = Wn[0];
    if (lane == 0) {
        Wn[0] = SnapWin{w0.entry, w0.exit, w0.out, WM_KEEP};
        s_x[0] = w0.exit;
        s_mode[0] = WM_KEEP;
    }
    for (uint32_t w = 1 + lane; w < nw; w += 64) {   // first guess: the previous window's own exit
        s_e[w] = w == 1 ? w0.exit : Wn[w - 1].exit;
        s_mode[w] = 0;
    }
    __syncthreads();
#ifdef PF_STAMPS
    const unsigned long long cstart = __builtin_amdgcn_s_memtime();
    if (lane == 0) { CSTAMP(17, 1); CSTAMP(18, nw); }
#endif
    bool bad = false;
    uint32_t base = 1;       // windows before base are final
    bool dirty_all = true;   // first round: evaluate every window
    while (base < nw) {
        // fixed-point rounds over [base, nw): re-evaluate windows whose entry changed (mode 0).
        // An unresolved window (mode 1) passes its own exit on as the guess for the next entry.
        for (;;) {
            for (uint32_t w = base + lane; w < nw; w += 64) {
                if (s_mode[w] == WM_DONE || (!dirty_all && s_mode[w] != 0)) continue;
                const uint32_t e = s_e[w];
                const uint32_t W0 = w * SNAP_WIN;
                const uint64_t wend = min(uint64_t(W0) + SNAP_WIN, n);
                uint32_t x, pos = 0, out = 0, mode;
                if (uint64_t(e) >= wend) {   // inside a literal that started earlier: no token here
                    x = e; pos = e; mode = WM_SKIP;
                } else {
                    const SnapWin sw = Wn[w];
                    SnapEnt T = mk_ent(e, ENT_SLOW, 0);
                    if (!(sw.flags & WIN_BROKEN)) {
#ifdef PF_STAMPS
                        const unsigned long long dt0 = __builtin_amdgcn_s_memtime();
#endif
                        // the record window w - 1 left, if it answers this entry; else a walk in HBM. A record
                        // that did not resolve its own entry stands for every entry: where the chains from W0 and
                        // from one entry stay apart that long, they do from the others (in SF1, 3984 of the 4032
                        // entries of such windows; round 6), and the walk would cost a third of the exact parse.
                        const uint4 rec = *reinterpret_cast<const uint4*>(E + size_t(w) * 64);
                        const bool hit = rec.z == e || (rec.z != REC_NONE && (rec.x >> 30) == ENT_SLOW);
                        T = hit ? SnapEnt{rec.x, rec.y} : deep_walk(job, w, e, wend, LO + size_t(w) * 64);
#ifdef PF_STAMPS
                        if (!hit) { CSTAMP(11, 1); CSTAMP(12, __builtin_amdgcn_s_memtime() - dt0); }
#endif
                    }
                    const uint32_t fl = T.pos >> 30, tp = T.pos & ENT_POS;
                    x = sw.exit; mode = 1u;
                    if (fl == ENT_MERGE) { pos = tp; out = sw.out + T.out; mode = WM_MERGE; }
                    else if (fl == ENT_NOMERGE) { x = tp; pos = tp; out = T.out; mode = WM_FULL; }
                }
                s_x[w] = x; s_pos[w] = pos; s_out[w] = out; s_mode[w] = mode;
            }
            dirty_all = false;
            if (lane == 0) CSTAMP(13, 1);
            __syncthreads();
            bool changed = false;
            for (uint32_t w = base + lane; w < nw; w += 64) {   // window base - 1 is final
                const uint32_t ne = s_x[w - 1];
                if (ne != s_e[w]) { s_e[w] = ne; s_mode[w] = 0; changed = true; }
            }
            __syncthreads();
            if (!__any(changed)) break;
        }
        // the first unresolved window: its entry is final now, parse it exactly
        uint32_t u = nw;
        for (uint32_t w = base + lane; w < nw; w += 64)
            if (s_mode[w] == 1u) { u = w; break; }
        #pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) u = min(u, uint32_t(__shfl_xor(u, dd, 64)));
        if (u >= nw) break;
#ifdef PF_STAMPS
        const unsigned long long xt0 = __builtin_amdgcn_s_memtime();
#endif
        const uint32_t e = s_e[u];
        const uint32_t W0 = u * SNAP_WIN;
        stage_pad(sp, job.src, n, W0, lane);
        __syncthreads();
        WinLane WL{};
        const uint32_t X = win_parse(job.src, n, W0, e, sp, xs, sbits, slo, WL);
        if (X == SNAP_INVALID) { bad = true; break; }
        const uint32_t sum = wave_sum_sat(WL.out);
        store_window(job.tokmap + size_t(u) * SNAP_WWORDS, LO + size_t(u) * 64, WL, lane);
        __syncthreads();
        if (lane == 0) {
            s_x[u] = X; s_pos[u] = X; s_out[u] = sum; s_mode[u] = WM_DONE;
        }
        __syncthreads();
        base = u + 1;
#ifdef PF_STAMPS
        if (lane == 0) { CSTAMP(14, 1); CSTAMP(16, __builtin_amdgcn_s_memtime() - xt0); }
#endif
    }
    if (!bad) {
        bad = uint64_t(s_x[nw - 1]) != n;
        for (uint32_t w = 1 + lane; w < nw && !bad; w += 64) Wn[w] = SnapWin{s_e[w], s_pos[w], s_out[w], s_mode[w]};
    }
    if (bad && lane == 0) fb[j] = FB_SERIAL;
#ifdef PF_STAMPS
    if (lane == 0) { const unsigned long long dt_ = __builtin_amdgcn_s_memtime() - cstart; CSTAMP(19, dt_); atomicMax(&pf_cstamps[20], dt_); }
#endif
}

// One wave per window: make the bitmap and lane output counts of windows whose true entry is not
// their own chain's start exact — tokens in [W0, merge point) for WM_MERGE, the whole window for
// WM_FULL — by parsing from the true entry on the staged window; clear the bitmap of windows the
// chain jumps over (WM_SKIP).
__device__ void repair_window(const SnappyJob* __restrict__ jobs, const int2 jw, const SnapWin* __restrict__ win,
                              uint32_t* __restrict__ lane_out, int* __restrict__ fb, uint8_t* stage, uint32_t* sbits,
                              uint32_t* slo) {
    const SnappyJob job = jobs[jw.x];
    const int lane = threadIdx.x;
    if (fb[jw.x] >= FB_SERIAL) return;
    const uint32_t w = uint32_t(jw.y);
    const SnapWin sw = win[job.win_base + w];
    const uint32_t W0 = w * SNAP_WIN;
    if (sw.flags == WM_SKIP) {   // inside a literal: no token starts here (the index pass's guesses are cleared,
                                 // so the bitmap is exact over the whole stream)
        reinterpret_cast<uint4*>(job.tokmap + size_t(w) * SNAP_WWORDS)[lane] = make_uint4(0, 0, 0, 0);
        return;
    }
    if (!((sw.flags == WM_MERGE && sw.entry != W0) || sw.flags == WM_FULL)) return;
    const uint64_t n = job.src_len;
    const uint64_t wend = min(uint64_t(W0) + SNAP_WIN, n);
    const uint64_t stop = sw.flags == WM_FULL ? wend : uint64_t(sw.exit);
    // WM_MERGE reads the window only up to its merge point's lane region (+ a token's bytes and the
    // parse's 64-position lookahead): usually the first 256 bytes, not the whole 8 KiB (round 5)
    const uint32_t need = sw.flags == WM_FULL ? SNAP_WSTAGE
                                              : min(SNAP_WSTAGE, ((sw.exit - W0) / SNAP_RB + 1) * SNAP_RB + 128u);
    const uint32_t woff = snap_stage(stage, job.src, n, W0, need, lane);
    reinterpret_cast<uint4*>(sbits)[lane] = make_uint4(0, 0, 0, 0);
    slo[lane] = 0;
    __syncthreads();
    uint32_t sum;
    const uint32_t X = seq_parse(stage, woff, W0, n, sw.entry, stop, sbits, slo, sum);
    __syncthreads();
    uint32_t* tm = job.tokmap + size_t(w) * SNAP_WWORDS;
    uint32_t* lo = lane_out + size_t(job.win_base + w) * 64;
    if (sw.flags == WM_FULL) {
        if (X == SNAP_INVALID || uint64_t(X) < wend) { if (lane == 0) atomicMax(&fb[jw.x], FB_SERIAL); return; }
        reinterpret_cast<uint4*>(tm)[lane] = reinterpret_cast<const uint4*>(sbits)[lane];
        lo[lane] = slo[lane];
        return;
    }
    if (X != sw.exit) { if (lane == 0) atomicMax(&fb[jw.x], FB_SERIAL); return; }
    // WM_MERGE: bits below the merge point m come from the parse, bits from m on stay
    const uint32_t rel = sw.exit - W0, rm = rel / SNAP_RB;
    if (uint32_t(lane) > rm) return;
    uint32_t nb[4];
    #pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t wi = uint32_t(lane) * 4 + k, b0 = wi * 32;
        const uint32_t low = b0 + 32 <= rel ? 0xffffffffu : (b0 >= rel ? 0u : (1u << (rel - b0)) - 1u);
        nb[k] = low == 0xffffffffu ? sbits[wi] : ((sbits[wi] & low) | (tm[wi] & ~low));
        tm[wi] = nb[k];
    }
    if (uint32_t(lane) < rm) { lo[lane] = slo[lane]; return; }
    // the merge point's region: parsed tokens below m plus the window's own tokens from m on
    uint32_t acc = slo[lane];
    #pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t b0 = (uint32_t(lane) * 4 + k) * 32;
        uint32_t mm = nb[k] & ~(b0 + 32 <= rel ? 0xffffffffu : (b0 >= rel ? 0u : (1u << (rel - b0)) - 1u));
        while (mm) {
            const uint32_t i = b0 + uint32_t(__ffs(mm) - 1);
            mm &= mm - 1;
            acc += snap_tok(lds_read8(stage, woff + i)).ol;
        }
    }
    lo[lane] = acc;
}

// Grid-stride over the windows (PF_REPAIR_GRID bounds the grid; by default one block per window):
// only windows the chain pass could not resolve (WM_MERGE / WM_FULL) and windows inside a literal
// (WM_SKIP: bitmap cleared) do work.
__global__ __launch_bounds__(64) void k_snappy_repair(const SnappyJob* __restrict__ jobs, const int2* __restrict__ wins,
                                                      int n_wins, const SnapWin* __restrict__ win,
                                                      uint32_t* __restrict__ lane_out, int* __restrict__ fb) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[SNAP_WSTAGE];
    __shared__ __attribute__((aligned(16))) uint32_t sbits[SNAP_WWORDS];
    __shared__ uint32_t slo[64];
    for (int b = blockIdx.x; b < n_wins; b += gridDim.x) {
        repair_window(jobs, wins[b], win, lane_out, fb, stage, sbits, slo);
        __syncthreads();
    }
}

// One workgroup per page: wave 0 checks the output total (window prefix sums into LDS); then each
// wave takes pieces in turn and finds the input position of the token that starts at the piece's
// 64 KiB output boundary with all of its loads issued together: the window's 64 lane-region output
// counts (one per lane; a ballot picks the region), then the region's 128 bytes (+ 8 for the last
// token's length bytes) and its 4 token-start bitmap words, then one token per lane position and a
// wave scan of their output lengths. (Round 3 walked the region counts and the tokens one dependent
// load at a time per piece: ~50 us per launch.)
constexpr int SP_NT = 256;
__global__ __launch_bounds__(SP_NT) void k_snappy_splits(const SnappyJob* __restrict__ jobs, const SnapWin* __restrict__ win,
                                                         const uint32_t* __restrict__ lane_out, uint32_t* __restrict__ splits,
                                                         int* __restrict__ fb) {
    __shared__ uint32_t s_pre[FIX_MAXW + 1];
    __shared__ __attribute__((aligned(16))) uint8_t s_reg[SP_NT / 64][SNAP_RB + 16];
    __shared__ uint32_t s_tm[SP_NT / 64][4];
    __shared__ int s_ok;
    const int j = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const SnappyJob job = jobs[j];
    if (fb[j] >= FB_SERIAL) return;   // (block-uniform)
    const uint32_t nw = job.n_win;
    const uint64_t n = job.src_len;
    const SnapWin* Wn = win + job.win_base;
    const uint32_t* LO = lane_out + size_t(job.win_base) * 64;
    if (wv == 0) {
        uint32_t run = 0;
        bool ovf = false;
        for (uint32_t w0i = 0; w0i < nw; w0i += 64) {
            const uint32_t w = w0i + lane;
            const uint32_t o = w < nw ? Wn[w].out : 0u;
            uint64_t x = o;
            #pragma unroll
            for (int dd = 1; dd < 64; dd <<= 1) {
                const uint64_t y = __shfl_up(x, dd, 64);
                if (lane >= dd) x += y;
            }
            if (w < nw) s_pre[w] = uint32_t(run + x - o);
            const uint64_t t = uint64_t(run) + __shfl(x, 63, 64);
            ovf |= t > 0xffffffffull;
            run = uint32_t(t);
        }
        const bool ok = !ovf && run == job.dst_len;
        if (lane == 0) { s_ok = ok; if (!ok) fb[j] = FB_SERIAL; }
    }
    __syncthreads();
    if (!s_ok) return;
    uint32_t* sp = splits + job.split_base;
    uint8_t* R = s_reg[wv];
    const PF_GLOBAL uint8_t* src = gptr(job.src);
    for (uint32_t k = 1 + uint32_t(wv); k < job.n_pieces; k += SP_NT / 64) {
        const uint32_t B = k * SNAP_BLOCK;
        uint32_t a = 0, b = nw;   // last window with s_pre <= B
        while (b - a > 1) {
            const uint32_t m = (a + b) / 2;
            if (s_pre[m] <= B) a = m; else b = m;
        }
        const uint32_t w = a;
        // the lane region holding output byte B: the first of regions 0..62 whose end passes B (else 63)
        const uint32_t v = LO[size_t(w) * 64 + lane];
        uint64_t x = v;
        #pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {
            const uint64_t y = __shfl_up(x, dd, 64);
            if (lane >= dd) x += y;
        }
        const uint64_t base = s_pre[w];
        const uint64_t past = __ballot(lane < 63 && uint64_t(B) < base + x);
        const int l = past ? __ffsll((unsigned long long)past) - 1 : 63;
        const uint64_t cum0 = base + __shfl(x - v, l, 64);   // output before region l
        // the region's bytes (zero past the stream) and its token-start bitmap
        const uint32_t rs = w * SNAP_WIN + uint32_t(l) * SNAP_RB;
        const uint64_t q0 = uint64_t(rs) + uint32_t(lane), q1 = q0 + 64, q2 = q0 + 128;
        const uint8_t c0 = q0 < n ? src[q0] : uint8_t(0), c1 = q1 < n ? src[q1] : uint8_t(0);
        const uint8_t c2 = (lane < 16 && q2 < n) ? src[q2] : uint8_t(0);
        const uint32_t tw = lane < 4 ? job.tokmap[size_t(w) * SNAP_WWORDS + uint32_t(l) * 4 + uint32_t(lane)] : 0u;
        R[lane] = c0; R[64 + lane] = c1;
        if (lane < 16) R[128 + lane] = c2;
        if (lane < 4) s_tm[wv][lane] = tw;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // one position per lane and half: output length of the token starting there (0: none)
        uint32_t ol[2];
        bool st[2];
        for (int h = 0; h < 2; h++) {
            const uint32_t i = uint32_t(h) * 64 + uint32_t(lane);
            st[h] = (s_tm[wv][i >> 5] >> (i & 31)) & 1u;
            uint64_t t8 = 0;
            #pragma unroll
            for (int u = 0; u < 8; u++) t8 |= uint64_t(R[i + u]) << (8 * u);
            ol[h] = st[h] ? snap_tok(t8).ol : 0u;
        }
        // the first token whose preceding output reaches B: found when it equals B
        uint32_t found = SNAP_INVALID;
        uint64_t cum = cum0;
        for (int h = 0; h < 2; h++) {
            uint64_t y = ol[h];
            #pragma unroll
            for (int dd = 1; dd < 64; dd <<= 1) {
                const uint64_t z = __shfl_up(y, dd, 64);
                if (lane >= dd) y += z;
            }
            const uint64_t before = cum + y - ol[h];
            const uint64_t hit = __ballot(st[h] && before >= uint64_t(B));
            if (hit) {
                const int f = __ffsll((unsigned long long)hit) - 1;
                if (__shfl(before, f, 64) == uint64_t(B)) found = rs + uint32_t(h) * 64 + uint32_t(f);
                break;
            }
            cum += __shfl(y, 63, 64);
        }
        if (lane == 0) sp[k] = found;
        __builtin_amdgcn_wave_barrier();   // (the region buffer is rewritten by the next piece)
    }
}

// Parse stage (token-start bitmaps, chain, 64 KiB split points). The execute stage is launch_snappy_exec
// (pf_snappy_exec.hip): separate launchers, so the runtime can time the stages apart.
void launch_snappy_parse(const SnappyJob* d_jobs, int n_jobs, const int2* d_wins, int n_wins, SnapWin* d_win,
                         SnapEnt* d_ent, uint32_t* d_lane_out, uint32_t* d_splits, int* d_fb, int max_nwin, hipStream_t s) {
    if (n_jobs <= 0) return;
    hipLaunchKernelGGL(k_snappy_index, dim3(n_wins), dim3(64), 0, s, d_jobs, d_wins, d_win, d_ent, d_lane_out, d_fb);
    // per-window tables of the largest page (multiple of 16 windows; pages above FIX_MAXW go serial)
    const uint32_t cap = uint32_t(std::min(FIX_MAXW, (std::max(max_nwin, 1) + 15) & ~15));
    hipLaunchKernelGGL(k_snappy_chain, dim3(n_jobs), dim3(64), 5 * 4 * cap, s, d_jobs, d_win, (const SnapEnt*)d_ent,
                       d_lane_out, d_fb, cap);
#ifndef PF_REPAIR_GRID   // (1024: SF1 3.30 ms mean of 6 interleaved runs; 4096: 3.28; one per window: 3.26 of 3)
#define PF_REPAIR_GRID (1 << 24)
#endif
    hipLaunchKernelGGL(k_snappy_repair, dim3(std::min(n_wins, PF_REPAIR_GRID)), dim3(64), 0, s, d_jobs, d_wins, n_wins,
                       (const SnapWin*)d_win, d_lane_out, d_fb);
    hipLaunchKernelGGL(k_snappy_splits, dim3(n_jobs), dim3(SP_NT), 0, s, d_jobs, (const SnapWin*)d_win,
                       (const uint32_t*)d_lane_out, d_splits, d_fb);
}

}  // namespace pf
