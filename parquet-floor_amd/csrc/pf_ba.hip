// pf_ba.hip — the PLAIN BYTE_ARRAY length walk on gfx950.
//
// Replaces the serial <4-byte LE length><bytes> chain parquet-mr 1.12.2 reads value by value in
// BinaryPlainValuesReader.readBytes (data pages) and PlainValuesDictionary.PlainBinaryDictionary
// (dictionary pages): one BaJob (pf_internal.h) per stream, guessed tile-parallel and verified, so
// that the positions and lengths are always the ones the serial walk would give.
//
// Kernels (256 threads; a grid of (job, BA_TILE-byte tile) pairs unless noted):
//   k_ba_tile     short values: candidates, both link levels, count and chain check in one pass
//   k_ba_cand, k_ba_link (x2), k_ba_count, k_ba_verify   the same steps as separate kernels
//   k_ba_scan     per job: exclusive scan of the tile counts; the total must be the value count
//   k_ba_emit     value k's chars start (and length) by rank
//   k_ba_fallback grid-stride over the jobs: a rejected job is re-linked over its whole bitmap
//                 (ba_relink_wg) or walked by one workgroup (binary_walk_wg, which ends in the
//                 exact one-lane plain_binary_walk)
#include <hip/hip_runtime.h>

#include "pf_launch.h"
#include "pf_pages.h"

namespace pf {

// ---- PLAIN BYTE_ARRAY walk (one lane; v1) --------------------------------------------------
// BinaryPlainValuesReader: <4-byte LE length><bytes> repeated. Writes the chars start of
// value k into pos[k]; returns total chars or -1 on overrun.
__device__ inline int64_t plain_binary_walk(const uint8_t* p, uint64_t n, int64_t count, uint32_t* pos, uint32_t* len) {
    uint64_t i = 0;
    int64_t total = 0;
    for (int64_t k = 0; k < count; k++) {
        if (i + 4 > n) return -1;
        uint32_t l = ld32le(p, i, n);
        i += 4;
        if (l > n - i) return -1;
        pos[k] = uint32_t(i);
        if (len) len[k] = l;
        i += l;
        total += l;
    }
    return total;
}

// ---- workgroup-parallel PLAIN BYTE_ARRAY walk --------------------------------------------------
// The <len><bytes> chain is serial, but a 4-byte little-endian length is "plausible" at position q
// only if q + 4 + len <= n, and a true prefix is followed by another plausible prefix (or by the
// stream end). Inside text (or most payloads) only the true prefixes pass both tests: the second
// one drops the candidates text produces just before each true prefix (the previous value's last
// byte + the low bytes of the next length). Every thread tests BW_BPT positions of a tile staged
// in LDS; the true chain is then the tile's entry plus the candidates that are another
// candidate's successor, and it must chain exactly (q_next == q + 4 + len) from the entry. Any
// mismatch — a false candidate that got linked, overflow, too few values — falls back to the exact
// serial walk, so the result is always the chain parquet-mr's BinaryPlainValuesReader reads.
constexpr int BW_BPT = 4;                           // positions per thread per tile (4: 5.5 KiB of LDS, so the
                                                    // normally idle k_ba_fallback launch does not wait for
                                                    // CUs with 21 KiB free while other streams run)
constexpr int BW_TILE = NT * BW_BPT;                // bytes per tile
constexpr int BW_LOOK = 64;                         // staged lookahead for successor tests
constexpr int BW_STAGE = BW_TILE + BW_LOOK + 16;    // + alignment shift
constexpr int BW_CAP = BW_TILE / 4;                 // candidates per tile (true prefixes are >= 4 bytes apart)

struct BinWalkLds {
    __attribute__((aligned(16))) uint8_t stage[BW_STAGE];
    uint32_t cand[BW_CAP];
    uint32_t next[BW_CAP];
    uint8_t linked[BW_CAP];    // candidate is another candidate's successor
    uint32_t acand[BW_CAP];    // accepted chain, in order
    uint32_t anext[BW_CAP];
    uint32_t scan[NT / 64];
    unsigned long long chars;
    uint32_t found, carry, bad;
};

// 4 bytes from LDS at byte offset a (a + 8 must be staged when a is not 4-aligned).
__device__ __forceinline__ uint32_t lds_read4(const uint8_t* s, uint32_t a) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(s + (a & ~3u));
    const uint32_t sh = 8u * (a & 3u);
    return sh ? (w[0] >> sh) | (w[1] << (32u - sh)) : w[0];
}

// Stage p[base - woff, base - woff + bytes) into LDS with 16-byte loads by the whole workgroup;
// 16-byte chunks wholly at or past n read as zero. Returns woff (base's 16-B misalignment).
__device__ __forceinline__ uint32_t wg_stage(uint8_t* stage, const uint8_t* p, uint64_t n, uint64_t base,
                                             uint32_t bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p + base);
    const uint32_t woff = uint32_t(a & 15u);
    const uint4* src = reinterpret_cast<const uint4*>(a - woff);
    const int64_t first = int64_t(base) - int64_t(woff);
    for (uint32_t c = threadIdx.x; c < bytes / 16; c += blockDim.x) {
        const int64_t q = first + int64_t(c) * 16;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (q < int64_t(n)) v = src[c];
        reinterpret_cast<uint4*>(stage)[c] = v;
    }
    return woff;
}

// The walk over candidates inside a tile: the true chain is the tile's entry E plus every
// candidate that is the successor of another candidate (a true value's successor is the next true
// value; a false candidate's successor is a random far position, so false candidates are almost
// never linked). The accepted list must still chain exactly from E and leave the tile; a false
// candidate that does get linked breaks that check and the page takes the serial walk.
constexpr int BW_CPT = BW_CAP / NT;                 // candidates owned by a thread (contiguous)

__device__ inline int64_t binary_walk_wg(const uint8_t* p, uint64_t n, int64_t count, uint32_t* pos, uint32_t* len,
                                         BinWalkLds& W) {
    const int tid = threadIdx.x;
    if (tid == 0) { W.found = 0; W.carry = 0; W.bad = 0; W.chars = 0; }
    __syncthreads();
    if (count == 0) return 0;
    if (n > 0x7fffffffull) return -1;
    for (uint64_t t0 = 0; t0 < n; t0 += BW_TILE) {
        if (W.found >= uint64_t(count) || W.bad) break;
        const uint32_t E = W.carry;                 // true chain position entering this tile
        const uint64_t tend = min(t0 + BW_TILE, n);
        if (E >= tend) continue;                    // one value spans the whole tile
        const uint32_t woff = wg_stage(W.stage, p, n, t0, BW_STAGE);
        for (uint32_t i = tid; i < BW_CAP / 4; i += NT) reinterpret_cast<uint32_t*>(W.linked)[i] = 0;
        __syncthreads();

        const uint64_t b0 = t0 + uint64_t(tid) * BW_BPT;
        uint32_t flags = 0, L[BW_BPT];
        #pragma unroll
        for (int i = 0; i < BW_BPT; i++) {
            const uint64_t q = b0 + i;
            L[i] = 0;
            if (q + 4 <= n && q >= E) {
                const uint32_t l = lds_read4(W.stage, woff + uint32_t(q - t0));
                if (uint64_t(l) <= n - q - 4) {
                    const uint64_t s = q + 4 + l;
                    bool ok = s == n;
                    if (!ok && s + 4 <= n) {
                        const uint32_t l2 = s + 8 <= t0 + BW_TILE + BW_LOOK ? lds_read4(W.stage, woff + uint32_t(s - t0))
                                                                              : ld32le(p, s, n);
                        ok = uint64_t(l2) <= n - s - 4;
                    }
                    if (ok) { flags |= 1u << i; L[i] = l; }
                }
            }
        }
        uint32_t tot;
        uint32_t idx = block_excl_scan<NT>(__popc(flags), W.scan, tot);

        if (tot > BW_CAP || tot == 0) { if (tid == 0) W.bad = 1; __syncthreads(); break; }
        #pragma unroll
        for (int i = 0; i < BW_BPT; i++) {
            if ((flags >> i) & 1u) {
                const uint32_t q = uint32_t(b0 + i);
                W.cand[idx] = q;
                W.next[idx] = q + 4 + L[i];
                idx++;
            }
        }
        __syncthreads();
        // link: mark every candidate that is another candidate's successor
        for (uint32_t i = tid; i < tot; i += NT) {
            const uint32_t s = W.next[i];
            if (s >= tend) continue;
            uint32_t lo = i + 1, hi = tot;   // successors lie at higher indices
            while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (W.cand[m] < s) lo = m + 1; else hi = m; }
            if (lo < tot && W.cand[lo] == s) W.linked[lo] = 1;
        }
        __syncthreads();

        // accepted = the entry + linked candidates, ranked in position order over contiguous ranges
        const uint32_t i0 = uint32_t(tid) * BW_CPT;
        uint32_t am = 0;
        #pragma unroll
        for (int k = 0; k < BW_CPT; k++) {
            const uint32_t i = i0 + k;
            am |= uint32_t(i < tot && (W.linked[i] || W.cand[i] == E)) << k;
        }
        uint32_t atot;
        uint32_t r = block_excl_scan<NT>(__popc(am), W.scan, atot);
        const uint32_t base = W.found;
        uint64_t my_chars = 0;
        #pragma unroll
        for (int k = 0; k < BW_CPT; k++) {
            if (!((am >> k) & 1u)) continue;
            const uint32_t q = W.cand[i0 + k], s = W.next[i0 + k];
            W.acand[r] = q;
            W.anext[r] = s;
            const uint64_t kk = uint64_t(base) + r;
            if (kk < uint64_t(count)) {
                pos[kk] = q + 4;
                if (len) len[kk] = s - q - 4;
                my_chars += s - q - 4;
            }
            r++;
        }
        __syncthreads();

        // the accepted list chains exactly from E and its last value leaves the tile
        int bad = 0;
        for (uint32_t a = tid; a < atot; a += NT) {
            if (uint64_t(base) + a >= uint64_t(count)) continue;
            bad |= W.acand[a] != (a == 0 ? E : W.anext[a - 1]);
        }
        if (tid == 0 && (atot == 0 || (W.anext[atot - 1] < tend && uint64_t(base) + atot < uint64_t(count)))) bad = 1;
        if (my_chars) atomicAdd(&W.chars, (unsigned long long)my_chars);
        bad = __syncthreads_or(bad);
        if (tid == 0) {
            if (bad) W.bad = 1;
            else W.carry = W.anext[atot - 1];
            W.found = base + atot;
        }
        __syncthreads();
    }
    __syncthreads();
    if (!W.bad && W.found >= uint64_t(count)) return int64_t(W.chars);
    // exact serial fallback (candidates the filters could not separate, or corrupt pages)
    __shared__ long long s_res;
    if (tid == 0) s_res = plain_binary_walk(p, n, count, pos, len);
    __syncthreads();
    return s_res;
}

// ---- tile-parallel PLAIN BYTE_ARRAY walk (k_ba_*) ----------------------------------------------
// BinaryPlainValuesReader reads <4-byte LE length><bytes> values one after another: a serial
// chain. Spread over the whole GPU instead of one workgroup per page:
//   k_ba_cand   every stream position q is a candidate if its length fits the stream, the
//               position after the value is the stream end or again a fitting length, and q + 1
//               is not plausible too (in text that pair is <char><len><0><0>: q is the char);
//   k_ba_link   (twice) link1 = successors of candidates, link2 = successors of link1 members
//               (position 0 is in both): a true value k >= 2 is in link2; a false candidate
//               needs two false predecessors lined up to get there;
//   k_ba_count / k_ba_scan  accepted = cand & link2, counted per tile, scanned per job; the total
//               must be the page's value count;
//   k_ba_emit   value k's chars start (and length) by rank;
//   k_ba_verify every accepted value's end must be the next accepted value's start, value 0 at 0;
//   k_ba_fallback  jobs that failed any check take the workgroup walk (binary_walk_wg, which ends
//               in the exact serial walk), so results never depend on the filters.
static_assert(BA_TILE == NT * 32, "8 KiB of stream per tile (pf_internal.h): one bitmap word per thread");
constexpr uint32_t BA_STAGE = BA_TILE + 32;    // + alignment shift and the lookahead of a length

__device__ __forceinline__ uint32_t ba_stage(uint8_t* stg, const uint8_t* p, uint64_t n, uint64_t base) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p + base);
    const uint32_t woff = uint32_t(a & 15u);
    const uint4* src = reinterpret_cast<const uint4*>(a - woff);
    const int64_t first = int64_t(base) - int64_t(woff);
    constexpr uint32_t NCH = BA_STAGE / 16, BU = (NCH + NT - 1) / NT;   // (all loads in flight, round 6)
    uint4 v[BU];
    #pragma unroll
    for (uint32_t u = 0; u < BU; u++) {
        const uint32_t c = threadIdx.x + NT * u;
        v[u] = make_uint4(0, 0, 0, 0);
        if (c < NCH && first + int64_t(c) * 16 < int64_t(n)) v[u] = src[c];
    }
    #pragma unroll
    for (uint32_t u = 0; u < BU; u++) {
        const uint32_t c = threadIdx.x + NT * u;
        if (c < NCH) reinterpret_cast<uint4*>(stg)[c] = v[u];
    }
    return woff;
}

__device__ __forceinline__ uint32_t lds_le32(const uint8_t* s, uint32_t a) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(s + (a & ~3u));
    const uint32_t sh = 8u * (a & 3u);
    return sh ? ((w[0] >> sh) | (w[1] << (32u - sh))) : w[0];
}

__global__ __launch_bounds__(NT) void k_ba_cand(BaJob* __restrict__ jobs, const int2* __restrict__ tiles) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[BA_STAGE];
    const int2 jt = tiles[blockIdx.x];
    const BaJob& J = jobs[jt.x];
    if (J.state != BA_OK) return;
    const uint32_t n = J.n;
    const uint32_t t0 = uint32_t(jt.y) * BA_TILE;
    if (t0 >= n) return;
    const uint8_t* p = J.p;
    const uint32_t woff = ba_stage(stg, p, n, t0);
    __syncthreads();
    const uint32_t wi = t0 / 32 + threadIdx.x;
    const uint32_t q0 = t0 + threadIdx.x * 32u;
    // lengths that fit the stream, for all 33 positions q0 .. q0 + 32 at once: the 36 bytes from q0
    // as 9 byte-aligned dwords, each position's little-endian length one v_alignbyte away (text
    // almost never passes: its "lengths" are 4 characters, far larger than the page)
    uint64_t fit = 0;
    {
        const uint32_t a = woff + threadIdx.x * 32u;
        const uint32_t* d = reinterpret_cast<const uint32_t*>(stg + (a & ~3u));
        const uint32_t s = a & 3u;
        uint32_t D[10], E[9];
        #pragma unroll
        for (int i = 0; i < 10; i++) D[i] = (a & ~3u) + 4u * i + 4u <= BA_STAGE ? d[i] : 0u;
        #pragma unroll
        for (int i = 0; i < 9; i++) E[i] = __builtin_amdgcn_alignbyte(D[i + 1], D[i], s);
        const int64_t room = int64_t(n) - int64_t(q0) - 4;   // a length at q0 + b fits if <= room - b
        #pragma unroll
        for (int b = 0; b <= 32; b++) {
            const uint32_t l = (b & 3) == 0 ? E[b >> 2] : __builtin_amdgcn_alignbyte(E[(b >> 2) + 1], E[b >> 2], b & 3);
            fit |= uint64_t(int64_t(l) <= room - b) << b;
        }
    }
    uint64_t m = 0;   // plausible positions: the length fits and the next value's length fits too
    for (uint64_t f = fit; f;) {
        const int b = __ffsll((unsigned long long)f) - 1;
        f &= f - 1;
        const uint32_t q = q0 + uint32_t(b);
        const uint32_t sv = q + 4 + lds_le32(stg, woff + (q - t0));
        bool ok = sv == n;
        if (!ok && uint64_t(sv) + 4 <= n) {
            const uint32_t ls = sv - t0 + 4 <= BA_TILE + 8 ? lds_le32(stg, woff + (sv - t0)) : ld32le(p, sv, n);
            ok = ls <= n - sv - 4;
        }
        m |= uint64_t(ok) << b;
    }
    // a plausible position followed by another is the byte before a true length prefix in text
    // (<char><len><0><0>): drop it (a true value that this drops fails the count check and takes
    // the exact fallback walk)
    J.cand[wi] = uint32_t(m & ~(m >> 1));
    J.link1[wi] = wi == 0 ? 1u : 0u;
    J.link2[wi] = wi == 0 ? 1u : 0u;
}

__global__ __launch_bounds__(NT) void k_ba_link(BaJob* __restrict__ jobs, const int2* __restrict__ tiles, int level) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[BA_STAGE];
    const int2 jt = tiles[blockIdx.x];
    const BaJob& J = jobs[jt.x];
    if (J.state != BA_OK) return;
    const uint32_t n = J.n;
    const uint32_t t0 = uint32_t(jt.y) * BA_TILE;
    if (t0 >= n) return;
    const uint32_t woff = ba_stage(stg, J.p, n, t0);
    __syncthreads();
    const uint32_t wi = t0 / 32 + threadIdx.x;
    const uint32_t* cand = J.cand;
    uint32_t* to = level == 1 ? J.link1 : J.link2;
    uint32_t m = cand[wi];
    if (level == 2) m &= J.link1[wi];
    while (m) {
        const uint32_t q = wi * 32u + uint32_t(__ffs(m) - 1);
        m &= m - 1;
        const uint32_t sv = q + 4 + lds_le32(stg, woff + (q - t0));
        if (sv < n && ((cand[sv >> 5] >> (sv & 31u)) & 1u)) atomicOr(&to[sv >> 5], 1u << (sv & 31u));
    }
}

// k_ba_cand + k_ba_link (both levels) + k_ba_count + k_ba_verify's chain check in one kernel per tile
// (round 4). The links of a position come from candidates at most BA_HALO bytes before it, so a tile
// computes candidates over [t0 - 2 BA_HALO, t1 + BA_HALO), first links over [t0 - BA_HALO, t1 +
// BA_HALO) and second links over [t0, t1 + BA_HALO) from one staged window (LDS bitmaps, no global
// atomics); positions both tiles see get the same bits. It writes the tile's accepted words and count,
// and checks the chain locally: every accepted value of the tile must end exactly at the next accepted
// position (and the job's first accepted position is 0); with the count check of k_ba_scan that is
// k_ba_verify's test. A value longer than BA_HALO - 4 bytes is not linked here: its page fails the count
// or the chain check (BA_RELINK) and k_ba_fallback re-links it over the whole job (ba_relink_wg, any
// value length) before it would take the exact walk, so the emitted positions are always the verified
// true chain.
constexpr int BA_HALO = 128;
constexpr uint32_t BA_XW = (2 * BA_HALO) / 32;                       // halo words before the tile
constexpr uint32_t BA_NW = BA_XW + BA_TILE / 32 + BA_HALO / 32;        // words of the window
constexpr uint32_t BA_FSTAGE = 3 * BA_HALO + BA_TILE + 48;           // staged bytes from t0 - 2 BA_HALO
__global__ __launch_bounds__(NT) void k_ba_tile(BaJob* __restrict__ jobs, const int2* __restrict__ tiles) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[BA_FSTAGE + 16];
    __shared__ uint32_t C[BA_NW], L1[BA_NW], L2[BA_NW];
    __shared__ uint32_t tmp[NT / 64];
    const int2 jt = tiles[blockIdx.x];
    BaJob& J = jobs[jt.x];
    // a job another tile already rejected (BA_RELINK) still needs this tile's candidate words:
    // ba_relink_wg re-links the job from the whole candidate bitmap
    const int32_t st0 = J.state;
    if (st0 == BA_SKIP || st0 == BA_FALLBACK) return;
    const uint32_t n = J.n;
    const uint32_t t0 = uint32_t(jt.y) * BA_TILE;
    if (t0 >= n) {
        if (threadIdx.x == 0) J.tile_cnt[jt.y] = 0;
        return;
    }
    const uint8_t* p = J.p;
    const int64_t sb = int64_t(t0) - 2 * BA_HALO;   // stream position of word 0 / stage byte woff
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(p) + uintptr_t(sb);
    const uint32_t woff = uint32_t(a0 & 15u);
    {   // 16-byte loads; chunks wholly before the stream start or at / past its end are zero (the chunk
        // holding byte 0 is read whole, as ba_stage does)
        const int64_t first = sb - int64_t(woff);
        const PF_GLOBAL u32x4* src = (const PF_GLOBAL u32x4*)(a0 - woff);
        constexpr uint32_t NCH = (BA_FSTAGE + 16) / 16, BU = (NCH + NT - 1) / NT;   // (all loads in flight, round 6)
        u32x4 v[BU];
        #pragma unroll
        for (uint32_t u = 0; u < BU; u++) {
            const uint32_t c = threadIdx.x + NT * u;
            const int64_t q = first + int64_t(c) * 16;
            v[u] = u32x4{0u, 0u, 0u, 0u};
            if (c < NCH && q + 16 > 0 && q < int64_t(n)) v[u] = src[c];
        }
        #pragma unroll
        for (uint32_t u = 0; u < BU; u++) {
            const uint32_t c = threadIdx.x + NT * u;
            if (c < NCH) reinterpret_cast<u32x4*>(stg)[c] = v[u];
        }
    }
    for (uint32_t i = threadIdx.x; i < BA_NW; i += NT) { C[i] = 0; L1[i] = 0; L2[i] = 0; }
    __syncthreads();
    auto len_at = [&](int64_t q) { return lds_le32(stg, woff + uint32_t(q - sb)); };   // q in the window
    // ---- candidates (k_ba_cand's rule)
    for (uint32_t w = threadIdx.x; w < BA_NW; w += NT) {
        const int64_t q0 = sb + int64_t(w) * 32;
        if (q0 + 32 <= 0 || q0 >= int64_t(n)) continue;
        const uint32_t a = woff + w * 32u;
        const uint32_t* d = reinterpret_cast<const uint32_t*>(stg + (a & ~3u));
        const uint32_t s = a & 3u;
        uint32_t D[10], E[9];
        #pragma unroll
        for (int i = 0; i < 10; i++) D[i] = d[i];
        #pragma unroll
        for (int i = 0; i < 9; i++) E[i] = __builtin_amdgcn_alignbyte(D[i + 1], D[i], s);
        const int64_t room = int64_t(n) - q0 - 4;
        uint64_t fit = 0;
        #pragma unroll
        for (int b = 0; b <= 32; b++) {
            const uint32_t l = (b & 3) == 0 ? E[b >> 2] : __builtin_amdgcn_alignbyte(E[(b >> 2) + 1], E[b >> 2], b & 3);
            fit |= uint64_t(int64_t(l) <= room - b && q0 + b >= 0) << b;
        }
        uint64_t m = 0;
        for (uint64_t f = fit; f;) {
            const int b = __ffsll((unsigned long long)f) - 1;
            f &= f - 1;
            const int64_t q = q0 + b;
            const uint32_t sv = uint32_t(q) + 4 + len_at(q);
            bool ok = sv == n;
            if (!ok && uint64_t(sv) + 4 <= n) {
                // a successor past the staged window is taken as plausible without reading it (round 5):
                // in text that is mostly the byte before a true length (<char><len><0><0> reads as a
                // length of a few thousand), which the adjacency rule below drops anyway, and the chain
                // and count checks decide the rest; the global read per value was k_ba_tile's 2.3x fetch
                const int64_t r = int64_t(sv) - sb;
                ok = r + 4 > int64_t(BA_FSTAGE) || lds_le32(stg, woff + uint32_t(r)) <= n - sv - 4;
            }
            m |= uint64_t(ok) << b;
        }
        C[w] = uint32_t(m & ~(m >> 1));
    }
    __syncthreads();
    const int64_t wend = sb + int64_t(BA_NW) * 32;   // end of the window
    // ---- first links: successors (within the halo) of candidates, over [t0 - BA_HALO, wend)
    for (uint32_t w = threadIdx.x; w < BA_NW; w += NT) {
        uint32_t mm = C[w];
        while (mm) {
            const uint32_t b = uint32_t(__ffs(mm) - 1);
            mm &= mm - 1;
            const int64_t q = sb + int64_t(w) * 32 + b;
            const int64_t sv = q + 4 + int64_t(len_at(q));
            if (sv - q <= BA_HALO && sv >= int64_t(t0) - BA_HALO && sv < wend && sv < int64_t(n)) {
                const uint32_t r = uint32_t(sv - sb);
                atomicOr(&L1[r >> 5], 1u << (r & 31u));
            }
        }
    }
    if (threadIdx.x == 0 && t0 == 0) atomicOr(&L1[BA_XW], 1u);   // position 0 starts the chain
    __syncthreads();
    // ---- second links: successors of candidates that are first links, over [t0, wend)
    for (uint32_t w = BA_XW / 2 + threadIdx.x; w < BA_NW; w += NT) {
        uint32_t mm = C[w] & L1[w];
        while (mm) {
            const uint32_t b = uint32_t(__ffs(mm) - 1);
            mm &= mm - 1;
            const int64_t q = sb + int64_t(w) * 32 + b;
            const int64_t sv = q + 4 + int64_t(len_at(q));
            if (sv - q <= BA_HALO && sv >= int64_t(t0) && sv < wend && sv < int64_t(n)) {
                const uint32_t r = uint32_t(sv - sb);
                atomicOr(&L2[r >> 5], 1u << (r & 31u));
            }
        }
    }
    if (threadIdx.x == 0 && t0 == 0) atomicOr(&L2[BA_XW], 1u);
    __syncthreads();
    // ---- accepted = candidates & second links: the tile's words, its count, the local chain check
    const uint32_t w = BA_XW + threadIdx.x;
    const uint32_t acc = C[w] & L2[w];
    const uint32_t wi = t0 / 32 + threadIdx.x;
    J.cand[wi] = C[w];
    J.link2[wi] = L2[w];
    bool bad = t0 == 0 && threadIdx.x == 0 && !(acc & 1u);   // the chain starts at position 0
    for (uint32_t mm = acc; mm && !bad;) {
        const uint32_t b = uint32_t(__ffs(mm) - 1);
        mm &= mm - 1;
        const int64_t q = sb + int64_t(w) * 32 + b;
        const int64_t sv = q + 4 + int64_t(len_at(q));
        // a value ending past the halo cannot be checked here (the exact walk takes the page)
        if (sv != int64_t(n) && sv - q > BA_HALO) { bad = true; break; }
        // the next accepted position after q must be sv: no accepted bit in (q, min(sv, wend)), bit sv set
        const int64_t stop = min(sv, wend);
        for (int64_t x = q + 1; x < stop;) {
            const uint32_t r = uint32_t(x - sb), ww = r >> 5;
            const uint32_t word = (C[ww] & L2[ww]) >> (r & 31u);
            const int64_t span = min(int64_t(32 - (r & 31u)), stop - x);
            if (word & (span >= 32 ? 0xffffffffu : ((1u << span) - 1u))) { bad = true; break; }
            x += span;
        }
        if (!bad && sv < wend && sv < int64_t(n)) {
            const uint32_t r = uint32_t(sv - sb);
            bad = !(((C[r >> 5] & L2[r >> 5]) >> (r & 31u)) & 1u);
        }
    }
    uint32_t tot;
    block_excl_scan<NT>(__popc(acc), tmp, tot);
    if (threadIdx.x == 0) J.tile_cnt[jt.y] = tot;
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicExch(&J.state, int32_t(BA_RELINK));
}

__global__ __launch_bounds__(NT) void k_ba_count(BaJob* __restrict__ jobs, const int2* __restrict__ tiles) {
    __shared__ uint32_t tmp[NT / 64];
    const int2 jt = tiles[blockIdx.x];
    const BaJob& J = jobs[jt.x];
    if (J.state != BA_OK) return;
    const uint32_t t0 = uint32_t(jt.y) * BA_TILE;
    if (t0 >= J.n) {
        if (threadIdx.x == 0) J.tile_cnt[jt.y] = 0;
        return;
    }
    const uint32_t wi = t0 / 32 + threadIdx.x;
    uint32_t tot;
    block_excl_scan<NT>(__popc(J.cand[wi] & J.link2[wi]), tmp, tot);
    if (threadIdx.x == 0) J.tile_cnt[jt.y] = tot;
}

__global__ __launch_bounds__(NT) void k_ba_scan(BaJob* __restrict__ jobs, int32_t fail_state) {
    __shared__ uint32_t tmp[NT / 64];
    BaJob& J = jobs[blockIdx.x];
    if (J.state != BA_OK) return;
    uint64_t run = 0;
    for (uint32_t b = 0; b < J.n_tiles; b += NT) {
        const uint32_t i = b + threadIdx.x;
        const uint32_t v = i < J.n_tiles ? J.tile_cnt[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan<NT>(v, tmp, tot);
        if (i < J.n_tiles) J.tile_cnt[i] = uint32_t(run) + ex;
        run += tot;
    }
    if (threadIdx.x == 0 && int64_t(run) != J.count) J.state = fail_state;   // (fused: BA_RELINK; round-3 kernels: BA_FALLBACK)
}

__global__ __launch_bounds__(NT) void k_ba_emit(BaJob* __restrict__ jobs, const int2* __restrict__ tiles) {
    __shared__ uint32_t tmp[NT / 64];
    const int2 jt = tiles[blockIdx.x];
    const BaJob& J = jobs[jt.x];
    if (J.state != BA_OK) return;
    const uint32_t n = J.n;
    const uint32_t t0 = uint32_t(jt.y) * BA_TILE;
    if (t0 >= n) return;
    const uint32_t wi = t0 / 32 + threadIdx.x;
    uint32_t m = J.cand[wi] & J.link2[wi];
    uint32_t tot;
    uint64_t k = uint64_t(J.tile_cnt[jt.y]) + block_excl_scan<NT>(__popc(m), tmp, tot);
    const uint64_t count = uint64_t(J.count);
    while (m) {
        const uint32_t q = wi * 32u + uint32_t(__ffs(m) - 1);
        m &= m - 1;
        if (k < count) {
            J.pos[k] = q + 4;
            if (J.len || k + 1 == count) {
                const uint32_t l = ld32le(J.p, q, n);
                if (J.len) J.len[k] = l;
                if (k + 1 == count && J.chars_out) *J.chars_out = int64_t(q) + 4 + int64_t(l) - 4 * int64_t(count);
            }
        }
        k++;
    }
}

__global__ __launch_bounds__(NT) void k_ba_verify(BaJob* __restrict__ jobs, const int2* __restrict__ tiles) {
    __shared__ uint32_t tmp[NT / 64];
    const int2 jt = tiles[blockIdx.x];
    BaJob& J = jobs[jt.x];
    if (J.state != BA_OK) return;
    const uint32_t n = J.n;
    const uint32_t t0 = uint32_t(jt.y) * BA_TILE;
    if (t0 >= n) return;
    const uint32_t wi = t0 / 32 + threadIdx.x;
    uint32_t m = J.cand[wi] & J.link2[wi];
    uint32_t tot;
    uint64_t k = uint64_t(J.tile_cnt[jt.y]) + block_excl_scan<NT>(__popc(m), tmp, tot);
    const uint64_t count = uint64_t(J.count);
    int bad = 0;
    while (m) {
        const uint32_t q = wi * 32u + uint32_t(__ffs(m) - 1);
        m &= m - 1;
        const uint32_t nq = q + 4 + ld32le(J.p, q, n);
        if (k == 0 && q != 0) bad = 1;
        if (k + 1 < count) bad |= J.pos[k + 1] != nq + 4;
        else if (k + 1 == count) { if (J.chars_out) *J.chars_out = int64_t(nq) - 4 * int64_t(count); }
        else bad = 1;
        k++;
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicExch(&J.state, int32_t(BA_FALLBACK));
}

// A job k_ba_tile rejected (BA_RELINK), in one workgroup: k_ba_link's rule over the job's whole
// candidate bitmap (k_ba_tile wrote it; successors at any distance, so values of any length), then
// k_ba_count / k_ba_scan / k_ba_emit / k_ba_verify's count, emit and chain check over the job's words
// in order. Returns -1 on every thread when the chain does not verify (the exact walk takes the job);
// otherwise the job's chars on the thread holding its last value and 0 on the others.
// Link words are read back with agent-scope loads (their bits were set by global atomics).
__device__ int64_t ba_relink_wg(BaJob& J, uint32_t* tmp) {
    const uint32_t n = J.n;
    const int64_t count = J.count;
    if (n == 0 || count <= 0) return -1;
    const uint32_t nw = (n + 31u) / 32u;
    const uint8_t* p = J.p;
    const uint32_t* cand = J.cand;
    uint32_t* l1 = J.link1;
    uint32_t* l2 = J.link2;
    auto ld = [](const uint32_t* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    for (uint32_t w = threadIdx.x; w < nw; w += NT) { l1[w] = w == 0 ? 1u : 0u; l2[w] = w == 0 ? 1u : 0u; }
    __syncthreads();
    for (int level = 1; level <= 2; level++) {   // link1: successors of candidates; link2: of link1 members
        uint32_t* to = level == 1 ? l1 : l2;
        for (uint32_t w = threadIdx.x; w < nw; w += NT) {
            uint32_t m = cand[w];
            if (level == 2) m &= ld(l1 + w);
            while (m) {
                const uint32_t q = w * 32u + uint32_t(__ffs(m) - 1);
                m &= m - 1;
                const uint64_t sv = uint64_t(q) + 4 + ld32le(p, q, n);
                if (sv < n && ((cand[sv >> 5] >> (sv & 31u)) & 1u)) atomicOr(&to[sv >> 5], 1u << (sv & 31u));
            }
        }
        __syncthreads();
    }
    // accepted = cand & link2: emit by rank, then check the chain (value k + 1 starts where k ends)
    int64_t run = 0;
    for (uint32_t b = 0; b < nw; b += NT) {
        const uint32_t w = b + threadIdx.x;
        uint32_t m = w < nw ? cand[w] & ld(l2 + w) : 0u;
        uint32_t tot;
        int64_t k = run + block_excl_scan<NT>(__popc(m), tmp, tot);
        while (m) {
            const uint32_t q = w * 32u + uint32_t(__ffs(m) - 1);
            m &= m - 1;
            if (k < count) {
                J.pos[k] = q + 4;
                if (J.len) J.len[k] = ld32le(p, q, n);
            }
            k++;
        }
        run += tot;
    }
    if (run != count) return -1;   // (uniform: every thread ran the same scans)
    __syncthreads();
    int bad = 0;
    int64_t chars = 0;
    run = 0;
    for (uint32_t b = 0; b < nw; b += NT) {
        const uint32_t w = b + threadIdx.x;
        uint32_t m = w < nw ? cand[w] & ld(l2 + w) : 0u;
        uint32_t tot;
        int64_t k = run + block_excl_scan<NT>(__popc(m), tmp, tot);
        while (m) {
            const uint32_t q = w * 32u + uint32_t(__ffs(m) - 1);
            m &= m - 1;
            const uint64_t nq = uint64_t(q) + 4 + ld32le(p, q, n);
            if (k == 0 && q != 0) bad = 1;
            if (k + 1 < count) bad |= ld(J.pos + k + 1) != nq + 4;
            else chars = int64_t(nq) - 4 * count;   // (k + 1 == count: run == count)
            k++;
        }
        run += tot;
    }
    if (__syncthreads_or(bad)) return -1;
    return chars;   // (the thread that holds the last value; 0 on the others)
}

// Grid-stride over the jobs with a small grid: nearly every walk was accepted by the checks above,
// and a block per job (21 KB of LDS each) would wait for CUs held by other streams' kernels.
#ifdef PF_DIAG   // diagnostics build: jobs k_ba_fallback re-linked / walked exactly (tests)
__device__ unsigned long long pf_ba_counts[2];
extern "C" int pf_debug_ba_counts(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pf_ba_counts), sizeof(unsigned long long) * 2) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pf_ba_counts), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#define BA_COUNT(i) (threadIdx.x == 0 ? (void)atomicAdd(&pf_ba_counts[i], 1ull) : (void)0)
#else
#define BA_COUNT(i) ((void)0)
#endif
__global__ __launch_bounds__(NT) void k_ba_fallback(BaJob* __restrict__ jobs, int n_jobs, DevChunkResult* res) {
    __shared__ BinWalkLds W;
    __shared__ long long s_chars;
    for (int j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        BaJob& J = jobs[j];
        if (J.state == BA_RELINK) {
            if (threadIdx.x == 0) s_chars = 0;
            __syncthreads();
            const int64_t c = ba_relink_wg(J, W.scan);   // (c < 0 on every thread or on none)
            if (c > 0) atomicAdd(reinterpret_cast<unsigned long long*>(&s_chars), (unsigned long long)c);
            __syncthreads();
            if (c >= 0) {
                if (threadIdx.x == 0 && J.chars_out) *J.chars_out = s_chars;
                BA_COUNT(0);
                __syncthreads();
                continue;
            }
        } else if (J.state != BA_FALLBACK) {
            continue;
        }
        const int64_t t = binary_walk_wg(J.p, J.n, J.count, J.pos, J.len, W);
        BA_COUNT(1);
        if (threadIdx.x == 0) {
            if (t < 0) set_status(res, J.chunk, ST_CORRUPT, J.page);
            else if (J.chars_out) *J.chars_out = t;
        }
        __syncthreads();
    }
}


// ---- launcher ----------------------------------------------------------------------------------
// PLAIN BYTE_ARRAY walks of jobs [0, n_jobs) over tiles [0, n_tiles).
void launch_ba(BaJob* d_jobs, int n_jobs, const int2* d_tiles, int n_tiles, DevChunkResult* d_res, hipStream_t st,
               bool short_values) {
    if (n_jobs <= 0 || n_tiles <= 0) return;
    // candidates, both link levels, the count and the chain check in one kernel (k_ba_tile) for batches
    // of short values (short_values; the diagnostics option ba_fused=0 clears it); otherwise the round-3 kernels
    const bool fused = short_values;
    if (!fused) {
        hipLaunchKernelGGL(k_ba_cand, dim3(n_tiles), dim3(NT), 0, st, d_jobs, d_tiles);
        hipLaunchKernelGGL(k_ba_link, dim3(n_tiles), dim3(NT), 0, st, d_jobs, d_tiles, 1);
        hipLaunchKernelGGL(k_ba_link, dim3(n_tiles), dim3(NT), 0, st, d_jobs, d_tiles, 2);
        hipLaunchKernelGGL(k_ba_count, dim3(n_tiles), dim3(NT), 0, st, d_jobs, d_tiles);
    } else {
        hipLaunchKernelGGL(k_ba_tile, dim3(n_tiles), dim3(NT), 0, st, d_jobs, d_tiles);
    }
    hipLaunchKernelGGL(k_ba_scan, dim3(n_jobs), dim3(NT), 0, st, d_jobs, fused ? int32_t(BA_RELINK) : int32_t(BA_FALLBACK));
    hipLaunchKernelGGL(k_ba_emit, dim3(n_tiles), dim3(NT), 0, st, d_jobs, d_tiles);
    if (!fused) hipLaunchKernelGGL(k_ba_verify, dim3(n_tiles), dim3(NT), 0, st, d_jobs, d_tiles);
    hipLaunchKernelGGL(k_ba_fallback, dim3(std::min(n_jobs, 64)), dim3(NT), 0, st, d_jobs, n_jobs, d_res);
}

}  // namespace pf
