// pf_fix_ids.h — the dictionary ids of 8 consecutive values from a page's id run table and one contiguous load of the
// id stream, one text for the kernel (k_flat_fixed's eight-a-thread body, pf_flat.hip) and for the host check
// (tests/native/pf_fix_ids_check.cpp), shared like pf_dstr_ids.h.
//
// A bit-packed run holds groups of eight ids in `bw` contiguous bytes, so a group of 8 consecutive values that lies
// in one run is one run lookup and at most 8 * bw bits from one bit position: for bw <= 16 they lie in five aligned
// 32-bit words at most (17 bytes from any byte, up to 3 bytes of alignment before them). The three steps are
// separate so that the kernel can issue the loads of all its groups before it waits for any of them:
//   fix_locate   the group's run: not fast | one value for all (RLE run, width 0) | the place of its first
//                word and the bit its first id starts at. A group whose words do not all lie inside the id section is
//                not fast, so no byte outside the section is ever read
//   fix_load     the words that hold the group's bits
//   fix_unpack   the eight ids, every shift a constant of the width's template instance
// fix_ids8 is the three in a row. A group that is not fast is the caller's to decode entry by entry.
#pragma once
#include <stdint.h>

#include "pf_internal.h"

namespace pf {

constexpr int FIX_BW_MAX = 16;   // widest id of the fast path
constexpr int FIX_NDW = 5;       // most words of a group

enum : uint32_t { FIX_SLOW = 0, FIX_CONST = 1, FIX_PACKED = 2 };
struct FixGrp {
    uint32_t kind;   // FIX_*
    uint32_t val;    // FIX_CONST: the id of every value of the group; FIX_PACKED: the bit of the first word its first id starts at
    uint32_t off4;   // FIX_PACKED: the group's first word, in bytes from the frame's start (a multiple of 4)
};

// The rows of k_runs' table as they lie in memory (row i = {first value | packed << 31, RLE value or bit offset}; a run
// ends where the next one starts, the last one at `cov`). This is the host check's view of a table, and the kernel's
// when it is built to look runs up in global memory (PF_FIX8_GLOBAL); by default the kernel reads the same rows through
// its LDS copy of them (FixRowsLds, pf_flat.hip), so fix_locate, fix_load and fix_unpack are the shared text.
struct FixRowsRt {
    const uint32_t* rt;
    uint32_t nr, cov;
    PF_HD uint32_t first(uint32_t i) const { return rt[2 * i] & 0x7fffffffu; }
    PF_HD uint32_t end(uint32_t i) const { return i + 1 < nr ? (rt[2 * i + 2] & 0x7fffffffu) : cov; }
    PF_HD uint32_t packed(uint32_t i) const { return rt[2 * i] >> 31; }
    PF_HD uint32_t data(uint32_t i) const { return rt[2 * i + 1]; }
};

// Words a group of width bw is loaded as: 8 * bw bits from bit 0..7 of a byte that is 0..3 bytes into the first word.
PF_HD inline int fix_ndw(int bw) { return bw > 0 ? (8 * bw + 62) / 32 : 0; }

// Values [e0, e0 + n), n <= 8, of a page whose `nr` runs are R's rows (sorted by first value, row 0 starts at 0). The
// id section is ids_n bytes that start `mis` (0..3) bytes into a frame of aligned 32-bit words: the frame starts at the
// 4-byte boundary at or before the section. Fast: all n in one run, and that run RLE (or of width 0: no stream bit is
// read), or n == 8, bw <= FIX_BW_MAX and every word of the load inside the section. The first and the last packed
// group of a page are therefore not fast when the section does not start or end on a word's boundary.
template <class Rows>
PF_HD inline FixGrp fix_locate(const Rows& R, uint32_t nr, uint32_t e0, uint32_t n, int bw, uint32_t mis, uint64_t ids_n) {
    FixGrp g{FIX_SLOW, 0u, 0u};
    if (nr == 0 || n == 0 || n > 8) return g;
    uint32_t lo = 0, hi = nr;
    while (hi - lo > 1) {
        const uint32_t m = (lo + hi) >> 1;
        if (R.first(m) <= e0) lo = m; else hi = m;
    }
    const uint32_t first = R.first(lo);
    if (e0 < first || e0 + n > R.end(lo)) return g;
    if (!R.packed(lo) || bw == 0) {
        g.kind = FIX_CONST;
        g.val = R.packed(lo) ? 0u : R.data(lo);
    } else if (n == 8 && bw <= FIX_BW_MAX) {
        const uint64_t bit = uint64_t(R.data(lo)) + uint64_t(e0 - first) * uint64_t(bw);
        const uint64_t o = (bit >> 3) + mis;   // the first id's byte in the frame
        const uint64_t o4 = o & ~3ull;
        if (o4 >= mis && o4 + 4u * uint64_t(fix_ndw(bw)) <= uint64_t(mis) + ids_n) {
            g.kind = FIX_PACKED;
            g.val = uint32_t(o & 3u) * 8u + uint32_t(bit & 7u);
            g.off4 = uint32_t(o4);
        }
    }
    return g;
}

// q[0 .. fix_ndw(bw)) = the group's words; M(o) is the frame's word at byte o. (bw is the page's, uniform over a
// workgroup: the tests of i against the word count are scalar, and q is indexed by constants only.)
template <class Mem>
PF_HD inline void fix_load(int bw, uint32_t off4, const Mem& M, uint32_t (&q)[FIX_NDW]) {
    const int ndw = fix_ndw(bw);
#ifdef __HIP_DEVICE_COMPILE__
    #pragma unroll
#endif
    for (int i = 0; i < FIX_NDW; i++)
        if (i < ndw) q[i] = M(off4 + 4u * uint32_t(i));
}

// The eight BW-bit ids that start at bit pos0 (< 32) of q. The words are first shifted down by pos0, after which id k
// lies at the constant bit k * BW.
template <int BW>
PF_HD inline void fix_unpack_n(const uint32_t (&q)[FIX_NDW], uint32_t pos0, uint32_t (&id)[8]) {
    static_assert(BW >= 1 && BW <= FIX_BW_MAX, "widths of the fast path");
    constexpr int NR = (8 * BW + 31) / 32;   // (q[NR] is a loaded word: fix_ndw(BW) > NR)
    constexpr uint32_t mask = (1u << BW) - 1u;
    uint32_t r[NR + 1];
#ifdef __HIP_DEVICE_COMPILE__
    #pragma unroll
#endif
    for (int i = 0; i < NR; i++) r[i] = uint32_t(((uint64_t(q[i + 1]) << 32) | uint64_t(q[i])) >> pos0);
    r[NR] = 0;
#ifdef __HIP_DEVICE_COMPILE__
    #pragma unroll
#endif
    for (int k = 0; k < 8; k++) {
        const int w = (k * BW) >> 5, s = (k * BW) & 31;
        uint32_t x = r[w] >> s;
        if (s + BW > 32) x |= r[w + 1] << ((32 - s) & 31);
        id[k] = x & mask;
    }
}
PF_HD inline void fix_unpack(int bw, const uint32_t (&q)[FIX_NDW], uint32_t pos0, uint32_t (&id)[8]) {
    switch (bw) {
        case 1: fix_unpack_n<1>(q, pos0, id); break;
        case 2: fix_unpack_n<2>(q, pos0, id); break;
        case 3: fix_unpack_n<3>(q, pos0, id); break;
        case 4: fix_unpack_n<4>(q, pos0, id); break;
        case 5: fix_unpack_n<5>(q, pos0, id); break;
        case 6: fix_unpack_n<6>(q, pos0, id); break;
        case 7: fix_unpack_n<7>(q, pos0, id); break;
        case 8: fix_unpack_n<8>(q, pos0, id); break;
        case 9: fix_unpack_n<9>(q, pos0, id); break;
        case 10: fix_unpack_n<10>(q, pos0, id); break;
        case 11: fix_unpack_n<11>(q, pos0, id); break;
        case 12: fix_unpack_n<12>(q, pos0, id); break;
        case 13: fix_unpack_n<13>(q, pos0, id); break;
        case 14: fix_unpack_n<14>(q, pos0, id); break;
        case 15: fix_unpack_n<15>(q, pos0, id); break;
        case 16: fix_unpack_n<16>(q, pos0, id); break;
        default: break;
    }
}

// id[k] = dictionary id of value e0 + k for k < n, anything for the others; false: the group is not fast and id is
// untouched.
template <class Rows, class Mem>
PF_HD inline bool fix_ids8(const Rows& R, uint32_t nr, uint32_t e0, uint32_t n, int bw, uint32_t mis, uint64_t ids_n,
                           const Mem& M, uint32_t (&id)[8]) {
    const FixGrp g = fix_locate(R, nr, e0, n, bw, mis, ids_n);
    if (g.kind == FIX_SLOW) return false;
    if (g.kind == FIX_CONST) {
        for (int k = 0; k < 8; k++) id[k] = g.val;
        return true;
    }
    uint32_t q[FIX_NDW] = {0, 0, 0, 0, 0};
    fix_load(bw, g.off4, M, q);
    fix_unpack(bw, q, g.val, id);
    return true;
}

}  // namespace pf
