// pf_dstr_ids.h — the dictionary ids of 16 consecutive values from a page's id run table, one text for the kernel
// (k_flat_dstr, pf_flat_dstr.hip) and for the host check (tests/native/pf_dstr_ids_check.cpp), shared like pf_pred.h.
//
// The run table is k_runs' (pf_flat_count.hip): row i = {first value | packed << 31, RLE value or the bit offset of the
// run's packed values in the id stream}; a run ends where the next one starts, the last one at `cov`.
// The id stream is read through a word loader W: W(w) is the little-endian 32-bit word w of a frame in which stream
// bit b is frame bit b + bias (the kernel's frame is its LDS stage, which starts at a 16-byte aligned address at
// or before the block's first id byte). Frame bytes past the stream's end must read as zero (parquet-mr zero-pads a
// truncated bit-packed run), and W(w + 1) must be loadable for every word w that holds a wanted bit.
#pragma once
#include <stdint.h>

#include "pf_internal.h"

namespace pf {

// Index of the run holding value e (rows sorted by first value, row 0 starts at 0).
PF_HD inline uint32_t dstr_run_at(const uint32_t* rt, uint32_t nr, uint32_t e) {
    uint32_t lo = 0, hi = nr;
    while (hi - lo > 1) {
        const uint32_t m = (lo + hi) >> 1;
        if ((rt[2 * m] & 0x7fffffffu) <= e) lo = m; else hi = m;
    }
    return lo;
}

// id[k] = dictionary id of value e0 + k for k < n (n <= 16), 0 for the others and for values at or past `cov`.
// One run lookup, then the runs in order: run boundaries anywhere inside the 16, RLE runs, widths 0 to 32.
template <class Words>
PF_HD inline void dstr_ids16(const uint32_t* rt, uint32_t nr, uint32_t cov, uint32_t e0, uint32_t n, int bw, int64_t bias,
                             const Words& W, uint32_t (&id)[16]) {
    const uint64_t mask = bw >= 32 ? 0xffffffffull : ((1ull << bw) - 1ull);
    uint32_t r = nr ? dstr_run_at(rt, nr, e0) : 0u;
    uint32_t first = 0, end = 0, data = 0, packed = 0;
    if (nr) {
        const uint32_t f = rt[2 * r];
        first = f & 0x7fffffffu;
        packed = f >> 31;
        data = rt[2 * r + 1];
        end = r + 1 < nr ? (rt[2 * r + 2] & 0x7fffffffu) : cov;
    }
#ifdef __HIP_DEVICE_COMPILE__
    #pragma unroll
#endif
    for (uint32_t k = 0; k < 16; k++) {
        id[k] = 0;
        const uint32_t e = e0 + k;
        if (k >= n || e >= cov || nr == 0) continue;
        while (e >= end && r + 1 < nr) {   // (empty runs are not in the table; a run may still be one value)
            r++;
            const uint32_t f = rt[2 * r];
            first = f & 0x7fffffffu;
            packed = f >> 31;
            data = rt[2 * r + 1];
            end = r + 1 < nr ? (rt[2 * r + 2] & 0x7fffffffu) : cov;
        }
        if (!packed || bw == 0) { id[k] = packed ? 0u : data; continue; }   // (width 0: no stream bit is read)
        const uint64_t fb = uint64_t(int64_t(uint64_t(data) + uint64_t(e - first) * uint64_t(bw)) + bias);
        const uint32_t wi = uint32_t(fb >> 5), sh = uint32_t(fb & 31u);
        const uint64_t x = (uint64_t(W(wi)) | (uint64_t(W(wi + 1u)) << 32)) >> sh;
        id[k] = uint32_t(x & mask);
    }
}

}  // namespace pf
