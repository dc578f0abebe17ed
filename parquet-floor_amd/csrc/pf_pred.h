// pf_pred.h — the comparisons of a row filter (pf_decode_row_group_filter), one text for the kernel (pf_filter.hip)
// and for the host check (tests/native/pf_filter_check.cpp), shared like pf_xxh64.h and pf_zstd_core.h.
//   pred_cmp_bytes   unsigned bytewise, a proper prefix first: the order of Statistics / ColumnIndex for BYTE_ARRAY
//   pred_range_int   signed integers (INT32, INT64, BOOLEAN)
//   pred_range_real  IEEE lo <= v && v <= hi: NaN matches no bound, -0.0 equals +0.0 (FLOAT widened to double: exact)
//   pred_range_at    a packed PF_PRED_RANGE over value i of a column's arrays: a row of a decoded chunk (k_sel_mask), or
//                    an entry of a kept dictionary (k_sel_dict) -- the same text, so both routes match the same values
// A missing bound is unbounded. Unsigned and decimal logical orders are not covered.
#pragma once
#include <stdint.h>

#include "pf_internal.h"
#include "pfloor.h"

namespace pf {

// < 0: a before b, 0: equal, > 0: a after b
PF_HD inline int pred_cmp_bytes(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb) {
    const uint32_t n = na < nb ? na : nb;
    for (uint32_t i = 0; i < n; i++) {
        const int d = int(a[i]) - int(b[i]);
        if (d != 0) return d;
    }
    return na < nb ? -1 : (na > nb ? 1 : 0);
}

PF_HD inline bool pred_range_int(int64_t v, bool has_lo, int64_t lo, bool has_hi, int64_t hi) {
    return (!has_lo || lo <= v) && (!has_hi || v <= hi);
}

PF_HD inline bool pred_range_real(double v, bool has_lo, double lo, bool has_hi, double hi) {
    // (a NaN value or bound fails every comparison it takes part in; with both bounds missing every present row matches)
    return (!has_lo || lo <= v) && (!has_hi || v <= hi);
}

PF_HD inline bool pred_range_bytes(const uint8_t* v, uint32_t n, bool has_lo, const uint8_t* lo, uint32_t nlo, bool has_hi,
                                   const uint8_t* hi, uint32_t nhi) {
    return (!has_lo || pred_cmp_bytes(lo, nlo, v, n) <= 0) && (!has_hi || pred_cmp_bytes(v, n, hi, nhi) <= 0);
}

// The PF_PRED_RANGE predicate p over present value i of a column: values (fixed width) or offsets + chars (BYTE_ARRAY).
PF_HD inline bool pred_range_at(const DevPred& p, const uint8_t* values, const int32_t* offsets, const uint8_t* chars, int64_t i,
                                const uint8_t* blob) {
    const bool has_lo = p.flags & PRED_HAS_LO, has_hi = p.flags & PRED_HAS_HI;
    switch (p.ptype) {
    case PF_BOOLEAN: return pred_range_int(values[i], has_lo, p.lo_i, has_hi, p.hi_i);
    case PF_INT32: return pred_range_int(reinterpret_cast<const int32_t*>(values)[i], has_lo, p.lo_i, has_hi, p.hi_i);
    case PF_INT64: return pred_range_int(reinterpret_cast<const int64_t*>(values)[i], has_lo, p.lo_i, has_hi, p.hi_i);
    case PF_FLOAT: return pred_range_real(double(reinterpret_cast<const float*>(values)[i]), has_lo, p.lo_f, has_hi, p.hi_f);
    case PF_DOUBLE: return pred_range_real(reinterpret_cast<const double*>(values)[i], has_lo, p.lo_f, has_hi, p.hi_f);
    case PF_BYTE_ARRAY: {
        const int32_t a = offsets[i], b = offsets[i + 1];
        return pred_range_bytes(chars + a, uint32_t(b - a), has_lo, blob + p.lo_off, p.lo_len, has_hi, blob + p.hi_off, p.hi_len);
    }
    default: return false;
    }
}

}  // namespace pf
