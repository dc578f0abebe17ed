// pf_sel.h — what the two translation units of the filter stage share on the device (pf_filter.hip, pf_filter_dict.hip):
// the tile shape of the k_sel_* kernels and the evaluation of one predicate on one row of a decoded chunk.
#pragma once
#include "pf_internal.h"
#include "pf_pred.h"

namespace pf {

constexpr int SB = 256;                           // threads of every kernel
constexpr int SEL_WORDS = int(SEL_TILE / 64);     // mask words of a tile
constexpr int SEL_WPW = SEL_WORDS / 4;            // ... of one wave: rows [wave * 64 * SEL_WPW, + 64 * SEL_WPW) of the tile
static_assert(SEL_TILE % 256 == 0 && SEL_TILE >= 256, "a tile is whole mask words for each of four waves");

__device__ __forceinline__ bool sel_present(const DevSelChunk& c, int64_t r) {
    return !(c.max_def > 0 && c.validity) || ((c.validity[r >> 3] >> (r & 7)) & 1);
}

__device__ __forceinline__ bool eval_row(const DevPred& p, const DevSelChunk& c, int64_t r, const uint8_t* __restrict__ blob) {
    const bool present = sel_present(c, r);
    if (p.op == PF_PRED_IS_NULL) return !present;
    if (p.op == PF_PRED_NOT_NULL || !present) return present;
    return pred_range_at(p, c.values, c.offsets, c.chars, r, blob);
}

}  // namespace pf
