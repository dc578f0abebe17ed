// pf_filter_dict.hip — predicates over kept dictionaries (pf_decode_row_group_dict_filter; gfx950, wave64).
// A kept chunk goes through the filter stage as what it is: a fixed-width column of index_width-byte indices with a
// validity bitmap (k_sel_prep sizes it from the DevKeep table), plus a dictionary that nobody moves. A PF_PRED_RANGE on
// such a chunk is matched once per dictionary entry and then looked up per row:
//   k_sel_dict       grid (entry tile, kept RANGE predicate): one lane per entry evaluates the predicate with the text
//                    the row-wise route uses (pred_range_at, pf_pred.h); ballots give the words of the match bitmap
//   k_sel_mask_dict  launched in place of k_sel_mask when some predicate is on a kept chunk: for such a predicate a
//                    present row loads its index and tests one bit of the bitmap; every other predicate is eval_row
// The bitmaps lie in global memory (SelDictBufs.bits): a small one is a few words every lane reads through the same
// cache lines, a 65537-entry one is 8 KiB that stays in L2. Like the rest of the stage: 256 threads, no atomics (but
// the diagnostics build's counters), sizes the device knows meet grids the host sized.
#include "pf_launch.h"
#include "pf_sel.h"

namespace pf {

#ifdef PF_DIAG   // diagnostics build: predicates resolved through a dictionary, dictionary entries evaluated (tests)
__device__ unsigned long long pf_sel_dict_counts[2];
extern "C" int pf_debug_sel_dict_counts(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pf_sel_dict_counts), sizeof(unsigned long long) * 2) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pf_sel_dict_counts), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#define SELD_COUNT(i, n) (threadIdx.x == 0 ? (void)atomicAdd(&pf_sel_dict_counts[i], (unsigned long long)(n)) : (void)0)
#else
#define SELD_COUNT(i, n) ((void)0)
#endif

namespace {

static_assert(SELD_TILE == uint32_t(SB), "one dictionary entry per thread, one bitmap word per wave");

// Entries [blockIdx.x * SELD_TILE, + SELD_TILE) of the dictionary of predicate record blockIdx.y. A predicate whose
// chunk failed (a chars arena overflow that the batch will rerun for is such a failure: d_chars is null then) writes
// nothing. An entry past the dictionary's end is no match, so the tail bits of the last word are zero.
__global__ __launch_bounds__(SB) void k_sel_dict(SelBufs f, SelDictBufs fd) {
    const DevSelDict rec = fd.recs[blockIdx.y];
    const DevPred& p = f.preds[rec.pred];
    if (f.sc[p.chunk].status != 0) return;
    const int64_t base = int64_t(blockIdx.x) * SELD_TILE;
    if (blockIdx.x == 0) SELD_COUNT(0, 1);
    if (base >= rec.n_entries) return;   // (an empty dictionary: nothing to evaluate, no word to write)
    const DevKeep& kp = fd.keeps[rec.keep];
    const bool ba = p.ptype == PF_BYTE_ARRAY;
    if (ba ? (!kp.d_offsets || !kp.d_chars) : !kp.d_values) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t e = base + tid;
    SELD_COUNT(1, rec.n_entries - base < int64_t(SELD_TILE) ? rec.n_entries - base : int64_t(SELD_TILE));
    const bool m = e < rec.n_entries && pred_range_at(p, kp.d_values, kp.d_offsets, kp.d_chars, e, f.blob);
    const uint64_t w = __ballot(m);
    const uint64_t word = uint64_t(base / 64) + uint64_t(wave);
    if (lane == 0 && word < rec.n_words) fd.bits[rec.word_off + word] = w;
}

// k_sel_mask with the dictionary route: the same tiles, words and counts.
__global__ __launch_bounds__(SB) void k_sel_mask_dict(SelBufs f, SelDictBufs fd) {
    const int64_t rows_in = f.head->rows_in;   // 0 when the stage failed
    const int64_t tile = blockIdx.x, base = tile * SEL_TILE;
    if (base >= rows_in) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ uint32_t s_cnt[4];
    uint32_t cnt = 0;
    #pragma unroll 1
    for (int k = 0; k < SEL_WPW; k++) {
        const int word = wave * SEL_WPW + k;
        const int64_t r = base + word * 64 + lane;
        bool m = r < rows_in;
        for (int i = 0; i < f.n_preds; i++) {
            if (!m) continue;
            const DevPred& p = f.preds[i];
            const DevSelChunk& c = f.sc[p.chunk];
            const int32_t d = fd.dict_of[i];
            if (d < 0) { m = eval_row(p, c, r, f.blob); continue; }
            m = sel_present(c, r);   // a null row matches no range, and its index 0 is never looked up
            if (m) {
                const DevSelDict& rec = fd.recs[d];
                const uint64_t idx = c.width == 1 ? uint64_t(c.values[r])
                                   : c.width == 2 ? uint64_t(reinterpret_cast<const uint16_t*>(c.values)[r])
                                                  : uint64_t(reinterpret_cast<const uint32_t*>(c.values)[r]);
                m = idx < uint64_t(rec.n_entries) && ((fd.bits[rec.word_off + (idx >> 6)] >> (idx & 63)) & 1ull);
            }
        }
        const uint64_t w = __ballot(m);
        if (lane == 0) f.mask[tile * SEL_WORDS + word] = w;
        cnt += uint32_t(__popcll(w));
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) f.tile_count[tile] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

}  // namespace

void launch_sel_dict(const SelBufs& f, const SelDictBufs& fd, unsigned row_tiles, hipStream_t st) {
    if (fd.n_recs <= 0) return;
    hipLaunchKernelGGL(k_sel_dict, dim3(unsigned(fd.tiles < 1 ? 1 : fd.tiles), unsigned(fd.n_recs)), dim3(SB), 0, st, f, fd);
    hipLaunchKernelGGL(k_sel_mask_dict, dim3(row_tiles < 1 ? 1 : row_tiles), dim3(SB), 0, st, f, fd);
}

}  // namespace pf
