// pf_result.h — host-only result side of one decode batch (pf_result.cpp), next to its planner (pf_plan.h). Plain
// C++: no HIP runtime call and no context, so everything here is checked without a GPU
// (tests/native/pf_result_check.cpp).
//
//   layouts     where the side tables of a batch lie: the results block, the window tables, the filter stage's
//               buffer, the host layout of a batch copy. Each is computed once and read by every user.
//   decisions   the arena sizes of a batch, whether growing them must wait for a pending copy, whether a chars
//               overflow runs the batch again.
//   assembly    the decode's, the window's and the selection's view of every chunk merged into pf_column_info.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "pf_internal.h"
#include "pf_plan.h"
#include "pfloor.h"

namespace pf {

// The pinned results block: [DevChunkResult[n] | pad to 256 | DevChunk[n] as the device left them | 256 spare].
struct ResLayout {
    size_t res_bytes, chunks_off, chunks_bytes, total;
};
ResLayout res_layout(int n_chunks);

// The window tables, on the device and in their pinned mirror: [DevWin[n] up | pad to 256 | DevWinRes[n] down].
struct WinLayout {
    size_t wins_bytes, res_off, res_bytes, total;
};
WinLayout win_layout(int n_wins);
// k_win_copy's workgroups per chunk stride over its tiles: a bound from the host's counts, at most 512.
int win_grid(const BatchPlan& p, const std::vector<DevWin>& wins);

// Twin arena base - decode arena base, in bytes: a chunk keeps its offsets in the twins.
struct TwinDelta {
    int64_t out = 0, bits = 0;
};

// The filter stage's buffer. [head | DevSelChunk[n]] comes down (the bytes below o_up), [DevPred[] | blob | win_of[n]]
// goes up ([o_up, up_end)), the rest is the kernels' own. Every region is 256-byte aligned.
struct SelLayout {
    size_t o_head = 0, o_sc = 0, o_up = 0, o_preds = 0, o_blob = 0, o_winof = 0, up_end = 0;
    size_t o_mask = 0, o_tc = 0, o_tb = 0, o_rows = 0, o_bs = 0, o_bb = 0, o_bt = 0, total = 0;
    // predicates resolved through kept dictionaries (FilterPlan.dicts; none: every field is 0 and the fields above are
    // what they are without): [DevSelDict[] | dict_of[n_preds]] behind win_of in the uploaded part, the match bitmaps
    // (dict_words 64-bit words) behind ba_total
    size_t o_drec = 0, o_dof = 0, o_dbits = 0;
    int dict_tiles = 0;              // k_sel_dict's grid.x: SELD_TILE tiles of the largest dictionary, at least one
    int64_t rows_cap = 0;            // bounds rows_in: the first predicate chunk's rows after its window
    size_t tiles = 1;                // SEL_TILE tiles of rows_cap, at least one
    int grid = 1;                    // the gather kernels' workgroups: min(tiles, 256)
    std::vector<int32_t> win_of;     // per chunk: its entry in wins, -1 without one
};
SelLayout layout_filter(const BatchPlan& p, const FilterPlan& f, const std::vector<DevWin>& wins);
// The uploaded tables into the pinned mirror h (up_end bytes, zeroed first).
void fill_filter(const SelLayout& l, const FilterPlan& f, uint8_t* h);
// The stage's pointers for a buffer at `base`.
SelBufs bind_sel(const SelLayout& l, const FilterPlan& f, uintptr_t base);
// The dictionary route's pointers (n_recs = 0 and no tables without FilterPlan.dicts); keeps / keep_of: the batch's
// DevKeep[] and keep_of[] on the device (null: nothing kept), passed on as they are.
SelDictBufs bind_sel_dict(const SelLayout& l, const FilterPlan& f, uintptr_t base, const DevKeep* keeps, const int32_t* keep_of);

// Arena capacities a batch asks for (out: before the "at least one byte" of its allocation).
struct ArenaNeeds {
    size_t out, bits, chars;
};
ArenaNeeds arena_needs(const BatchPlan& p, uint64_t chars_need, bool twins);
struct ArenaCaps {
    size_t out, bits, chars, wout, wbits, wchars;
};
// True: an arena (or, with twins, a twin below its decode arena's size) will be reallocated, so a pending copy out of
// them must have finished on the host first. False: the stream waiting on the copy's event is enough.
bool arenas_grow(const ArenaNeeds& n, const ArenaCaps& c, bool twins);

// A chars arena overflow that one more run with `need` bytes (+ the caller's slack) cures.
struct CharsOverflow {
    bool rerun;
    uint64_t need;
};
CharsOverflow chars_overflow(const BatchPlan& p, const DevChunkResult* r);

// What came down from the device for one batch. n_wins 0 without windows, sel_head nullptr without a filter.
struct BatchResults {
    const DevChunkResult* res;       // [n_chunks]
    const DevChunk* dev_chunks;      // [n_chunks] the device-written copies (chars)
    const DevWin* wins;              // [n_wins], chunks ascend
    const DevWinRes* wres;           // [n_wins]
    size_t n_wins;
    TwinDelta twin;
    const DevSelHead* sel_head;
    const DevSelChunk* sel_chunks;   // [n_chunks]
    const int32_t* sel_rows;         // SelBufs.rows
    const DevKeep* keeps = nullptr;  // [p.keeps.size()] as the device left them (d_chars, num_chars); nullptr: none kept
};
struct FirstError {
    int code = PF_OK;
    std::string msg;                 // "chunk %d: decode failed (status %d, page %d)" of the lowest failing chunk
};
// info[n_chunks]: the decode's view; the window's where the decode is OK and the window is not an identity; the
// selection's over that. A failed stage's status stands, the earliest stage first. *sel_info is written for a filtered
// batch with at least one chunk.
// dinfo[n_chunks] (optional): every chunk's pf_dict_info; a kept chunk's info has width = its index width, no offsets
// or chars and num_chars = 0.
FirstError assemble_info(const BatchPlan& p, const BatchResults& in, pf_column_info* info, pf_selection_info* sel_info,
                         pf_dict_info* dinfo = nullptr);

// Host layout of pf_copy_batch_async: [out arena | bits arena | chars arena], each 256-B aligned.
struct BatchLayout {
    size_t out, bits_off, bits, chars_off, chars, total;
};
// dicts (optional): the kept dictionaries, whose chars lie in the chars arena too.
BatchLayout batch_layout(const BatchPlan& p, const std::vector<pf_column_info>& info, const void* d_chars,
                         const std::vector<pf_dict_info>* dicts = nullptr);
// A device pointer into one of the three arenas as the host address of the same byte in a batch copy at `host`
// (an arena's end included); nullptr for nullptr and for a pointer outside every arena.
struct ArenaPtrs {
    const void *out, *bits, *chars;
};
const void* rebase(const BatchLayout& b, const ArenaPtrs& a, const void* host, const void* q);
pf_column_info rebase_info(const BatchLayout& b, const ArenaPtrs& a, const void* host, pf_column_info ci);
pf_dict_info rebase_dict(const BatchLayout& b, const ArenaPtrs& a, const void* host, pf_dict_info di);

// The eight arrays of a chunk against the caller's buffers: n bytes from src into dst of cap bytes.
struct CopyItem {
    void* dst;
    size_t cap;
    const void* src;
    size_t n;
    bool wanted() const { return dst && src; }
};
void copy_items(const pf_column_info& ci, const pf_column_out& o, CopyItem items[8]);
// The three arrays of a kept dictionary (values, offsets, chars) against the caller's buffers.
void dict_copy_items(const pf_dict_info& di, const pf_column_out& o, CopyItem items[3]);

}  // namespace pf
