// pf_page_tables.h — the per-page side tables in scratch through which the decode kernels pass work
// to each other: what each holds, how many bytes the planner (pf_plan.cpp) reserves for it and where
// its parts lie. Plain C++17: the kernels, the host planner and the native checks include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

// The host planner (pf_plan.cpp) includes this header from plain C++
#ifdef __HIPCC__
#define PF_HD __host__ __device__
#else
#define PF_HD
#endif

namespace pf {

constexpr uint32_t FBLK = 4096;            // entries per (page, block) pair of the flat kernels

// ---- id run table (DevPage::runtab): dictionary data page of a flat chunk, written by k_runs.
// A run's count is the next run's first - its first; the last run ends at `covered`.
#ifndef PF_RUN_CAP
#define PF_RUN_CAP 256
#endif
constexpr int RUN_CAP = PF_RUN_CAP;        // most runs k_runs writes and a reader accepts (their LDS tables)
struct IdRunTab {
    uint32_t nruns;
    uint32_t covered;                      // values the runs cover
    uint32_t valid;                        // 1: the rows are the page's id runs (indexed by value: pages with nulls hold
                                           // fewer ids than entries, the walk then ends with the stream)
    uint32_t all_present;                  // 1: valid and every definition level present (k_flat_fixed / k_flat split)
    uint32_t rows[2 * RUN_CAP];            // per run {first value | packed << 31, RLE value or bit offset of its first id}
    // The words of run i. Each word's index is computed on its own and in the caller's index type, as
    // the kernels always have (T[4 + 2 * i], T[5 + 2 * i]): an array of row structs makes the compiler
    // merge and re-base these accesses. next_first(i) is first(i + 1) as T[6 + 2 * i].
    template <class I> PF_HD uint32_t& fp(I i) { return (&nruns)[4 + 2 * i]; }
    template <class I> PF_HD uint32_t& data(I i) { return (&nruns)[5 + 2 * i]; }
    template <class I> PF_HD uint32_t fp(I i) const { return (&nruns)[4 + 2 * i]; }
    template <class I> PF_HD uint32_t data(I i) const { return (&nruns)[5 + 2 * i]; }
    template <class I> PF_HD uint32_t first(I i) const { return fp(i) & 0x7fffffffu; }
    template <class I> PF_HD uint32_t packed(I i) const { return fp(i) >> 31; }
    template <class I> PF_HD uint32_t next_first(I i) const { return (&nruns)[6 + 2 * i] & 0x7fffffffu; }
};
// Words of the head and the first nruns rows (k_lvl copies them to LDS)
PF_HD inline uint32_t id_tab_words(uint32_t nruns) {
    return uint32_t(offsetof(IdRunTab, rows) / 4) + 2 * nruns;
}
constexpr uint32_t RT_BYTES = 8208;        // reserved per table (more than it needs: every later scratch offset depends on it)
static_assert(offsetof(IdRunTab, rows) == 16 && sizeof(IdRunTab) <= RT_BYTES,
              "RUN_CAP runs fit the bytes the planner reserves");

// ---- level run table (DevPage::lvltab): nullable fixed-width page of a flat chunk, written by k_lvl:
// the head, DevPage::lvl_cap run rows, then one block row per FBLK entries (k_flat_null).
struct LvlHead {
    uint32_t nruns;
    uint32_t fit;                          // 1: the tables are valid and every block row fits k_flat_null's LDS stages
    uint32_t present;                      // present values of the page
    uint32_t pad;
};
struct LvlRun {
    uint32_t first;                        // first entry
    uint32_t data;                         // RLE value, or bit offset of the run's first level in the level section
    uint32_t cw;                           // count | packed << 31
    uint32_t before;                       // present values before the run
    PF_HD uint32_t count() const { return cw & 0x7fffffffu; }
    PF_HD uint32_t packed() const { return cw >> 31; }
};
struct LvlBlock {
    uint32_t r0, r1;                       // the runs the block overlaps: [r0, r1)
    uint32_t vb, ve;                       // value index of its first entry and of its end
    uint32_t d0, d1;                       // level bytes its packed runs read: [d0, d1)
    uint32_t i0, i1;                       // dictionary-id bytes of its values: [i0, i1)
};
constexpr uint32_t LT_BT_WORDS = 8;        // words of a block row
static_assert(sizeof(LvlHead) == 16 && sizeof(LvlRun) == 16 && sizeof(LvlBlock) == 4 * LT_BT_WORDS, "k_lvl table rows");
constexpr uint32_t LT_BLOCK_RUNS = 512;    // most runs one k_flat_null block may overlap (its LDS table)
constexpr uint32_t NL_DST = 4096;          // most level bytes one k_flat_null block stages in LDS
constexpr uint32_t NULL_DICT_LDS = 16384;   // k_flat_null stages dictionaries up to this many bytes in LDS
constexpr uint32_t NL_IST = 12288;         // most dictionary-id bytes one k_flat_null block stages in LDS
constexpr uint32_t NL_SLACK = 256;         // run-header bytes a block's level / id byte range may add
// k_flat_null's dynamic LDS, per batch: level bytes (dcap), dictionary-id bytes (icap) a block may
// stage -- from the batch's widest level / id bit width (host-known: max definition level, dictionary
// size), FBLK values of it + NL_SLACK, at most NL_DST / NL_IST; k_lvl's block rows are checked against
// the same caps -- and the dictionary bytes it stages (dlds, 0: none). Multiples of 16.
struct NullCaps {
    uint32_t dcap, icap, dlds;
};
PF_HD inline uint32_t lvl_table_cap(int32_t num_values) {
    // RLE runs are >= 8 repeats and bit-packed groups 8 values for the writers we know (parquet-mr,
    // Arrow): <= 2 runs per 16 entries; a page needing more is left to k_flat / k_decode
    return uint32_t(num_values) / 8u + 64u;
}
PF_HD inline LvlRun* lvl_runs(LvlHead* t) { return reinterpret_cast<LvlRun*>(t + 1); }
// Run row r of `runs` (the table's, or a copy in LDS) and block row blk, their word indices in 32-bit
// arithmetic (runs[4 * r + k]) as the kernels always have
template <class Row> PF_HD inline Row& lvl_run(Row* runs, uint32_t r) {
    return *(Row*)((const uint32_t*)runs + 4 * r);
}
PF_HD inline LvlBlock* lvl_block(LvlHead* t, uint32_t lvl_cap, uint32_t blk) {
    return reinterpret_cast<LvlBlock*>(reinterpret_cast<uint32_t*>(t + 1) + 4 * lvl_cap + LT_BT_WORDS * blk);
}
PF_HD inline uint64_t lvl_table_bytes(int32_t num_values) {
    return sizeof(LvlHead) + sizeof(LvlRun) * uint64_t(lvl_table_cap(num_values)) +
           sizeof(LvlBlock) * (uint64_t(num_values) / FBLK + 1);
}

// ---- block chars (behind DevPage::aux of a BYTE_ARRAY data page): after the page's aux_cap + 1 aux
// words (value positions or dictionary ids), 8-byte aligned, one u64 per FBLK entries: the chars of
// the block (k_count_dict), then of the entries before it (k_count_flat, k_count).
constexpr uint64_t BC_BAD = ~0ull;         // a block's chars word when one of its ids is out of the dictionary
PF_HD inline uint64_t* block_chars(uint32_t* aux, int64_t aux_cap) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(aux + aux_cap + 1);
    return reinterpret_cast<uint64_t*>((a + 7) & ~uintptr_t(7));
}
PF_HD inline uint64_t aux_chars_bytes(uint64_t num_values) {   // the aux words and the block chars
    return 4 * num_values + 16 + 8 * (num_values / FBLK + 2);
}

// ---- DELTA length tables (DevPage::dx; k_dlen, pf_delta.hip), u64 each, cap = DevPage::aux_cap:
// cpos[k] = chars of values [0, k), len_a[k] = DELTA_LENGTH_BYTE_ARRAY length / DELTA_BYTE_ARRAY prefix
// length, len_b[k] = DELTA_BYTE_ARRAY suffix length.
PF_HD inline uint64_t* dx_cpos(uint64_t* dx) { return dx; }                                 // [cap + 1]
PF_HD inline uint64_t* dx_len_a(uint64_t* dx, uint64_t cap) { return dx + cap + 1; }         // [cap]
PF_HD inline uint64_t* dx_len_b(uint64_t* dx, uint64_t cap) { return dx + cap + 1 + cap; }   // [cap]
PF_HD inline uint64_t dx_bytes(uint64_t num_values) { return 8 * (3 * num_values + 1); }

// ---- block-parallel DELTA_BINARY_PACKED tables (DevPage::dbp; k_dbp_*, pf_delta.hip), bcap =
// DevPage::dbp_bcap: the blocks' header positions, then (8-byte aligned) their delta sums, later bases.
struct DbpTabs {
    uint32_t* pos;                         // [bcap]
    uint64_t* sum;                         // [bcap]
};
PF_HD inline DbpTabs dbp_tabs(uint8_t* dbp, uint32_t bcap) {
    return {reinterpret_cast<uint32_t*>(dbp), reinterpret_cast<uint64_t*>(dbp + 4ull * bcap + 8 - ((4ull * bcap) & 7))};
}
PF_HD inline uint64_t dbp_bytes(uint32_t bcap) { return 12ull * bcap + 16; }

}  // namespace pf
