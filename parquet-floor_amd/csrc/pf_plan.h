// pf_plan.h — host-only planning of one decode batch (pf_plan.cpp). Plain C++: no HIP runtime
// call, no context, not a byte of the input read -- only arithmetic on the descriptors, so the
// routing of every page can be checked without a GPU (tests/native/pf_plan_check.cpp).
//
//   plan_batch  descriptors -> DevChunk / DevPage / SnappyJob / ZstdJob / Lz4Job / BaJob tables, the launch lists and
//               grids, the arena sizes and the metadata layout; which chunks keep their dictionary. Offsets only.
//   bind_batch  offsets -> device pointers, given where the runtime allocated the arenas.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pf_internal.h"
#include "pfloor.h"

namespace pf {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bytes per value of a physical type (0: BYTE_ARRAY, -1: unsupported).
int type_width(int ptype, int type_length);

// The launch lists of a batch, in the order they lie in the metadata block (one int array).
// L_FLAT, L_NSEG and L_CDICT hold (page, block / segment) pairs.
enum ListId {
    L_DELTA,    // DELTA_BINARY_PACKED INT32 / INT64 pages (k_delta, k_dbp_*)
    L_COUNT,    // pages of chunks that need counts: the n_count_flat flat BYTE_ARRAY pages first
    L_SCAN,     // chunks that need k_scan
    L_FLAT,     // four (page, block) grids: k_flat_fixed, k_flat_all, k_flat_null<4>, <8>
    L_DECODE,   // every data page: the n_decode_first pages that will need k_decode first
    L_RUNS,     // pages with a dictionary-id run table (k_runs)
    L_DLEN,     // DELTA_LENGTH_BYTE_ARRAY / DELTA_BYTE_ARRAY pages (k_dlen)
    L_DBA,      // DELTA_BYTE_ARRAY pages (k_dba_chars)
    L_LVL,      // pages with a definition-level run table (k_lvl)
    L_DJOBS,    // Snappy jobs that are k_snappy_litcopy candidates
    L_NEST,     // nested pages decoded in segments (k_nest_lvl)
    L_NSEG,     // their (page, segment) pairs
    L_CDICT,    // (page, block) pairs of flat dictionary BYTE_ARRAY pages (k_count_dict)
    L_ZSTD,     // ZSTD jobs in dispatch order: the most compressed bytes first (k_zstd)
    L_LZ4,      // LZ4_RAW jobs in dispatch order: the most compressed bytes first (k_lz4)
    L_IDS,      // (page, block) pairs of the data pages of kept-dictionary chunks, FBLK entries each (k_flat_ids)
    N_LISTS
};

constexpr uint64_t NO_OFF = ~0ull;

// Where a page's regions lie (NO_OFF: the page has none).
struct PagePlan {
    uint64_t in_off;        // the page's first body byte in the input (v2: its levels)
    uint64_t scratch_off;   // decompressed body (Snappy, ZSTD and LZ4_RAW pages), 16-byte aligned
    uint64_t aux_off;       // BYTE_ARRAY value positions / ids, DELTA_BINARY_PACKED values, dictionary pos + len
    uint64_t rt_off;        // k_runs table
    uint64_t dx_off;        // k_dlen tables
    uint64_t lt_off;        // k_lvl tables
    uint64_t seg_off;       // nested segment records
    uint64_t pub_off;       // ... and their window hand-overs, relative to off_npub
    uint64_t dbp_off;       // k_dbp_* block tables
    uint64_t dbp_pub_off;   // ... and their window hand-overs, relative to off_npub
};

// Where a chunk's output arrays lie: values, offsets, list offsets and levels in the out arena,
// validity and list validity in the bits arena (NO_OFF: the chunk has none).
struct OutPlan {
    uint64_t values, validity, offsets, list_offsets, list_validity, def, rep;
};

// Snappy tables of a set of jobs: 8 KiB index windows and 64 KiB pieces. The tokmap arena holds,
// per window, 1 KiB of token-start bitmap, then 64 lane output counts, then the SnapWin records,
// then the entry tables; the index pass writes every word, so nothing needs clearing.
struct SnappyPlan {
    std::vector<Int2> wins, pieces;   // (job, window) / (job, piece), pieces in dispatch order
    uint32_t n_splits = 0;
    int max_snap_win = 1;             // index windows of the largest job (k_snappy_chain's tables)
    size_t off_lane_out = 0, off_win = 0, off_ent = 0, tokmap_bytes = 0;
    // bound
    uint32_t* d_lane_out = nullptr;
    SnapWin* d_win = nullptr;
    SnapEnt* d_ent = nullptr;
};
void plan_snappy(std::vector<SnappyJob>& jobs, SnappyPlan& sp);
void bind_snappy(std::vector<SnappyJob>& jobs, SnappyPlan& sp, uintptr_t tokmap);

// Base addresses of the arenas of a batch.
struct ArenaBases {
    uintptr_t in, scratch, out, bits, meta, tokmap;
};

// A kept-dictionary chunk (pf_decode_row_group_dict): its index width and where its dictionary's output arrays lie
// in the out arena (NO_OFF: it has none; the chars of a BYTE_ARRAY dictionary are placed on the device).
struct KeepPlan {
    int32_t chunk, index_width;
    int64_t n_entries;
    int32_t width;            // bytes per dictionary entry, 0 for BYTE_ARRAY
    uint64_t values, offsets;
};
// 1, 2 or 4: the smallest index that holds n_entries - 1.
inline int dict_index_width(int64_t n_entries) { return n_entries <= 256 ? 1 : (n_entries <= 65536 ? 2 : 4); }
// The eligibility rule of pf_decode_row_group_dict (include/pfloor.h), from the descriptor alone.
bool keep_eligible(const pf_chunk_desc& cd);

// Everything one batch needs between its descriptors and its launches.
struct BatchPlan {
    int n_chunks = 0;
    std::vector<DevChunk> chunks;          // host copies (device pointers once bound)
    std::vector<DevPage> pages;
    std::vector<SnappyJob> jobs;
    std::vector<ZstdJob> zjobs;            // ZSTD pages (k_zstd); L_ZSTD is their dispatch order
    std::vector<Lz4Job> ljobs;             // LZ4_RAW pages (k_lz4); L_LZ4 is their dispatch order
    std::vector<BaJob> bajobs;             // PLAIN BYTE_ARRAY walks: dictionary pages, then data pages
    std::vector<Int2> ba_tiles;            // (job relative to its half, tile)
    SnappyPlan snap;
    std::vector<int64_t> host_status;      // per chunk: planning error, 0 if none
    std::vector<int> lists[N_LISTS];
    size_t list_base[N_LISTS + 1] = {};    // first int of each list in the metadata block's list array
    int n_decode_first = 0, n_count_flat = 0;
    int n_flat_fixed = 0, n_flat_all = 0, n_null4 = 0, n_null8 = 0;   // grid lengths within L_FLAT, in pairs
    int n_ba_dict = 0, n_ba_dict_tiles = 0;
    bool ba_short_dict = true, ba_short_data = true;   // every walk's values average <= BA_SHORT bytes: k_ba_tile
    int max_nwin = 0, max_dbp_nwin = 0;
    NullCaps null_caps{16, 16, 0};         // k_flat_null's level / id byte stages and its dictionary stage
    // arenas
    size_t scratch_bytes = 0, out_bytes = 0, bits_bytes = 0;
    size_t off_npub = 0, npub_bytes = 0;   // window hand-overs (scratch), zeroed before the batch
    // k_zstd's literal areas (scratch): one of zlit_stride bytes per resident workgroup, not per page
    size_t off_zlit = 0;
    uint32_t zlit_stride = 0, zstd_grid = 0;
    uint64_t chars_hint = 0;               // uncompressed bytes of the BYTE_ARRAY data pages
    // metadata block; its last 256 bytes hold the chars arena counter
    size_t off_chunks = 0, off_pages = 0, off_jobs = 0, off_lists = 0, off_res = 0, off_pieces = 0, off_splits = 0,
           off_fallback = 0, off_wins = 0, off_bajobs = 0, off_batiles = 0, off_nfbq = 0, off_zjobs = 0, off_ljobs = 0, meta_bytes = 0;
    std::vector<PagePlan> pplan;           // per page
    std::vector<OutPlan> oplan;            // per chunk
    std::vector<uint64_t> ba_bm;           // per BaJob: its bitmaps and tile counts (scratch)
    // kept dictionaries: the kept chunks in chunk order, each chunk's entry in `keeps` (-1: not kept), and the
    // device tables DevKeep[keeps.size()] and int keep_of[n_chunks] behind the other metadata (bound by bind_batch)
    std::vector<KeepPlan> keeps;
    std::vector<int32_t> keep_of;
    std::vector<DevKeep> dkeeps;
    size_t off_keeps = 0, off_keepof = 0;
};

// keep: one flag per chunk (pf_decode_row_group_dict), nullptr: none is kept -- the plan of pf_decode_row_group.
void plan_batch(const pf_chunk_desc* cds, int n_chunks, size_t n_bytes, const PfOpts& opts, BatchPlan& p,
                const uint8_t* keep = nullptr);
void bind_batch(BatchPlan& p, const ArenaBases& a);

// The predicates of a filtered decode, validated and packed for the device: the DevPred table and, behind it, the
// blob that holds the BYTE_ARRAY bounds (DevPred.lo_off / hi_off). Reads the descriptors and the bounds, nothing else.
// dicts / dict_of / dict_words (plan_filter_dict): the PF_PRED_RANGE predicates on kept chunks, each with a match bitmap
// over its dictionary's entries; all empty / 0 for a batch without one, whose filter stage is then what it always was.
struct FilterPlan {
    std::vector<DevPred> preds;
    std::vector<uint8_t> blob;
    std::vector<DevSelDict> dicts;
    std::vector<int32_t> dict_of;          // per predicate: its entry in dicts, -1; empty when dicts is
    uint64_t dict_words = 0;               // 64-bit words of all bitmaps
    int64_t dict_max_entries = 0;          // entries of the largest dictionary among dicts
};
// PF_OK, or the call error of pf_decode_row_group_filter with its text in *why (f is then empty).
int plan_filter(const pf_chunk_desc* cds, int n_chunks, const pf_predicate* preds, int n_preds, FilterPlan& f, const char** why);
// After plan_batch: which of f's predicates are resolved through a kept dictionary (p.keep_of), and where their bitmaps
// of ceil(n_entries / 64) words lie, back to back in predicate order. IS_NULL / NOT_NULL read the validity only and get
// none. Reads the plan, nothing else.
void plan_filter_dict(const BatchPlan& p, FilterPlan& f);

}  // namespace pf
