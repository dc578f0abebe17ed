// pf_internal.h — device-side work descriptors shared by the HIP kernels, the host planner
// (pf_plan.cpp) and the host runtime (pf_runtime.hip). Not part of the C ABI.
//
// HBM layout of one decode batch (one pf_decode_row_group call):
//   in      : the caller's chunk bytes (resident, or one H2D copy of the pinned buffer)
//   scratch : decompressed page bodies, 16-B aligned, in page order (k_snappy writes,
//             the page kernels read); per-page BYTE_ARRAY value positions / dict ids
//   out     : per chunk: values | validity | offsets | chars | list offsets | levels,
//             each array 256-B aligned inside one arena
//   meta    : DevChunk[], DevPage[], DevChunkResult[] (small)
#pragma once
#include <stdint.h>

#include "pf_page_tables.h"   // PF_HD, FBLK and the per-page side tables

namespace pf {

// (a, b) index pair of the launch tables: (job, window), (job, piece), (job, tile), (page, block),
// (page, segment). Laid out as HIP's int2, which is how the kernels read it.
struct Int2 {
    int x, y;
};

// Decoder options. The product library (libpfloor.so) always runs these defaults and reads no
// environment. The diagnostics build (-DPF_DIAG, diag/libpfloor_diag.so) takes them from PF_*
// environment variables once per context, at pf_ctx_create: A/B selectors for the tools and the
// switches tests use to force rare paths (forced fallbacks, segment lengths, skipped stages).
struct PfOpts {
    int exec = 5;             // PF_EXEC: block-parallel Snappy executor: 5 producer / consumer (pf_snappy_exec.hip) |
                              // 2 one wave (pf_snappy_exec2.hip, diagnostics build only)
    bool ba_fused = true;     // PF_BA_FUSED=0: the round-3 PLAIN BYTE_ARRAY walk kernels
    bool page_null = false;   // PF_PAGE_NULL=1: k_page_null before k_lvl
    int null_stagger = 0;     // PF_DEBUG_NULL_STAGGER=k: k_flat_null's blocks > 0 wait k rounds (race tests)
    bool nest_timeout = false;   // PF_DEBUG_NEST_TIMEOUT=1: every k_nest_lvl hand-over times out (whole-page path; tests)
    uint32_t null_dcap = 0;   // PF_NULL_DCAP=b: k_flat_null's level-byte stage instead of the batch's (16: blocks with
                              // level bytes do not fit, so k_lvl refuses the page and the fallback queue decodes it; tests)
    unsigned debug_skip = 0;  // PF_DEBUG_SKIP=parse,exec,ba,levels,count,flat,decode (results are wrong)
    int force_serial = 0;     // PF_DEBUG_FORCE_SERIAL=k: every k-th Snappy job to the serial kernel
    int force_redo = 0;       // PF_DEBUG_FORCE_REDO=k: every k-th Snappy job rejected by the block executor
    bool zc = true;           // PF_ZC=0: SDMA copies for the batch tables instead of k_copy_words
    bool dl_kernel = true;    // PF_DL_KERNEL=0: pf_copy_batch_async by SDMA copies instead of k_download
    bool h2d_kernel = false;  // PF_H2D_KERNEL=1: pinned chunk bytes to the device by a kernel instead of SDMA (E2E: no gain, r06)
    int h2d_grid = 256;       // PF_H2D_GRID: that kernel's workgroups (fewer: a slower upload beside the downloads)
    bool dl_stream = true;    // PF_DL_STREAM=0: pf_copy_batch_async on the decode stream instead of the copy stream
    bool dl_prio = false;     // PF_DL_PRIO=1: the copy stream at the device's highest stream priority
    bool debug_plan = false;  // PF_DEBUG_PLAN=1: host planning phase times on stderr
    int64_t nest_seg = 0;     // PF_NEST_SEG=n: nested segment length, forced (0: default, not forced)
    bool nest_seg_set = false;
    bool dbp_par = true;      // PF_DBP_PAR=0: every DELTA_BINARY_PACKED page on k_delta
    bool bloom_first = true;  // PF_BLOOM_FIRST=0: a dictionary-encoded chunk's Bloom filter hashes every value, not the first occurrences
    bool flat_dstr = true;    // PF_FLAT_DSTR=0: k_flat_dstr takes no page (k_flat_all decodes the small-dictionary string pages)
    int fix_shift = 1;        // PF_FIX_BLK=4096|8192|16384: fixed-width flat blocks (log2 of the multiple of 4096)
};

// Numbers the host planner sizes tables by and the kernels index them by
constexpr uint32_t BA_TILE = 8192;         // stream bytes per PLAIN BYTE_ARRAY walk tile (k_ba_*)
// k_ba_tile links values of up to ~124 bytes within a tile; pages of longer values would all take
// the exact fallback walk there, so a batch with a walk whose values average more than BA_SHORT
// bytes keeps the multi-kernel walk
constexpr uint64_t BA_SHORT = 48;
constexpr uint32_t STICKY_DICT = 64u << 10;   // dictionaries above this keep their chunk's flat blocks on one XCD label
constexpr uint32_t SNAP_RB = 128;                 // input bytes per lane region (Snappy index pass)
constexpr uint32_t SNAP_WIN = 64 * SNAP_RB;       // 8 KiB of input per index window
constexpr uint32_t SNAP_WWORDS = SNAP_WIN / 32;   // token-start bitmap words per window
constexpr uint32_t SNAP_BLOCK = 65536;            // Google Snappy block = executor piece

// Result of the Snappy index pass for one 8 KiB input window.
struct SnapWin {
    uint32_t entry;   // chain start the window's bitmap was built from
    uint32_t exit;    // first chain position at/after the window end (or the stream end)
    uint32_t out;     // output bytes of the tokens in the window (on that chain)
    uint32_t flags;
};

// Snappy entry-table record (pos carries a 2-bit flag in its top bits).
struct SnapEnt {
    uint32_t pos;
    uint32_t out;
};

enum : int32_t {
    PG_V2 = 1,            // DATA_PAGE_V2
    PG_COMPRESSED = 2,    // body lives in scratch after k_snappy
    PG_DICT = 4,          // dictionary page
};

// One decompression job (Snappy raw stream -> dst).
struct SnappyJob {
    const uint8_t* src;
    uint8_t* dst;
    uint32_t src_len;
    uint32_t dst_len;
    int32_t page;         // global page index (for error attribution)
    int32_t chunk;
    uint32_t split_base;  // first entry of this job's 64 KiB split table
    uint32_t n_pieces;    // ceil(dst_len / 65536), >= 1
    uint32_t* tokmap;     // bit i = a token starts at input byte i (n_win * 256 words, index pass)
    uint32_t win_base;    // first entry of this job's 8 KiB index windows (SnapWin / lane outs)
    uint32_t n_win;       // ceil(src_len / 8192), >= 1
    // direct pages (k_snappy_head): output bytes [dlo, dst_len) go to ddst + offset (the column's
    // values) instead of dst + offset; bytes below dlo (the v1 level section) still go to dst.
    // dgran: the store width (4, 8 or 16 bytes) ddst's alignment allows (flush chunks sit at 16-byte
    // aligned output offsets). Only the
    // block-parallel executor writes direct; the whole-page redo and the serial kernel write dst.
    uint8_t* ddst;
    uint32_t dlo;
    uint32_t dgran;
    uint32_t dflags;      // bit 0 (diagnostics) = the block-parallel executor rejects the job (PF_DEBUG_FORCE_REDO);
                          // bit 1 = k_snappy_litcopy candidate (dictionary page, or a data page that did not compress)
    uint32_t lit;         // FB_LITCOPY: the page's literal count (their table is in tokmap)
};

// One ZSTD decompression job (pf_zstd.hip): the frames of src -> dst.
struct ZstdJob {
    const uint8_t* src;
    uint8_t* dst;
    uint32_t src_len;
    uint32_t dst_len;     // room at dst; exact = 1: what the frames have to produce (a page's body)
    int32_t page;         // global page index (for error attribution)
    int32_t chunk;
    uint32_t exact;
    uint32_t produced;    // out: bytes written (0 when the job failed)
};
constexpr int ZSTD_GRID = 512;                   // most workgroups of k_zstd: each owns a literal area
constexpr uint32_t ZSTD_LIT_MAX = 128u << 10;    // literals of one block (Block_Maximum_Size)
// Bytes of one workgroup's literal area when the largest job produces max_dst bytes.
PF_HD inline uint32_t zstd_lit_stride(uint32_t max_dst) {
    return ((max_dst < ZSTD_LIT_MAX ? max_dst : ZSTD_LIT_MAX) + 255u) / 256u * 256u + 256u;
}

// One LZ4 decompression job (pf_lz4.hip): the raw block src -> exactly dst_len bytes at dst.
struct Lz4Job {
    const uint8_t* src;
    uint8_t* dst;
    uint32_t src_len;
    uint32_t dst_len;
    int32_t page;         // global page index (for error attribution)
    int32_t chunk;
    uint32_t produced;    // out: bytes written (0 when the job failed)
    uint32_t pad;
};
constexpr int LZ4_GRID = 2048;                   // most workgroups of k_lz4 (they stride over the jobs)

// DONE_PAGE: k_page_null decoded the whole page (with DONE_NULL); k_lvl and k_flat_null skip only
// such pages -- never DONE_NULL itself, which k_flat_null's own finished blocks of the page set.
// DONE_DSTR: k_flat_dstr decoded the page (set together with DONE_FLAT); k_flat_all's blocks of the page return at it.
enum : int32_t { DONE_FIXED = 1, DONE_FLAT = 2, DONE_NULL = 4, DONE_PAGE = 8, DONE_DSTR = 16 };

// DevPage.direct (k_snappy_head): how the page's decompressed body reaches the decoders
enum : int32_t { DIRECT_NONE = 0, DIRECT_VALUES = 1, DIRECT_INPLACE = 2 };

struct DevPage {
    const uint8_t* body;      // v1: [rep][def][values] uncompressed; v2: values section
    const uint8_t* lvl;       // v2: [rep][def] raw levels (never compressed); v1: null
    uint32_t body_len;
    uint32_t rep_len;         // v2 byte lengths
    uint32_t def_len;
    int32_t chunk;
    int32_t flags;
    int32_t encoding;
    int32_t def_enc;
    int32_t rep_enc;
    int32_t num_values;       // level entries
    int32_t done;             // DONE_FIXED | DONE_FLAT: k_flat_fixed / k_flat decoded (or failed) the page; k_decode skips it
    int64_t entry_start;      // first level entry of this page within its chunk (host prefix sum)
    // written by k_count, consumed by k_scan
    int64_t n_slots;
    int64_t n_values;
    int64_t n_rows;
    int64_t n_chars;
    // written by k_scan (or host for flat fixed-width chunks)
    int64_t slot_start;
    int64_t value_start;
    int64_t row_start;
    int64_t char_start;
    // per-page scratch: BYTE_ARRAY value positions (PLAIN) or dictionary ids, then the block chars (block_chars)
    uint32_t* aux;
    int64_t aux_cap;          // entries
    int32_t ba_job;           // PLAIN BYTE_ARRAY data page: its BaJob (k_count fills it), else -1
    int32_t counted;          // 1: k_count_flat counted the page (k_count skips it)
    IdRunTab* runtab;         // dictionary data page of a flat chunk: id run table (k_runs), else null
    LvlHead* lvltab;          // nullable fixed-width page of a flat chunk: definition-level run table (k_lvl), else null
    uint32_t lvl_cap;         // runs the level table can hold
    // DELTA_LENGTH_BYTE_ARRAY / DELTA_BYTE_ARRAY page (k_dlen, pf_delta.hip): the length tables (dx_cpos,
    // dx_len_a, dx_len_b), values in the length streams, first bad value, and where the chars / suffixes
    // start in the values section; else null
    uint64_t* dx;
    int64_t dx_total;
    int64_t dx_bad;
    uint32_t dx_data;
    uint32_t dx_pad;
    // Snappy data pages: the job's fallback flag (FB_*, read after the executor), and what
    // k_snappy_head decided (DIRECT_*): VALUES = a PLAIN fixed-width page with every level present
    // whose values the executor wrote straight into the column (k_flat_fixed then only sets the
    // validity bits, unless the job fell back to the redo / serial path, which writes the body);
    // INPLACE = the stream is one literal: body points at it in the compressed input, no executor.
    const int* jfb;
    int32_t direct;
    int32_t direct_pad;
    // nested data pages split into segments of seg_len entries (k_nest_*, pf_decode.hip), else null:
    // {RleState ck[3][nseg] (rep, def, value stream state at each segment's start), SegRec rec[nseg]}
    uint8_t* seg;
    int32_t nseg;
    int32_t seg_len;
    int32_t seg_ok;           // k_nest_lvl: 1 = the segment kernels decode the page (k_count / k_decode skip it)
    int32_t nwin;             // k_nest_lvl windows per level stream (the page's bytes / NEST_WIN, rounded up)
    struct WinPub* npub;      // [2][nwin]: what each window of the rep / def stream passes to the next (zeroed per batch)
    // large DELTA_BINARY_PACKED INT32 / INT64 pages decoded block-parallel (k_dbp_*, pf_delta.hip): the block
    // tables (dbp_tabs), else null
    uint8_t* dbp;
    struct WinPub* dbp_pub;   // [dbp_nwin] window hand-overs of the block chain (zeroed per batch)
    int32_t dbp_nwin;
    int32_t dbp_ok;           // 1: k_dbp_* decoded the page; 0 / 2 (not taken / failed): k_delta decodes it
    uint32_t dbp_bcap;        // blocks the tables hold
    uint32_t dbp_pad;
};

// k_nest_lvl / k_dbp_pos: a window's hand-over to the next window of its stream -- the position of
// the first run header (block header) at or past the window's end, the entries (blocks) before it,
// whether the chain ended (st = 1) -- packed in one 64-bit word (0 until published) that is stored and
// polled with relaxed agent-scope atomics (round 5: three stores and a release flag made every
// hand-over write back the XCD's L2 and every acquire invalidate the reader's).
// winpub_put / winpub_get: pf_device.h.
struct WinPub {
    uint64_t w;
};
#ifndef PF_NEST_WIN
#define PF_NEST_WIN 2048
#endif
constexpr uint32_t NEST_WIN = PF_NEST_WIN;  // k_nest_lvl window bytes (power of two)
#ifndef PF_DBP_WIN
#define PF_DBP_WIN 4096
#endif
constexpr uint32_t DBP_WIN = PF_DBP_WIN;    // k_dbp_pos window bytes (power of two)
constexpr int32_t DBP_PAR_MIN = 16384;      // DELTA_BINARY_PACKED pages with at least this many entries go block-parallel

// One segment of a nested page: its level counts (k_count_seg), their exclusive prefixes over the
// page (k_nest_scan), the chars of its values and their prefix (k_nest_ids / k_nest_chars).
struct SegRec {
    uint32_t ns, nv, nr, pad;
    uint64_t chars;
    uint32_t sb, vb, rb, pad2;
    uint64_t cb;
};
constexpr uint32_t NEST_CK_BYTES = 40;      // sizeof(RleState) (pf_device.h)
constexpr uint32_t NEST_SEG = 2048;         // default entries per segment
constexpr uint32_t NEST_MAX_SEGS = 1024;    // segments per page (k_nest_scan keeps their targets in LDS)
PF_HD inline uint64_t nest_seg_bytes(int32_t nseg) {
    return uint64_t(nseg) * (3ull * NEST_CK_BYTES + sizeof(SegRec));
}

// One PLAIN BYTE_ARRAY length walk (a BYTE_ARRAY dictionary page, or the values section of a
// PLAIN BYTE_ARRAY data page), done tile-parallel by the k_ba_* kernels (pf_ba.hip).
// BA_RELINK: the fused tile pass (k_ba_tile) rejected the job -- a value longer than its halo, or
// filters it could not separate -- and k_ba_fallback re-links it over the whole job before any walk
enum : int32_t { BA_OK = 0, BA_FALLBACK = 1, BA_SKIP = 2, BA_RELINK = 3 };
struct BaJob {
    const uint8_t* p;         // stream (data pages: set by k_count)
    uint32_t* pos;            // out: chars start of value k
    uint32_t* len;            // out (optional): length of value k
    int64_t* chars_out;       // out (optional): total chars
    uint32_t* cand;           // bitmaps over the stream, n_cap / 32 + 1 words each
    uint32_t* link1;
    uint32_t* link2;
    uint32_t* tile_cnt;       // per tile: accepted positions, then their exclusive scan
    int64_t count;            // values to read (data pages: set by k_count)
    uint32_t n;               // stream bytes (data pages: set by k_count; <= n_cap)
    uint32_t n_cap;           // host bound: tiles and bitmaps are sized for it
    uint32_t n_tiles;
    int32_t chunk, page;
    int32_t state;            // BA_* (data pages: BA_SKIP until k_count fills the job)
};

struct DevChunk {
    int32_t ptype, type_length, width, max_def, max_rep, repeated_def, list_null_def, codec;
    int32_t dict_page;        // global page index of the dictionary page, -1 if none
    int32_t first_page;       // first data page (global index)
    int32_t n_pages;          // data pages
    int32_t needs_count;      // 1: BYTE_ARRAY or nested -> k_count + k_scan
    int64_t num_entries;
    // dictionary (k_dict): fixed width -> dict_data is the decoded PLAIN page;
    // BYTE_ARRAY -> dict_pos[i] = byte offset of entry i's length prefix in dict_data
    const uint8_t* dict_data;
    uint32_t* dict_pos;       // n+1 entries: start of chars of entry i (after the prefix), end at [n] sentinel
    uint32_t* dict_len;
    int64_t dict_n;
    // outputs
    uint8_t* values;
    uint8_t* validity;
    int32_t* offsets;
    uint8_t* chars;
    int32_t* list_offsets;
    uint8_t* list_validity;
    uint8_t* def_levels;
    uint8_t* rep_levels;
    int64_t values_cap, chars_cap, slots_cap, rows_cap;   // capacities (bytes / elements)
};

struct DevChunkResult {
    int64_t num_slots, num_values, num_rows, num_chars;
    int32_t status;           // pf_status (first error wins, atomicMin on negative codes)
    int32_t err_page;
};

// Kept dictionaries (pf_flat_ids.hip, pf_decode_row_group_dict): one DevKeep per chunk that is decoded to indices +
// dictionary. The chunk's DevChunk.values holds its indices (index_width bytes per slot); it has no offsets or chars of
// its own and is on none of the count, scan, flat or decode lists. The dictionary's output arrays lie in the out arena
// (values, or offsets) and, for BYTE_ARRAY, in the chars arena (k_dict_offsets takes the room and writes d_chars /
// num_chars, which come down with the results).
struct DevKeep {
    int32_t chunk;
    int32_t index_width;      // 1, 2 or 4
    int64_t n_entries;
    uint8_t* d_values;        // fixed width: n_entries * width bytes
    int32_t* d_offsets;       // BYTE_ARRAY: n_entries + 1
    uint8_t* d_chars;         // BYTE_ARRAY: device-written (null: the arena was full)
    int64_t num_chars;        // device-written
};
constexpr uint32_t DICT_LONG = 64;           // k_dict_pack: entries longer than this are copied by the whole workgroup

// Row windows (pf_window.hip, pf_decode_row_group_rows): one DevWin per chunk whose window is not {0, -1}, and what
// k_win_bounds finds for it. k_win_copy writes the window's arrays into the twin output arenas (out, bits, chars: the
// decode arenas' sizes and per-chunk offsets), in tiles of WIN_TILE output bytes per array.
constexpr uint32_t WIN_TILE = 4096;
struct DevWin {
    int32_t chunk, pad;
    int64_t skip, take;       // rows from the first row of the first data page; take -1: to the end
};
struct DevWinRes {
    int64_t e0, n_entries;    // the window's first level entry, and how many it has
    int64_t s0, n_slots;
    int64_t c0, n_chars;
    int64_t n_values, n_rows;
    const uint8_t* chars_src; // the chunk's chars (k_scan placed them) and their twin
    uint8_t* chars_dst;
    int32_t status;           // pf_status of the window (the decode's own status when that failed)
    int32_t identity;         // 1: the window keeps every row; nothing was copied, the decode arenas hold the result
};

// Row filters (pf_filter.hip, pf_decode_row_group_filter): the predicates as plan_filter packs them, each chunk's input
// and output arrays as k_sel_prep resolves them on the device (the input lies where the window stage left it; the output
// goes to the arena that does not hold the input), and the stage's head. Tiles are SEL_TILE rows: 16 mask words.
constexpr uint32_t SEL_TILE = 1024;          // rows per workgroup round of the k_sel_* kernels (a multiple of 256)
constexpr uint32_t SEL_LONG = 32;            // BYTE_ARRAY values longer than this are copied by a whole wave
constexpr int32_t PRED_HAS_LO = 1, PRED_HAS_HI = 2;
constexpr int32_t PRED_BOUND_MAX = 4096;     // bytes of a BYTE_ARRAY bound
struct DevPred {
    int32_t chunk, op, ptype, flags;   // op: PF_PRED_*; flags: PRED_HAS_*
    int64_t lo_i, hi_i;                // INT32, INT64, BOOLEAN
    double lo_f, hi_f;                 // FLOAT (widened), DOUBLE
    uint32_t lo_off, lo_len, hi_off, hi_len;   // BYTE_ARRAY: the bounds in the blob behind the table
};
struct DevSelChunk {
    const uint8_t* values;    // input
    const uint8_t* validity;
    const int32_t* offsets;
    const uint8_t* chars;
    uint8_t* o_values;        // output
    uint8_t* o_validity;
    int32_t* o_offsets;
    uint8_t* o_chars;
    int64_t n_rows;           // rows of the input (after its window)
    int64_t n_values, n_chars;   // of the selection (k_sel_fin)
    int32_t width, ptype, max_def;
    int32_t status;           // the chunk's status after the filter
};
struct DevSelHead {
    int64_t rows_in, rows_selected;
    int32_t status;           // a predicate chunk's failure (every chunk takes it), or rows_in out of range
    int32_t pad;
};
// The filter stage's device buffers (one context buffer, sized from the host's row counts: layout_filter, pf_result.h).
// rows_cap bounds rows_in; tiles_cap = the tiles of rows_cap, also the stride of ba_sum / ba_base (one row per chunk).
struct SelBufs {
    DevSelHead* head;
    DevSelChunk* sc;          // [n_chunks]
    const DevPred* preds;     // [n_preds], then the blob of BYTE_ARRAY bounds
    const uint8_t* blob;
    const int32_t* win_of;    // [n_chunks]: the chunk's entry in the window tables, -1 without one
    uint64_t* mask;           // [tiles_cap * SEL_TILE / 64]
    uint32_t* tile_count;     // [tiles_cap] selected rows per tile, and their exclusive scan
    uint32_t* tile_base;
    int32_t* rows;            // [rows_cap] the selected row numbers (16-byte aligned)
    uint32_t* ba_sum;         // [n_chunks * tiles_cap] chars per output tile, and their exclusive scan
    uint32_t* ba_base;
    int64_t* ba_total;        // [n_chunks]
    int64_t rows_cap, tiles_cap;
    int32_t n_preds;
};

// Predicates over kept dictionaries (pf_filter_dict.hip, pf_decode_row_group_dict_filter): a PF_PRED_RANGE on a kept
// chunk is evaluated once per dictionary entry into a match bitmap (k_sel_dict) and looked up per row through the
// chunk's indices (k_sel_mask_dict). One DevSelDict per such predicate, in a table of its own behind the filter
// stage's other tables, so DevPred and SelBufs are what they are for a batch without one.
constexpr uint32_t SELD_TILE = 256;          // dictionary entries per workgroup of k_sel_dict: four bitmap words
struct DevSelDict {
    int32_t pred;             // the predicate's entry in SelBufs.preds
    int32_t keep;             // its chunk's entry in the DevKeep table
    int64_t n_entries;        // the dictionary page's num_values
    uint64_t word_off;        // first word of its bitmap in SelDictBufs.bits
    uint64_t n_words;         // ceil(n_entries / 64)
};
struct SelDictBufs {
    const DevSelDict* recs;   // [n_recs]
    const int32_t* dict_of;   // [n_preds]: the predicate's entry in recs, -1: evaluated row by row
    uint64_t* bits;           // the match bitmaps, back to back
    const DevKeep* keeps;     // the batch's kept-dictionary tables (metadata block)
    const int32_t* keep_of;
    int32_t n_recs;
    int32_t tiles;            // SELD_TILE tiles of the largest dictionary, at least one
};

// GPU page-header scan (pf_scan.hip, pf_scan_pages)
struct ScanChunk {            // device copy of pf_scan_chunk
    const uint8_t* base;      // chunk's first byte
    uint64_t size;
    int64_t num_values;
    int32_t page_base;
    int32_t page_cap;
};

struct ScanCrc {              // per page slot: header crc and the page bytes it covers
    const uint8_t* body;
    uint32_t len;
    uint32_t crc;
    int32_t has_crc;
    int32_t chunk;
};

struct ScanResult {           // mirrors pf_scan_result
    int32_t n_pages;
    int32_t status;
    int32_t err_page;
    int32_t crc_pages;
};

}  // namespace pf
