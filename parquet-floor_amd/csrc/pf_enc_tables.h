// pf_enc_tables.h — the write path's tables as plain data: what the host planner (pf_enc_plan.cpp) fills,
// the runtime (pf_enc_runtime.hip) uploads and the kernels (pf_encode.hip, pf_enc_*.hip) read. No HIP type
// and no HIP header, so a plain C++ compiler takes it; the launchers are declared in pf_encode.h. Internal.
#pragma once
#include <cstdint>

namespace pf {

// Compression job: 8 KiB of input, compressed independently (copies never leave the job), so a
// 64 KiB Snappy block is eight jobs: 8x the waves of one wave per block (the kernel is latency-bound
// per job), for ~3 % larger output; tokens still never cross the 64 KiB output boundaries the read
// path's piece executor splits at. 64 KiB -> 16 KiB -> 8 KiB jobs: 33 -> 10 -> 6.6 ms per SF1 row group.
constexpr uint32_t SC_BLOCK = 8192;
// worst case of one compressed job (literal headers of <= 3 bytes per run): Google's bound
constexpr uint32_t SC_SLOT = ((32u + SC_BLOCK + SC_BLOCK / 6u) + 255u) & ~255u;

// ZSTD (pf_zstd_enc.hip): the same job geometry, one job = one block of the section's frame, written whole
// (3-byte header included) into its slot, so a job never takes more than 3 + its length (a block that does
// not shrink is stored raw). 8 KiB as for Snappy; larger blocks are not measured yet.
constexpr uint32_t ZC_BLOCK = 8192;
constexpr uint32_t ZC_SLOT = ((3u + ZC_BLOCK) + 255u) & ~255u;

struct CompJob {
    const uint8_t* src;
    uint8_t* dst;      // SC_SLOT / ZC_SLOT bytes
    uint32_t len;      // <= SC_BLOCK / ZC_BLOCK
    uint32_t last;     // ZSTD: the job ends its section (Last_Block); Snappy: 0
};
using SnapCJob = CompJob;
using ZstdCJob = CompJob;

struct EncPage {
    uint64_t out_off;  // values section in vals_out
    uint32_t d0, cnt;  // dense values [d0, d0 + cnt)
    uint32_t dict, bw;
};

// Every device array of one chunk's encode (one arena, laid out by the host).
struct EncArgs {
    int32_t ptype, width;
    int64_t n;                       // rows
    const uint8_t* values;           // row-indexed input
    const uint8_t* validity;         // nullptr: all present
    const int32_t* offsets;
    const uint8_t* chars;
    uint32_t* flag;                  // n + 1
    uint32_t* pos;                   // n + 1 (exclusive scan of flag)
    uint8_t* dense;                  // m x width (fixed, BOOLEAN)
    uint32_t* dsrc;                  // strings: chars offset of dense value
    uint32_t* dlen;                  // strings: length
    uint32_t* vsz;                   // strings: 4 + length (m + 1)
    uint32_t* vpre;                  // strings: exclusive scan of vsz (m + 1)
    uint64_t* key;                   // m
    uint64_t* skey;                  // m (sorted)
    uint32_t* didx;                  // m (0..m-1)
    uint32_t* sidx;                  // m (sorted)
    uint32_t* headpos;               // m
    uint32_t* head;                  // m
    uint32_t* mark;                  // m + 1
    uint32_t* did;                   // m + 1
    uint32_t* dsz;                   // m + 1
    uint32_t* doff;                  // m + 1
    uint32_t* ids;                   // m
    uint32_t* collide;               // 1
    uint8_t* dict_out;               // dictionary page (PLAIN)
    uint8_t* vals_out;               // data pages' values sections
};

// ---- DELTA_BINARY_PACKED / DELTA_BYTE_ARRAY pages (pf_enc_delta.hip) ----
// One DELTA_BINARY_PACKED stream: `cnt` elements of `ew` bytes (4 | 8, signed) at `src`. Its items in
// the size table are item0 (the stream header) and one per 128-delta block after it.
struct DeltaStream {
    const uint8_t* src;
    uint32_t ew, cnt, page, item0;
};

// A data page: streams [s0, s0 + ns) back to back (integers: 1; strings: prefix lengths, suffix
// lengths, followed by the suffix bytes) over dense values [d0, d0 + cnt).
struct DeltaPage {
    uint64_t out_off;   // values section in `out` (known after the size pass)
    uint32_t d0, cnt, s0, ns;
};

struct DeltaArgs {
    const DeltaStream* streams;      // n_streams + 1 (the last: item0 = n_items)
    const DeltaPage* pages;          // n_pages
    uint32_t n_streams, n_pages, n_items;
    uint32_t* bytes;                 // n_items + 1: bytes of every item
    uint32_t* off;                   // n_items + 1 (exclusive scan of bytes)
    long long* minv;                 // n_items: min delta of a block
    uint32_t* widths;                // n_items: the 4 miniblock widths, one byte each
    uint32_t* totals;                // n_pages: bytes of a page's values section
    uint32_t* pfx;                   // strings, m + 1: prefix length
    uint32_t* sfx;                   // strings, m + 1: suffix length
    uint32_t* spre;                  // strings, m + 1 (exclusive scan of sfx); nullptr for integers
    uint8_t* out;                    // data pages' values sections
};

// ---- RLE / bit-packed hybrid streams in parquet-mr's run shape (pf_enc_hybrid.hip) ----
enum { HY_VALIDITY = 0, HY_IDS = 1, HY_BOOL = 2 };                 // HybridStream.kind
enum { HY_PREFIX_NONE = 0, HY_PREFIX_WIDTH = 1, HY_PREFIX_LENGTH = 2 };   // bytes in front of out_off

// One stream: `cnt` entries from entry `first` of `src` at bit width `bw`: the validity bits of a page's
// rows (nullptr: all set), the uint32 dictionary ids or the dense BOOLEAN bytes of its present values.
struct HybridStream {
    const uint8_t* src;
    uint64_t out_off;   // first byte of the stream in `out` (known after the size pass)
    uint32_t kind, first, cnt, bw, prefix, page;
};

struct HybridArgs {
    const HybridStream* streams;     // n_streams
    uint32_t n_streams;
    uint32_t* bytes;                 // n_streams: bytes of every stream (size pass)
    uint8_t* out;
};

// ---- page and chunk statistics (pf_enc_stats.hip; PF_ENCODE_STATISTICS) ----
constexpr uint32_t ST_TILE = 4096;    // dense values of one workgroup
constexpr uint32_t ST_LIMIT = 4096;   // len(min) + len(max) at or above it: no Statistics struct

struct StatTile {
    uint32_t page, d0, cnt, pad;      // dense values [d0, d0 + cnt) of data page `page`
};

// A tile's partial, a page's result and the chunk's. Partials hold keys; results hold the PLAIN bits of a
// fixed-width min / max, or for strings the winners' dense indices and lengths.
struct StatPart {
    uint64_t mn, mx;
    uint32_t mnl, mxl;                // strings: min(len, 8) beside a key, the full length in a result
    uint32_t mni, mxi;                // strings: dense index of the winner
    uint32_t any, pad;                // 0: no value (FLOAT / DOUBLE: none that is not NaN); 1: min / max; 2: over ST_LIMIT
};

struct StatArgs {
    const StatTile* tiles;           // n_tiles, in page order
    const uint32_t* ptile;           // n_pages + 1: page p owns tiles [ptile[p], ptile[p + 1])
    uint32_t n_tiles, n_pages;
    StatPart* part;                  // n_tiles
    uint32_t* win;                   // strings, 2 x n_tiles: a tile's winners among the values with the page's extreme keys
    StatPart* out;                   // n_pages + 1: the pages, then the chunk
    uint8_t* bytes;                  // strings, (n_pages + 1) x ST_LIMIT: min ‖ max of every entry with any == 1
};

// ---- page index (pf_enc_pgindex.hip; PF_ENCODE_PAGE_INDEX) ----
constexpr uint32_t PX_NO_TRUNC = 0xffffffffu;   // PgIndexArgs::trunc: BYTE_ARRAY values are written whole

// The ColumnIndex lists of one chunk, from the page results k_enc_stats_combine left in StatArgs::out. The
// outputs are one block of the arena (the host copies it back in one piece): head, null_counts, off, null_pages, values.
struct PgIndexHead {
    uint32_t valid;                  // 1: a ColumnIndex can be written
    uint32_t order;                  // 0 UNORDERED, 1 ASCENDING, 2 DESCENDING
    uint32_t value_bytes;            // = off[2 * n_pages]
    uint32_t non_null;               // pages with a present value
};
struct PgIndexArgs {
    const StatPart* pages;           // n_pages page results
    const uint32_t* rows;            // n_pages: rows of a page
    const uint32_t* cnt;             // n_pages: its present values
    uint32_t n_pages, trunc;         // trunc: longest BYTE_ARRAY entry, or PX_NO_TRUNC
    uint32_t value_cap;              // bytes at `values`
    uint32_t* nn;                    // n_pages scratch: the pages that are not null pages, in order
    PgIndexHead* head;
    long long* null_counts;          // n_pages
    uint32_t* off;                   // 2 * n_pages + 1
    uint8_t* null_pages;             // n_pages
    uint8_t* values;                 // value_cap
};

// ---- page CRCs (pf_enc_crc.hip; PF_ENCODE_PAGE_CRC) ----
struct CrcPiece {
    const uint8_t* ptr;
    const uint32_t* len_ptr;         // the length in device memory (a compression job's), or nullptr: `len`
    uint32_t len, cap;               // cap: bytes readable at ptr
};
struct CrcOut {
    uint32_t raw, len, x8len, pad;   // raw CRC (zero init, no final xor), bytes, x^(8 len) mod P
};

}  // namespace pf
