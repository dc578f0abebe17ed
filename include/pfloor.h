/*
 * pfloor.h — C ABI of the MI355X-native Parquet column-chunk decoder.
 *
 * This is the drop-in boundary beneath parquet-floor's
 *   ParquetReader.streamContent(File|InputFile, HydratorSupplier[, columns])
 *   (reference: src/main/java/blue/strategic/parquet/ParquetReader.java:47-61)
 * Today that call pulls every value through parquet-mr 1.12.2's ColumnReader
 * (ParquetReader.java:141-168, :176-212) and decompresses pages through the
 * Hadoop codec shim into snappy-java (src/main/java/org/apache/hadoop/io/compress/
 * DecompressorStream.java:61-70,101-173; ReflectionUtils.java:10-21; CodecPool.java:6-8).
 *
 * The Java side keeps footer / schema / page-header (Thrift) parsing and fills the
 * POD descriptors below; chunk bytes are handed over in one buffer (pinned host memory
 * from pf_host_alloc, or device memory already resident in HBM).  The library decodes
 * every page on the GPU and returns columnar buffers (values, validity, BYTE_ARRAY
 * offsets + chars, list offsets, raw levels) that the Java adapter walks in
 * ParquetReader.tryAdvance order to call Hydrator.add(record, path[0], value).
 *
 * Rules of the ABI: plain C, no C++/torch types, every function returns a pf_status
 * (0 = OK, negative = error) except pf_abi_version / pf_last_error. No callbacks into
 * the caller. One context per GPU; one host thread drives a context at a time.
 * Error text for the last failing call on a context (or, for ctx-less calls, the
 * calling thread) is returned by pf_last_error.
 */
#ifndef PFLOOR_H
#define PFLOOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_ABI_VERSION 1

/* ---- status codes (mapped by the Java bridge onto the reference's exceptions:
 *      IOException for open/footer errors, RuntimeException("Failed to read parquet", cause)
 *      for iteration errors — ParquetReader.java:120, :209-211) ---------------------- */
typedef enum pf_status {
    PF_OK = 0,
    PF_ERR_INVALID_ARG = -1,
    PF_ERR_CORRUPT_PAGE = -2,         /* bounds / varint / RLE overrun; never an OOB read */
    PF_ERR_UNSUPPORTED_ENCODING = -3,
    PF_ERR_UNSUPPORTED_CODEC = -4,
    PF_ERR_HIP = -5,
    PF_ERR_CAPACITY = -6,             /* caller buffer too small; required sizes are reported */
    PF_ERR_UNSUPPORTED_TYPE = -7,     /* ParquetReader.java:162-163 "Unsupported type" */
    PF_ERR_IO = -8,
    PF_ERR_STATE = -9
} pf_status;

/* ---- Parquet enums (Thrift ids of parquet-format; values are the wire values) ---- */
typedef enum pf_physical_type {
    PF_BOOLEAN = 0, PF_INT32 = 1, PF_INT64 = 2, PF_INT96 = 3,
    PF_FLOAT = 4, PF_DOUBLE = 5, PF_BYTE_ARRAY = 6, PF_FIXED_LEN_BYTE_ARRAY = 7
} pf_physical_type;

typedef enum pf_codec {
    PF_CODEC_UNCOMPRESSED = 0, PF_CODEC_SNAPPY = 1, PF_CODEC_GZIP = 2, PF_CODEC_LZO = 3,
    PF_CODEC_BROTLI = 4, PF_CODEC_LZ4 = 5, PF_CODEC_ZSTD = 6, PF_CODEC_LZ4_RAW = 7
} pf_codec;

typedef enum pf_page_type {
    PF_PAGE_DATA = 0, PF_PAGE_INDEX = 1, PF_PAGE_DICTIONARY = 2, PF_PAGE_DATA_V2 = 3
} pf_page_type;

typedef enum pf_encoding {
    PF_ENC_PLAIN = 0, PF_ENC_PLAIN_DICTIONARY = 2, PF_ENC_RLE = 3, PF_ENC_BIT_PACKED = 4,
    PF_ENC_DELTA_BINARY_PACKED = 5, PF_ENC_DELTA_LENGTH_BYTE_ARRAY = 6,
    PF_ENC_DELTA_BYTE_ARRAY = 7, PF_ENC_RLE_DICTIONARY = 8, PF_ENC_BYTE_STREAM_SPLIT = 9
} pf_encoding;

/* ---- descriptors filled from the Java Thrift parse (PageHeader / ColumnMetaData) ---- */

/* One page of a column chunk. `offset` locates the page BODY (the bytes after the
 * Thrift PageHeader) relative to the chunk's first byte. */
typedef struct pf_page_desc {
    uint64_t offset;
    uint32_t compressed_size;     /* PageHeader.compressed_page_size   (field 3) */
    uint32_t uncompressed_size;   /* PageHeader.uncompressed_page_size (field 2) */
    int32_t  page_type;           /* pf_page_type                       (field 1) */
    int32_t  encoding;            /* values encoding (DataPageHeader[V2] / DictionaryPageHeader) */
    int32_t  def_encoding;        /* v1 only: RLE or BIT_PACKED */
    int32_t  rep_encoding;        /* v1 only */
    int32_t  num_values;          /* level entries (data) / dictionary entries (dict) */
    int32_t  num_nulls;           /* v2: header; v1: page statistics null_count, -1 if absent.
                                     A routing hint (0 skips the null-page tables); results never
                                     depend on it */
    int32_t  num_rows;            /* v2 only */
    int32_t  def_bytes;           /* v2 only: definition_levels_byte_length */
    int32_t  rep_bytes;           /* v2 only: repetition_levels_byte_length */
    int32_t  is_compressed;       /* v2 only (Thrift default true); v1 pages: 1 */
} pf_page_desc;

/* One column chunk (one leaf column of one row group). */
typedef struct pf_chunk_desc {
    int32_t  physical_type;       /* pf_physical_type */
    int32_t  type_length;         /* FIXED_LEN_BYTE_ARRAY width; ignored otherwise */
    int32_t  max_def;             /* ColumnDescriptor.getMaxDefinitionLevel() */
    int32_t  max_rep;             /* ColumnDescriptor.getMaxRepetitionLevel() (<= 1 supported for list offsets) */
    int32_t  repeated_def;        /* def level of the innermost REPEATED ancestor (0 if max_rep == 0):
                                     an entry is a list element ("slot") iff def >= repeated_def */
    int32_t  list_null_def;       /* the innermost list is non-null iff def >= list_null_def */
    int32_t  codec;               /* pf_codec: UNCOMPRESSED, SNAPPY, ZSTD or LZ4_RAW (others: PF_ERR_UNSUPPORTED_CODEC) */
    int32_t  n_pages;             /* pages, including the dictionary page if present */
    const pf_page_desc* pages;
    uint64_t chunk_offset;        /* offset of the chunk's first byte in the bytes buffer */
    uint64_t chunk_size;          /* ColumnMetaData.total_compressed_size */
    int64_t  num_rows;            /* RowGroup.num_rows (flat columns: = level entries) */
} pf_chunk_desc;

/* Decoded layout of one column chunk ("slots" = rows for flat columns, list elements for
 * max_rep == 1; null slots hold zero bytes / zero-length strings):
 *   values        slots * width bytes (BOOLEAN: 1 byte 0/1; INT96: 12; FLBA: type_length)
 *   validity      ceil(slots/8) bytes, LSB-first, bit = (def == max_def)     [max_def > 0]
 *   offsets       (slots+1) int32, BYTE_ARRAY only; chars = concatenated bytes
 *   list_offsets  (rows+1) int32, max_rep == 1: slots before each row
 *   list_validity ceil(rows/8) bytes, bit = (def of the row's first entry >= list_null_def)
 *   def_levels / rep_levels  one byte per level entry                          [max_rep > 0]
 * Capacities are in BYTES. Any pointer may be NULL to skip that array. */
typedef struct pf_column_out {
    void*    values;        size_t values_cap;
    uint8_t* validity;      size_t validity_cap;
    int32_t* offsets;       size_t offsets_cap;
    uint8_t* chars;         size_t chars_cap;
    int32_t* list_offsets;  size_t list_offsets_cap;
    uint8_t* list_validity; size_t list_validity_cap;
    uint8_t* def_levels;    size_t def_levels_cap;
    uint8_t* rep_levels;    size_t rep_levels_cap;
} pf_column_out;

/* Sizes (and device pointers) of one decoded chunk, valid after pf_wait. */
typedef struct pf_column_info {
    int64_t num_entries;          /* level entries (= Σ page num_values) */
    int64_t num_slots;
    int64_t num_values;           /* non-null leaf values (def == max_def) */
    int64_t num_rows;             /* entries with rep == 0 */
    int64_t num_chars;            /* BYTE_ARRAY bytes */
    int32_t width;                /* bytes per slot in `values` (0 for BYTE_ARRAY) */
    int32_t status;               /* per-chunk pf_status */
    const void*    d_values;      /* device pointers (owned by the context, valid until the next decode) */
    const uint8_t* d_validity;
    const int32_t* d_offsets;
    const uint8_t* d_chars;
    const int32_t* d_list_offsets;
    const uint8_t* d_list_validity;
    const uint8_t* d_def_levels;
    const uint8_t* d_rep_levels;
} pf_column_info;

typedef struct pf_ctx pf_ctx;

int         pf_abi_version(void);
const char* pf_last_error(pf_ctx* ctx);           /* ctx may be NULL: thread-local message */

int pf_device_count(int* count);
int pf_ctx_create(int device, pf_ctx** out);
int pf_ctx_destroy(pf_ctx* ctx);
/* A second context on peer's GPU that enqueues onto peer's HIP stream (own device buffers,
 * results and completion event). Two such contexts let a reader plan and enqueue row group
 * i+1 while row group i is still decoding (the same stream keeps them in order), and pf_wait
 * on one waits only for its own decode. The shared stream lives until both are destroyed. */
int pf_ctx_create_shared(pf_ctx* peer, pf_ctx** out);
/* Per-stage timing events (pf_last_timing); on by default. Each event is a marker on the
 * stream between kernels, so a throughput-critical caller turns them off. */
int pf_ctx_set_timing(pf_ctx* ctx, int on);

/* Pinned host memory (hipHostMalloc) for chunk bytes and outputs; Java wraps it with
 * MemorySegment.reinterpret. */
int pf_host_alloc(pf_ctx* ctx, size_t bytes, void** out);
int pf_host_free(pf_ctx* ctx, void* ptr);

/* Device memory owned by the context (for callers that keep inputs resident in HBM). */
int pf_device_alloc(pf_ctx* ctx, size_t bytes, void** out);
int pf_device_free(pf_ctx* ctx, void* ptr);
int pf_memcpy_h2d(pf_ctx* ctx, void* dst, const void* src, size_t bytes);   /* async on ctx stream */

/* Enqueue the decode of n_chunks column chunks whose bytes live in `bytes`
 * (n_bytes long; host memory, ideally pinned, unless bytes_on_device != 0).
 * Asynchronous: returns after enqueueing H2D + kernels on the context's stream.
 * Descriptor arrays are copied before return. Results live in context-owned device
 * buffers until the next pf_decode_row_group on this context. */
int pf_decode_row_group(pf_ctx* ctx, const pf_chunk_desc* chunks, int n_chunks,
                        const uint8_t* bytes, size_t n_bytes, int bytes_on_device);

/* Windowed decode: chunk i's results are cut to rows [skip_rows, skip_rows + take_rows) of the pages listed (rows
 * counted from the first row of its first data page; take_rows -1: to the end), on the GPU, before anything crosses the
 * link. windows == NULL is pf_decode_row_group, call for call; otherwise one window per chunk. A negative skip_rows or
 * a take_rows < -1 is PF_ERR_INVALID_ARG and nothing is enqueued. After pf_wait, pf_column_info_get, pf_copy_column and
 * pf_copy_columns_async describe each chunk as if it had held only the window's rows, under the layout rules above:
 * num_rows = take, num_entries / num_slots / num_values / num_chars those of the window, values from the window's first
 * slot, validity and list_validity from bit 0 with the unused high bits of the last byte zero, offsets[0] = 0 and
 * list_offsets[0] = 0, chars / def_levels / rep_levels only the window's (take 0: empty arrays, offsets = {0},
 * list_offsets = {0}). Per-chunk status after pf_wait (the other chunks are unaffected): PF_ERR_INVALID_ARG when the
 * window reaches past the rows the pages hold (for v1 and nested pages only the device knows that count);
 * PF_ERR_CORRUPT_PAGE when the first entry of a max_rep = 1 chunk has a repetition level other than 0 (pages of an
 * indexed chunk start at row boundaries); PF_ERR_UNSUPPORTED_TYPE for max_rep > 1 unless the window keeps every row.
 * A window {0, -1} is the identity and costs nothing; any other window runs the window kernels (k_win_bounds,
 * k_win_copy: pf_window.hip), which write into twin output arenas (a window that turns out to keep every row is left
 * in place). The twins have the capacity of the decode arenas (the chars arena is at least 16 MiB) and stay allocated
 * until pf_ctx_destroy, so a context that has decoded with windows once holds twice the output memory. After a decode in which any chunk had a window other than {0, -1}, pf_batch_bytes, pf_copy_batch_async
 * and pf_column_info_host return PF_ERR_STATE: the arenas hold more than the windows, and compacting them into one
 * batch layout is not done. */
typedef struct pf_row_window { int64_t skip_rows; int64_t take_rows; } pf_row_window;   /* take_rows -1: to the end */
int pf_decode_row_group_rows(pf_ctx* ctx, const pf_chunk_desc* chunks, int n_chunks, const pf_row_window* windows,
                             const uint8_t* bytes, size_t n_bytes, int bytes_on_device);

/* Filtered decode: a conjunction of simple predicates is evaluated on the GPU over the decoded (and windowed) columns,
 * and every chunk of the batch is compacted to the matching rows on the device, so only those rows cross the link.
 * n_preds == 0 is pf_decode_row_group_rows, call for call (no stage, no allocation, batch copies allowed). Otherwise the
 * row mask is the AND of all predicates, and after pf_wait, pf_column_info_get, pf_copy_column and pf_copy_columns_async
 * describe every chunk as if it had held only the selected rows, in file order, under the layout rules above:
 * num_rows = num_entries = num_slots = rows_selected, num_values and num_chars those of the selection, validity from
 * bit 0 with the unused high bits of the last byte zero, offsets[0] = 0 and only the selected chars, null slots zero
 * (zero-length for BYTE_ARRAY); rows_selected == 0: empty arrays and offsets = {0}.
 * A bound is the PLAIN bytes of a value, as Statistics and the ColumnIndex hold them: 4 or 8 little-endian bytes for
 * INT32 / FLOAT and INT64 / DOUBLE, 1 byte (0 or 1) for BOOLEAN, the raw bytes (at most 4096) for BYTE_ARRAY; a NULL
 * bound is unbounded. INT32, INT64 and BOOLEAN compare as signed integers; FLOAT and DOUBLE by IEEE lo <= v && v <= hi
 * (a NaN value or bound matches nothing, -0.0 equals +0.0); BYTE_ARRAY unsigned bytewise, a proper prefix first. A null
 * row matches only PF_PRED_IS_NULL; a REQUIRED column has no nulls. Unsigned and decimal logical orders are out of
 * scope: a UINT_* or DECIMAL column is compared by the rules of its physical type.
 * Call errors (nothing is enqueued): PF_ERR_INVALID_ARG for n_preds outside [0, PF_MAX_PREDICATES], NULL preds with
 * n_preds > 0, a chunk index out of range, an unknown op, a bound whose length is not the type's width (over 4096 for
 * BYTE_ARRAY; a BOOLEAN bound other than 0 or 1), a non-NULL bound on IS_NULL / NOT_NULL; PF_ERR_UNSUPPORTED_TYPE for
 * a predicate on a chunk with max_rep > 0, and for PF_PRED_RANGE on INT96 or FIXED_LEN_BYTE_ARRAY (IS_NULL and NOT_NULL
 * take any flat type).
 * Per-chunk status after pf_wait: a predicate chunk that failed to decode or to window gives its status to every chunk
 * of the batch and to pf_selection_info.status; rows_in is the row count of the first predicate's chunk after its
 * window, and a chunk whose own count differs gets PF_ERR_INVALID_ARG (a predicate chunk: every chunk does); rows_in
 * above INT32_MAX is PF_ERR_INVALID_ARG; a payload chunk with max_rep > 0 gets PF_ERR_UNSUPPORTED_TYPE; a payload
 * chunk's own failure stays its own.
 * The filter kernels (k_sel_*: pf_filter.hip) write each chunk into the arena that does not hold its input: the twin
 * arenas of the window stage (allocated for any filtered batch), or back into the decode arenas for a chunk the window
 * stage moved. After a filtered decode pf_batch_bytes, pf_copy_batch_async and pf_column_info_host return PF_ERR_STATE,
 * as after a windowed one. */
#define PF_MAX_PREDICATES 8
#define PF_PRED_RANGE    0   /* present and lo <= v <= hi; a NULL bound is unbounded; both NULL: every present row */
#define PF_PRED_IS_NULL  1
#define PF_PRED_NOT_NULL 2
typedef struct pf_predicate {
    int32_t chunk;            /* index into the batch's chunks: the column the predicate reads */
    int32_t op;               /* PF_PRED_* */
    const uint8_t* lo; int32_t lo_len;   /* PLAIN bytes of the bound, as Statistics / ColumnIndex hold them */
    const uint8_t* hi; int32_t hi_len;
} pf_predicate;
int pf_decode_row_group_filter(pf_ctx* ctx, const pf_chunk_desc* chunks, int n_chunks, const pf_row_window* windows,
                               const pf_predicate* preds, int n_preds, const uint8_t* bytes, size_t n_bytes,
                               int bytes_on_device);
typedef struct pf_selection_info {
    int64_t rows_in;          /* rows the predicates were evaluated over (after the windows) */
    int64_t rows_selected;
    const int32_t* d_rows;    /* ascending row numbers, counted from the window's first row; device, ctx-owned */
    int32_t status;
} pf_selection_info;
/* After pf_wait of a filtered decode (PF_ERR_STATE otherwise). */
int pf_selection_info_get(pf_ctx* ctx, pf_selection_info* out);
/* The selected row numbers into a host buffer, synchronous; PF_ERR_CAPACITY (nothing copied) below 4 * rows_selected. */
int pf_copy_selection(pf_ctx* ctx, int32_t* rows, size_t cap_bytes);

/* Dictionary-preserving decode: keep[i] != 0 asks for chunk i as indices + dictionary instead of expanded values.
 * keep == NULL is pf_decode_row_group, call for call.
 * Eligibility is decided by the planner from the descriptors alone, never from page bytes. A chunk is kept when
 * keep[i] != 0, max_rep == 0, physical_type != PF_BOOLEAN, it has a dictionary page and at least one data page, and
 * every data page's encoding is PF_ENC_RLE_DICTIONARY or PF_ENC_PLAIN_DICTIONARY. Any other chunk (a writer that
 * fell back to PLAIN part-way, a nested chunk, DELTA or PLAIN pages, ...) gets kept = 0 and is decoded as
 * pf_decode_row_group decodes it, byte for byte; asking for it is never an error.
 * index_width is the smallest of 1, 2 or 4 bytes that holds n_entries - 1 (n_entries <= 256: 1, <= 65536: 2, else 4):
 * it follows the dictionary's size, not the id bit width the pages happen to use.
 * A kept chunk after pf_wait: pf_column_info.width = index_width, d_values = num_slots indices (unsigned
 * little-endian; a null slot holds 0), validity, num_entries, num_slots, num_values and num_rows exactly those of the
 * expanding decode, d_offsets = d_chars = NULL and num_chars = 0. pf_copy_column copies values and validity and leaves
 * non-NULL offsets / chars buffers untouched. The dictionary is described by pf_dict_info: its entries in file order
 * (unused ones included), fixed width as n_entries * width bytes, BYTE_ARRAY as n_entries + 1 offsets and the chars.
 * The invariant: values[s] = dict[index[s]] where the validity bit is set, zero bytes or a zero-length string where it
 * is not (BYTE_ARRAY offsets and chars rebuilt in slot order) is bit for bit what pf_decode_row_group gives.
 * Errors: an id >= n_entries in a present value (in a bit-packed run or as an RLE run's value) gives the chunk the
 * status and error page the expanding decode gives it, other chunks are unaffected; a damaged dictionary page is
 * reported as ever. An all-null chunk with an empty dictionary is valid: index_width 1, indices 0.
 * Indices and dictionary arrays live in the batch's out and chars arenas, so pf_batch_bytes, pf_copy_batch_async and
 * pf_column_info_host work after such a decode (the batch is that much smaller); pf_dict_info_host rebases as
 * pf_column_info_host does. The dictionary chars count towards the chars arena's need (an overflow reruns the batch).
 * pf_decode_row_group_rows and _filter take no keep flags: pf_decode_row_group_dict_filter (below) windows and filters
 * kept chunks. */
int pf_decode_row_group_dict(pf_ctx* ctx, const pf_chunk_desc* chunks, int n_chunks, const uint8_t* keep,
                             const uint8_t* bytes, size_t n_bytes, int bytes_on_device);
typedef struct pf_dict_info {
    int32_t kept;          /* 1: the chunk's `values` are indices into the dictionary below; 0: decoded as always */
    int32_t index_width;   /* 1, 2 or 4 bytes, unsigned little-endian; 0 when kept == 0 */
    int64_t n_entries;     /* DictionaryPageHeader.num_values, in file order, unused entries included */
    int32_t width;         /* bytes per entry (INT96 12, FLBA type_length); 0 for BYTE_ARRAY */
    int32_t pad;
    int64_t num_chars;     /* BYTE_ARRAY: bytes of all entries */
    const void*    d_values;   /* n_entries * width */
    const int32_t* d_offsets;  /* n_entries + 1, offsets[0] = 0 */
    const uint8_t* d_chars;
} pf_dict_info;
/* After pf_wait: chunk i's dictionary (all zero with kept = 0 for a chunk that was not kept, also after a decode
 * without keep flags). */
int pf_dict_info_get(pf_ctx* ctx, int chunk, pf_dict_info* out);
/* After pf_copy_batch_async + pf_sync: the same with the pointers rebased into the host copy. */
int pf_dict_info_host(pf_ctx* ctx, int chunk, const void* host, pf_dict_info* out);
/* Windows and predicates over kept dictionaries: pf_decode_row_group_filter with the keep flags of
 * pf_decode_row_group_dict. keep == NULL is pf_decode_row_group_filter, call for call; windows == NULL and n_preds == 0
 * is pf_decode_row_group_dict, batch copies included. The call errors are those of pf_decode_row_group_filter.
 * Eligibility, index_width and pf_dict_info are those of pf_decode_row_group_dict. A chunk that is asked for and not
 * eligible is decoded, windowed and filtered expanded, exactly as pf_decode_row_group_filter does it; never an error.
 * A kept chunk goes through both stages as a fixed-width column of index_width bytes with a validity bitmap:
 *   window   pf_column_info describes the window's slots: width = index_width, d_values = the window's indices (0 in a
 *            null slot), validity from bit 0 with the tail bits of the last byte zero, d_offsets = d_chars = NULL,
 *            num_chars = 0. The window's statuses are those of pf_decode_row_group_rows.
 *   filter   a PF_PRED_RANGE on a kept chunk is evaluated once per dictionary entry and looked up per row through the
 *            indices; the row mask is bit for bit the mask the predicate gives on the expanded chunk (a null row matches
 *            only IS_NULL, a NaN entry matches no bound, -0.0 equals +0.0, bytes compare unsigned with a proper prefix
 *            first). IS_NULL / NOT_NULL read the validity only and stay legal on kept INT96 and FIXED_LEN_BYTE_ARRAY
 *            chunks; PF_PRED_RANGE on those stays PF_ERR_UNSUPPORTED_TYPE. Indices and validity of every kept chunk
 *            are compacted through the row numbers: num_rows = num_entries = num_slots = rows_selected, num_values =
 *            the set validity bits, num_chars = 0.
 * The dictionary is never windowed, compacted or moved: pf_dict_info_get and pf_copy_dictionary give what they give
 * after pf_decode_row_group_dict on the same chunks, every entry in file order, entries no surviving row uses included.
 * The invariant: a kept chunk's result expanded on the host (values[s] = dict[index[s]] as above) is bit for bit what
 * pf_decode_row_group_filter returns for that chunk with the same windows and predicates; pf_selection_info and
 * pf_copy_selection are identical in both.
 * Errors: an id >= n_entries in a present value gives the chunk the status and error page of the expanding decode; if
 * the chunk carries a predicate every chunk takes the status (the rule of pf_decode_row_group_filter). An all-null
 * chunk over an empty dictionary is valid: every RANGE matches nothing, IS_NULL matches every row.
 * After a decode with a window that is not {0, -1} or any predicate, pf_batch_bytes, pf_copy_batch_async,
 * pf_column_info_host and pf_dict_info_host return PF_ERR_STATE; use pf_copy_column(s_async) and pf_copy_dictionary. */
int pf_decode_row_group_dict_filter(pf_ctx* ctx, const pf_chunk_desc* chunks, int n_chunks, const uint8_t* keep,
                                    const pf_row_window* windows, const pf_predicate* preds, int n_preds,
                                    const uint8_t* bytes, size_t n_bytes, int bytes_on_device);
/* The dictionary of a kept chunk into out->values (fixed width) or out->offsets / out->chars (BYTE_ARRAY); the other
 * fields of `out` are ignored. Host buffers, synchronous. PF_ERR_CAPACITY (nothing copied) if a non-NULL buffer is too
 * small; PF_ERR_STATE on a chunk with kept == 0; the chunk's own status if it failed to decode. */
int pf_copy_dictionary(pf_ctx* ctx, int chunk, const pf_column_out* out);

/* Block until the enqueued decode has finished; returns the first per-chunk error. */
int pf_wait(pf_ctx* ctx);

/* Sizes + device pointers of chunk i of the last decode (after pf_wait). */
int pf_column_info_get(pf_ctx* ctx, int chunk, pf_column_info* out);

/* Copy chunk i's decoded arrays into caller buffers (host, synchronous: returns when these
 * copies are done, without waiting for a peer context's work queued behind them).
 * Fails with PF_ERR_CAPACITY (nothing copied) if any non-NULL buffer is too small. */
int pf_copy_column(pf_ctx* ctx, int chunk, const pf_column_out* out);

/* Batched, asynchronous form of pf_copy_column for the end-to-end pipeline (the Java side reads
 * a row group's selected chunks into pinned output segments, ParquetReader.java:183-192): all
 * capacities are checked first (PF_ERR_CAPACITY, nothing enqueued), then the D2H copies of the
 * n chunks are enqueued on the context stream. Destination buffers should be pinned
 * (pf_host_alloc) and stay valid until pf_sync. A later pf_decode_row_group on the same
 * context is ordered after these copies (same stream), so decode i+1 can be enqueued at once. */
int pf_copy_columns_async(pf_ctx* ctx, int n, const int* chunks, const pf_column_out* outs);

/* Whole-batch form for the end-to-end pipeline: ONE D2H copy per output arena (values / offsets /
 * levels, validity bits, chars) into a caller buffer of pf_batch_bytes bytes (pinned), instead of
 * up to 8 copies per chunk. After pf_sync, pf_column_info_host returns chunk i's pf_column_info
 * with its d_* pointers rebased into that host buffer (same layout rules as the device arrays).
 * Valid after pf_wait until the next decode on this context. A mapped pinned buffer (pf_host_alloc,
 * hipHostMalloc) is written by a download kernel on a copy stream the context shares with its twin
 * (pf_ctx_create_shared), ordered after the decode, so the link carries uploads and downloads at
 * once (round 6); any other buffer takes SDMA copies on the context stream. All three return PF_ERR_STATE after a
 * pf_decode_row_group_rows in which any chunk had a window other than {0, -1}: use pf_copy_column(s_async) there. */
int pf_batch_bytes(pf_ctx* ctx, size_t* bytes);
int pf_copy_batch_async(pf_ctx* ctx, void* host, size_t cap);
int pf_column_info_host(pf_ctx* ctx, int chunk, const void* host, pf_column_info* out);

/* Block until the copies this context enqueued (pf_copy_columns_async / pf_copy_batch_async) have
 * finished. A peer context's decode queued behind them on a shared stream is not waited for. */
int pf_sync(pf_ctx* ctx);

/* Kernel timing of the last decode (sum of per-stage HIP-event times, ms). */
int pf_last_timing(pf_ctx* ctx, float* stage_ms, int n_stages, int* n_written);

/* Decompress one raw Snappy buffer (snappy-java Snappy.uncompress semantics) with the
 * page kernels (K1). Host buffers; synchronous. *out_len = uncompressed length.
 * Invalidates the results of the last pf_decode_row_group on this context. */
int pf_snappy_decompress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len);
/* Decompress one buffer of Zstandard frames (RFC 8878: concatenated and skippable frames, no
 * dictionary; the content checksum is consumed, not verified) with the page kernel. Host buffers;
 * synchronous. dst takes up to cap bytes; *out_len = bytes produced. PF_ERR_CORRUPT_PAGE when the
 * frames are damaged or produce more than cap. Invalidates the results of the last
 * pf_decode_row_group on this context. */
int pf_zstd_decompress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len);
/* Decompress one raw LZ4 block (the LZ4 block format, parquet-format codec LZ4_RAW: no frame, no
 * length) with the page kernel. The format carries no length, so the block has to produce exactly
 * size bytes: PF_ERR_CORRUPT_PAGE when it is damaged or produces one byte less or more; offset 0
 * and an empty src are refused. Host buffers of at most 1 GiB; synchronous. *out_len = size on
 * success. Invalidates the results of the last pf_decode_row_group on this context. */
int pf_lz4_decompress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t size, size_t* out_len);
/* 1 if the last pf_snappy_decompress needed the serial fallback kernel (stream not split into
 * independent 64 KiB blocks, or corrupt), 0 if the block-parallel kernels decoded it. */
int pf_snappy_last_fallback(pf_ctx* ctx);

/* ---- GPU page-header scan (the per-page Thrift walk of ParquetFileReader.readNextRowGroup,
 *      ParquetReader.java:183, moved to the device) with optional page CRC32 verification
 *      (parquet-mr ParquetReadOptions.usePageChecksumVerification: a page whose PageHeader.crc,
 *      field 4, differs from the CRC32 of its on-disk page bytes is rejected). Pages are read
 *      until the chunk's num_values level entries have been seen; INDEX / unknown pages are
 *      skipped; the descriptors are exactly what pf_file_chunk_desc (the host walk) produces.
 *      Both walks read Thrift compact as libthrift does: a field id is kept as i16, a bool inside a
 *      list, set or map is one byte, a varint has at most 10 bytes. A value they skip (an unknown
 *      field, Statistics min / max, ...) may have at most PF_THRIFT_MAX_NESTING containers (struct,
 *      list, set, map; the value itself included) open at once; one more is PF_ERR_CORRUPT_PAGE
 *      (libthrift itself reads deeper ones; no writer emits them). The walk of a chunk takes a number of steps bounded by the
 *      chunk's size, whatever its bytes say. */
#define PF_THRIFT_MAX_NESTING 16
typedef struct pf_scan_chunk {
    uint64_t chunk_offset;        /* first byte of the chunk in `bytes` */
    uint64_t chunk_size;          /* ColumnMetaData.total_compressed_size */
    int64_t  num_values;          /* ColumnMetaData.num_values */
    int32_t  page_base;           /* first slot of this chunk's descriptors in pages_out */
    int32_t  page_cap;            /* slots available to it */
} pf_scan_chunk;
typedef struct pf_scan_result {
    int32_t n_pages;              /* dictionary + data pages found */
    int32_t status;               /* PF_OK, PF_ERR_CORRUPT_PAGE (header, bounds or CRC), PF_ERR_CAPACITY */
    int32_t err_page;             /* chunk-relative page of the first error, -1 */
    int32_t crc_pages;            /* pages whose CRC was verified (verify_crc, header has a crc) */
} pf_scan_result;
/* Synchronous. `bytes` is host memory (copied to the device) unless bytes_on_device != 0.
 * pages_out has room for every chunk's [page_base, page_base + page_cap) slots; results has
 * n_chunks entries. Returns the first chunk error (PF_OK if none). Of a chunk's slots only the
 * first n_pages are written with descriptors: the slots past them, and slots no chunk owns, hold
 * whatever the context's scan buffer held before (unspecified). */
int pf_scan_pages(pf_ctx* ctx, const pf_scan_chunk* chunks, int n_chunks, const uint8_t* bytes, size_t n_bytes,
                  int bytes_on_device, int verify_crc, pf_page_desc* pages_out, pf_scan_result* results);
/* ---- host-side metadata parse: the stand-in for the Java side's parquet-mr footer /
 *      PageHeader parse (ParquetFileReader.open + readNextRowGroup,
 *      ParquetReader.java:120, :183). Builds the descriptors above from a file. ---- */
typedef struct pf_file pf_file;

typedef struct pf_column_meta {
    const char* path;             /* dotted path_in_schema */
    const char* top_name;         /* ColumnDescriptor.getPath()[0] (the Hydrator heading) */
    int32_t physical_type, type_length, max_def, max_rep, repeated_def, list_null_def;
    int32_t converted_type;       /* SchemaElement.converted_type or -1 */
    int32_t logical_type;         /* LogicalType union field id or 0 */
    int32_t scale, precision;     /* DECIMAL (SchemaElement 7/8 or LogicalType DecimalType) */
} pf_column_meta;

int pf_file_open(const char* path, pf_file** out);
int pf_file_close(pf_file* f);
int pf_file_num_row_groups(pf_file* f, int* out);
int pf_file_num_columns(pf_file* f, int* out);
int pf_file_num_rows(pf_file* f, int64_t* out);
int pf_file_column_meta(pf_file* f, int column, pf_column_meta* out);
int pf_file_row_group_rows(pf_file* f, int row_group, int64_t* out);
/* Byte range [start, start+size) of a chunk in the file. */
int pf_file_chunk_range(pf_file* f, int row_group, int column, uint64_t* start, uint64_t* size);
/* Parse the chunk's page headers; fills *desc (pages owned by the pf_file) with
 * chunk_offset = `chunk_offset_in_buffer`. The walk pf_scan_pages mirrors: the same Thrift reading
 * and the same PF_THRIFT_MAX_NESTING (above). */
int pf_file_chunk_desc(pf_file* f, int row_group, int column, uint64_t chunk_offset_in_buffer,
                       pf_chunk_desc* desc);
/* Read raw bytes of the file (host). */
int pf_file_read(pf_file* f, uint64_t offset, uint64_t size, void* dst);
/* The chunk's Bloom filter: *offset = ColumnMetaData.bloom_filter_offset (the file offset of its BloomFilterHeader), -1
 * if it has none; *length = bloom_filter_length (header + bitset), -1 if the writer left it out (parquet-mr 1.12: read
 * the header for numBytes). PF_ERR_IO if either points outside the file. */
int pf_file_chunk_bloom(pf_file* f, int row_group, int column, int64_t* offset, int32_t* length);
/* The chunk's page index (host only, no context). Ranges in the file: ColumnChunk column_index_offset / _length and
 * offset_index_offset / _length; -1 where absent. PF_ERR_IO if a range leaves the file. */
int pf_file_chunk_index_ranges(pf_file* f, int row_group, int column, int64_t* ci_off, int32_t* ci_len,
                               int64_t* oi_off, int32_t* oi_len);
typedef struct pf_page_location {
    int64_t offset;               /* file offset of the page header */
    int32_t compressed_page_size; /* header + stored body */
    int64_t first_row_index;      /* within the row group */
} pf_page_location;
/* OffsetIndex.page_locations: *n = their number (also when it exceeds cap: PF_ERR_CAPACITY, the first cap are written);
 * out may be NULL with cap 0. PF_ERR_STATE if the chunk has no OffsetIndex; PF_ERR_CORRUPT_PAGE if the struct is
 * damaged (a varint overrun, a size past the range); never an out-of-bounds read. Unknown fields are skipped. */
int pf_file_offset_index(pf_file* f, int row_group, int column, pf_page_location* out, int cap, int* n);
typedef struct pf_column_index {
    int32_t n_pages;
    int32_t boundary_order;       /* 0 UNORDERED, 1 ASCENDING, 2 DESCENDING */
    const uint8_t* null_pages;    /* n_pages bytes, 0 / 1 */
    const int64_t* null_counts;   /* n_pages, or NULL when the writer left them out */
    const uint8_t* values;        /* min and max of every page, back to back */
    const uint32_t* value_off;    /* 2 * n_pages + 1: page p's min is [off[2p], off[2p+1]), its max [off[2p+1], off[2p+2]) */
} pf_column_index;
/* ColumnIndex; the arrays are owned by the pf_file (valid until it is closed). PF_ERR_STATE if the chunk has none;
 * PF_ERR_CORRUPT_PAGE if the struct is damaged (list lengths that disagree, a varint overrun, a size past the
 * range). Unknown fields (the level histograms) are skipped. */
int pf_file_column_index(pf_file* f, int row_group, int column, pf_column_index* out);
/* ---- reading a row range of a row group. pf_file_chunk_desc_rows selects the data pages that hold rows
 *      [row_lo, row_hi) through the chunk's OffsetIndex and reads nothing else of the chunk: the index, the dictionary
 *      page (the bytes between the chunk's start and the first page location) and the selected pages' file range.
 *      `desc` describes a buffer that holds the dictionary range followed directly by the data range, starting at
 *      offset_in_buffer (chunk_size = dict_size + data_size; page offsets are relative to that start; num_rows = the
 *      rows the selected pages cover, from the index). The caller reads the two ranges into that buffer and passes
 *      {skip_rows, take_rows} to pf_decode_row_group_rows. A chunk without an OffsetIndex gets the descriptor of
 *      pf_file_chunk_desc (every page) with indexed = 0, first_row = 0, skip_rows = row_lo: the window still trims it.
 *      0 <= row_lo <= row_hi <= RowGroup.num_rows, else PF_ERR_INVALID_ARG. An empty range selects no page (all sizes
 *      0, first_row = row_lo). Headers are read at the locations the index gives, by the reader and with the limits of
 *      pf_file_chunk_desc. PF_ERR_CORRUPT_PAGE: a location outside the chunk, locations or first_row_index not
 *      increasing (the first row index must be 0), a compressed_page_size shorter than the header plus the stored body,
 *      a location of no data page, v2 num_rows that disagree with the index. The page arrays are owned by the pf_file,
 *      one per chunk, apart from those of pf_file_chunk_desc (valid until the next call for the same chunk). ---- */
typedef struct pf_chunk_rows {
    int32_t  indexed;        /* 1: pages were selected through the OffsetIndex; 0: the chunk has none, every page is listed */
    int32_t  first_page;     /* index (among the chunk's data pages) of the first data page selected */
    int32_t  n_data_pages;   /* data pages selected */
    int64_t  first_row;      /* row (within the row group) of the first entry of the first selected data page */
    int64_t  skip_rows;      /* row_lo - first_row */
    int64_t  take_rows;      /* row_hi - row_lo */
    uint64_t dict_start, dict_size;   /* file range of the dictionary page (header + body); size 0: none */
    uint64_t data_start, data_size;   /* file range of the selected data pages (headers + bodies, contiguous) */
} pf_chunk_rows;
int pf_file_chunk_desc_rows(pf_file* f, int row_group, int column, int64_t row_lo, int64_t row_hi,
                            uint64_t offset_in_buffer, pf_chunk_desc* desc, pf_chunk_rows* rows);
const char* pf_file_created_by(pf_file* f);

/* ---- write path: the reference's ParquetWriter (ParquetWriter.java:61-165: SNAPPY,
 *      WriterVersion.PARQUET_2_0, parquet-mr 1.12.2 defaults) with the column encoding on the
 *      GPU: dictionary encode (entries in first-occurrence order, like parquet-mr's
 *      DictionaryValuesWriter), RLE/bit-packed hybrid ids, PLAIN values, Snappy compression of
 *      every page. Flat schemas of the types the reference writes (ParquetWriter.java:143-157):
 *      BOOLEAN, INT32, INT64, FLOAT, DOUBLE, BYTE_ARRAY (UTF8). Opt-in, also on the GPU: statistics, page CRCs, the
 *      page index (PF_ENCODE_* bits below) and a split-block Bloom filter per chunk (pf_encode_column.bloom_bytes);
 *      pf_writer_close stores indexes and filters behind the last row group. ---- */
/* pf_encode_column.dictionary is a bit set (0 and 1 keep the meaning they always had). */
#define PF_ENCODE_DICTIONARY     1   /* dictionary-encode; the chunk falls back as a whole above
                                        dict_page_limit, on a hash collision, or for BOOLEAN */
#define PF_ENCODE_DELTA_FALLBACK 2   /* a chunk that is not dictionary-encoded (bit 0 clear, or any fallback)
                                        gets the encodings parquet-mr's PARQUET_2_0 writer falls back to:
                                        DELTA_BINARY_PACKED (INT32, INT64), DELTA_BYTE_ARRAY (BYTE_ARRAY);
                                        FLOAT, DOUBLE and BOOLEAN stay PLAIN. Clear: PLAIN */
#define PF_ENCODE_HYBRID_RUNS    4   /* RLE / bit-packed hybrid streams in the run shape of parquet-mr's
                                        RunLengthBitPackingHybridEncoder (RLE runs of >= 8 repeats between
                                        bit-packed groups), encoded on the GPU: the ids of RLE_DICTIONARY pages
                                        (width of dict_entries - 1: 0 for one entry), the definition levels of
                                        an OPTIONAL column whatever its values' encoding, and BOOLEAN values
                                        (PF_ENC_RLE: 4-byte length + stream). Clear: ids and levels are one
                                        bit-packed run per page, BOOLEAN is PLAIN */
#define PF_ENCODE_STATISTICS     8   /* Statistics (null_count, min_value / max_value, the legacy min / max where
                                        parquet-mr writes them) in every DataPageHeaderV2 and, through
                                        pf_writer_add_chunk, in ColumnMetaData, reduced on the GPU over the
                                        present values under ColumnOrder TYPE_ORDER: signed integers; NaN
                                        skipped, a zero min written -0.0 and a zero max +0.0; BYTE_ARRAY
                                        unsigned bytewise, untruncated; none when len(min) + len(max) >= 4096.
                                        Clear: no statistics, the bytes of every release before it */
#define PF_ENCODE_PAGE_CRC       16  /* PageHeader.crc (CRC-32 of the compressed_page_size bytes after the
                                        header, dictionary pages included), its pieces reduced on the GPU.
                                        Clear: no crc field */
#define PF_ENCODE_PAGE_INDEX 32      /* the chunk's page index (ColumnIndex and OffsetIndex of parquet-format's
                                        PageIndex): per data page null_page, null_count and min / max, the boundary
                                        order of the written values, and every page's location; built on the GPU
                                        from the results of the statistics kernels (pf_encoded_chunk.index_*).
                                        pf_writer_close stores them between the last row group and the Bloom filters.
                                        Independent of PF_ENCODE_STATISTICS: alone it runs the statistics kernels but
                                        writes no Statistics struct. Clear: no index, the bytes of every release
                                        before it */
#define PF_STATS_NULL_COUNT 1        /* pf_encoded_chunk.stats_flags: null_count is set */
#define PF_STATS_MIN_MAX    2        /* stat_min / stat_max are set */
typedef struct pf_encode_column {
    int32_t  physical_type;       /* PF_BOOLEAN, PF_INT32, PF_INT64, PF_FLOAT, PF_DOUBLE, PF_BYTE_ARRAY */
    int32_t  max_def;             /* 0 = REQUIRED, 1 = OPTIONAL */
    int64_t  num_rows;
    const void*    values;        /* fixed width, row-indexed (null rows ignored); BOOLEAN: one byte per row */
    const uint8_t* validity;      /* LSB-first, bit = present; NULL = all present (max_def 1) */
    const int32_t* offsets;       /* BYTE_ARRAY: num_rows + 1 (null rows: empty) */
    const uint8_t* chars;         /* BYTE_ARRAY */
    int64_t  chars_len;
    int32_t  dictionary;          /* PF_ENCODE_* bits; 1: dictionary-encode (PLAIN above dict_page_limit or on a
                                     hash collision), 3: the same with the DELTA_* fallback, 2: DELTA_* pages;
                                     | 4: parquet-mr's hybrid runs (7 = the encodings of its PARQUET_2_0 writer);
                                     | 8: statistics; | 16: page CRCs; | 32: page index */
    int32_t  page_rows;           /* rows per data page; 0 = 20000 (parquet-mr page.row.count.limit) */
    int32_t  dict_page_limit;     /* dictionary page bytes; 0 = 1 MiB (parquet.dictionary.page.size) */
    int32_t  codec;               /* PF_CODEC_SNAPPY (the reference's), PF_CODEC_ZSTD (every page section one frame,
                                     compressed on the GPU) or PF_CODEC_UNCOMPRESSED; others: PF_ERR_UNSUPPORTED_CODEC */
    int32_t  bloom_bytes;         /* split-block Bloom filter of the chunk's present values, filled on the GPU: its
                                     size in bytes, a power of two in [32, 128 MiB] (else PF_ERR_INVALID_ARG);
                                     0 = none, the bytes of every release before it. BOOLEAN: ignored, no filter */
    int32_t  index_truncate;      /* PF_ENCODE_PAGE_INDEX, BYTE_ARRAY: the longest min / max the ColumnIndex holds.
                                     0 = 64 (parquet-mr parquet.columnindex.truncate.length), -1 = no truncation,
                                     else in [1, 2047] (otherwise PF_ERR_INVALID_ARG). A longer min is cut to its
                                     first T bytes; a longer max is its first T bytes less trailing 0xFF bytes with
                                     the last byte left incremented (unsigned bytewise order; UTF-8 is not kept
                                     valid). Ignored for the other types and with the bit clear */
} pf_encode_column;

typedef struct pf_encoded_chunk {
    const uint8_t* bytes;         /* page headers + bodies as they appear in the file (owned by the ctx,
                                     valid until its next pf_encode_chunk) */
    int64_t  size;                /* = ColumnMetaData.total_compressed_size */
    int64_t  total_uncompressed_size;
    int64_t  num_values;
    int64_t  dictionary_page_offset;   /* relative to bytes, -1 if none */
    int64_t  data_page_offset;         /* relative to bytes */
    int32_t  n_data_pages;
    int32_t  dict_entries;        /* 0 when not dictionary-encoded */
    int32_t  data_encoding;       /* PF_ENC_RLE_DICTIONARY or PF_ENC_PLAIN; with PF_ENCODE_DELTA_FALLBACK also
                                     PF_ENC_DELTA_BINARY_PACKED / PF_ENC_DELTA_BYTE_ARRAY; with
                                     PF_ENCODE_HYBRID_RUNS PF_ENC_RLE for BOOLEAN */
    int32_t  fallback;            /* 0; 1 dictionary above the limit; 2 hash collision; 3 type (BOOLEAN) */
    int32_t  codec;               /* ColumnMetaData.codec */
    float    snappy_ms;           /* the compressor's time, k_snappy_compress or k_zstd_compress, whichever codec ran (the
                                     name is older than ZSTD; HIP events; 0 when stage timing is off) */
    float    encode_ms;           /* dictionary + page (PLAIN, ids, DELTA_*, hybrid runs) kernels time (HIP events; 0 when timing is off) */
    int64_t  snappy_in, snappy_out;    /* bytes into / out of the compressor, for whichever codec ran */
    /* Chunk statistics (PF_ENCODE_STATISTICS; all zero: none). pf_writer_add_chunk writes them as
     * ColumnMetaData.statistics, and a file with any gets FileMetaData.column_orders (TYPE_ORDER). */
    int32_t  stats_flags;         /* PF_STATS_* */
    int32_t  stat_min_len, stat_max_len;
    int64_t  null_count;
    const uint8_t* stat_min;      /* PLAIN bytes of the min / max (BYTE_ARRAY: no length prefix); owned by the ctx, */
    const uint8_t* stat_max;      /* valid until its next pf_encode_chunk, like bytes */
    /* Split-block Bloom filter (pf_encode_column.bloom_bytes; bloom_len 0: none): XXH64, seed 0, of the PLAIN bytes of
     * every present value (BYTE_ARRAY: without the length prefix; FLOAT / DOUBLE: the bits, so NaN payloads count and
     * -0.0 and +0.0 are two values) sets one bit in each of the eight uint32 words of the 32-byte block
     * ((hash >> 32) * blocks) >> 32. It does not depend on how the chunk was encoded. pf_writer_add_chunk copies it;
     * pf_writer_close stores it with its BloomFilterHeader behind the last row group. */
    const uint8_t* bloom;         /* the bitset alone, words little-endian; owned by the ctx, valid until its next
                                     pf_encode_chunk, like bytes */
    int32_t  bloom_len;
    float    bloom_ms;            /* the filter's zeroing and k_enc_bloom (HIP events; 0 when timing is off); not in encode_ms */
    /* Page index (PF_ENCODE_PAGE_INDEX; all zero / NULL with the bit clear). Arrays are owned by the ctx and valid until
     * its next pf_encode_chunk, like bytes. pf_writer_add_chunk copies them. */
    int32_t  index_pages;         /* = n_data_pages */
    const int64_t* page_offset;   /* OffsetIndex: every data page's header, relative to bytes */
    const int32_t* page_size;     /* header + stored body */
    const int64_t* page_first_row;
    int32_t  column_index;        /* 1: a ColumnIndex follows. 0: none (the OffsetIndex is written all the same): a page has
                                     present values but no min / max (FLOAT / DOUBLE, all NaN), a BYTE_ARRAY max cannot be
                                     truncated (its first T bytes are all 0xFF), or, with index_truncate = -1, an entry has
                                     len(min) + len(max) >= 4096. index_values / index_value_off are then NULL */
    int32_t  boundary_order;      /* 0 UNORDERED, 1 ASCENDING, 2 DESCENDING: over the written (truncated) min and max of the
                                     pages that are not null pages; ties and a single such page are ASCENDING, none UNORDERED */
    const uint8_t* index_null_pages;    /* one byte per page: 1 = the page has no present value */
    const int64_t* index_null_counts;
    const uint8_t* index_values;        /* the pages' min and max, PLAIN bytes (BYTE_ARRAY: no length prefix), back to back */
    const uint32_t* index_value_off;    /* 2 * index_pages + 1: page p's min is [off[2p], off[2p+1]), its max
                                           [off[2p+1], off[2p+2]); both empty for a null page */
} pf_encoded_chunk;

/* Encode one column chunk on the context's GPU. Inputs are host memory (copied) unless
 * on_device != 0. Synchronous. */
int pf_encode_chunk(pf_ctx* ctx, const pf_encode_column* col, int on_device, pf_encoded_chunk* out);
/* Snappy-compress one buffer on the GPU: independent 8 KiB jobs (one wave each; a job's matches stay
 * inside it, so tokens never cross a 64 KiB output boundary). Host buffers, synchronous;
 * *out_len = compressed length (cap >= 32 + n + n / 6 always suffices). */
int pf_snappy_compress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len);
/* ZSTD-compress one buffer on the GPU into one frame (RFC 8878; single segment, content size, no dictionary, no
 * checksum): independent 8 KiB jobs, one block each (RLE, compressed with Huffman literals and the predefined
 * sequence tables, or raw when that is not smaller). Host buffers, synchronous; *out_len = compressed length, also
 * when it exceeds cap (PF_ERR_CAPACITY; cap >= 12 + n + 3 * (n / 8192 + 1) always suffices). */
int pf_zstd_compress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len);

/* File writer (host): "PAR1", row groups of encoded chunks, Thrift compact FileMetaData footer. */
typedef struct pf_writer pf_writer;
typedef struct pf_write_field {
    const char* name;
    int32_t physical_type;
    int32_t optional;             /* 1 = OPTIONAL, 0 = REQUIRED */
    int32_t utf8;                 /* BYTE_ARRAY: STRING logical type (the only BINARY the reference writes) */
} pf_write_field;
int pf_writer_open(const char* path, const pf_write_field* fields, int n_fields, pf_writer** out);
/* Append the chunk of field `field` (fields in schema order) to the current row group. A Bloom filter
 * (bloom_len > 0: a power of two >= 32, bloom not null, else PF_ERR_INVALID_ARG) is copied and kept until close,
 * and so is a page index (index_pages > 0: page_offset, page_size, page_first_row, index_null_pages and
 * index_null_counts not null; column_index = 1: index_values and index_value_off not null and the offsets
 * non-decreasing; else PF_ERR_INVALID_ARG). */
int pf_writer_add_chunk(pf_writer* w, int field, const pf_encoded_chunk* chunk);
int pf_writer_end_row_group(pf_writer* w, int64_t num_rows);
/* Behind the last row group, in the order of parquet-mr 1.12's ParquetFileWriter.end(): every ColumnIndex
 * {1 null_pages, 2 min_values, 3 max_values, 4 boundary_order, 5 null_counts} in row-group then column order, every
 * OffsetIndex {1 page_locations {1 offset, 2 compressed_page_size, 3 first_row_index}} in the same order (ColumnChunk
 * offset_index_offset 4 / offset_index_length 5 / column_index_offset 6 / column_index_length 7; a file with any
 * ColumnIndex declares column_orders), the Bloom filters (BloomFilterHeader {1 numBytes, 2 BLOCK, 3 XXHASH,
 * 4 UNCOMPRESSED} + bitset each, same order; ColumnMetaData bloom_filter_offset 14 / bloom_filter_length 15), then the
 * footer; frees w (also on error). A file without indexed chunks keeps the bytes it always had. */
int pf_writer_close(pf_writer* w);
const char* pf_writer_last_error(void);
const char* pf_file_last_error(void);            /* thread-local message of the last pf_file_* error */

/* ---- probing a Bloom filter on the host (no context, no GPU): the hash and the block arithmetic are the text the
 *      kernel compiles (csrc/pf_xxh64.h). hash = pf_xxh64(PLAIN bytes of the value, n, 0). ---- */
uint64_t pf_xxh64(const void* p, size_t n, uint64_t seed);
/* 1: the value may be in the chunk; 0: it is not; PF_ERR_INVALID_ARG: n_bytes is no power of two in [32, 128 MiB].
 * bitset: the n_bytes behind the BloomFilterHeader. */
int pf_bloom_check(const uint8_t* bitset, size_t n_bytes, uint64_t hash);

#ifdef __cplusplus
}
#endif
#endif /* PFLOOR_H */
