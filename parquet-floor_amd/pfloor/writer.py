"""Host mirror of the reference's write API (src/main/java/blue/strategic/parquet/ParquetWriter.java,
Dehydrator.java, ValueWriter.java) over the GPU write path of libpfloor.so.

ParquetWriter.writeFile(schema, file, dehydrator) -> writer; writer.write(record); writer.close().
Like the reference (ParquetWriter.java:61-68) every column is SNAPPY-compressed with the
PARQUET_2_0 writer settings of parquet-mr 1.12.2: data pages v2 of 20,000 rows, dictionary
encoding with a whole-chunk fallback above the 1 MiB dictionary page size. Records are buffered per
row group on the host (dehydrated column by column, SimpleWriteSupport.writeField :143-160) and
each column chunk is encoded on the GPU (pf_encode_chunk: dictionary build, ids, PLAIN or DELTA_*
values, Snappy), then appended with its page headers by the host file writer (pf_writer_*).

codec=ZSTD (ParquetWriter(..., codec=ZSTD), PF_CODEC_ZSTD) compresses every page section into one ZSTD frame on
the GPU instead (k_zstd_compress: 8 KiB blocks, Huffman literals, the predefined sequence tables), the codec most
engines write today; codec=UNCOMPRESSED stores the sections as they are. The default stays SNAPPY, and every
option below combines with every codec.

The fallback encoding is PLAIN by default. With delta_fallback=True a chunk that is not
dictionary-encoded is written as parquet-mr's v2 writer writes it: DELTA_BINARY_PACKED (INT32,
INT64) or DELTA_BYTE_ARRAY (BINARY) data pages, encoded on the GPU in parquet-mr's stream layout;
FLOAT, DOUBLE and BOOLEAN stay PLAIN.

With hybrid_runs=True (PF_ENCODE_HYBRID_RUNS) the RLE / bit-packed hybrid streams get the run shape of
parquet-mr's RunLengthBitPackingHybridEncoder, encoded on the GPU: RLE runs of 8 or more repeats
between bit-packed groups in the dictionary ids (width 0 for a one-entry dictionary) and in the
definition levels of an OPTIONAL column, and BOOLEAN chunks in the RLE encoding. By default ids and
levels are one bit-packed run per page and BOOLEAN is PLAIN. delta_fallback=True with
hybrid_runs=True gives the encodings parquet-mr's PARQUET_2_0 writer gives.

With statistics=True (PF_ENCODE_STATISTICS) every data page header and every ColumnMetaData carries a
Statistics struct (null_count, min_value / max_value, and the legacy min / max where parquet-mr writes
them), reduced on the GPU over the present values under ColumnOrder TYPE_ORDER, and the footer declares
column_orders so that readers use them to skip row groups and pages. With page_checksums=True
(PF_ENCODE_PAGE_CRC) every page header, dictionary pages included, carries PageHeader.crc, the CRC-32 of
the stored page bytes, its pieces computed on the GPU; pf_scan_pages(verify_crc=1), parquet-mr and
pyarrow verify it. With both off (the default) files are byte for byte what they were before.

With bloom_filters={name: ...} the named columns get a split-block Bloom filter (parquet-mr's
parquet.bloom.filter.enabled#name): XXH64 of the PLAIN bytes of every present value of a chunk, hashed and
inserted on the GPU (pf_encode_column.bloom_bytes), stored with its BloomFilterHeader behind the last row group
and located by ColumnMetaData.bloom_filter_offset / bloom_filter_length, where parquet-mr, Arrow C++, Impala,
Trino and DuckDB look for it to answer = and IN predicates. The size comes from an expected distinct count and
a false-positive probability (bloom_optimal_bytes, Arrow's and parquet-mr's formula), capped at bloom_max_bytes.
The filter does not depend on how the chunk is encoded. BOOLEAN columns get none.

Differences that are allowed by the format and documented in DESIGN.md: the fallback is decided
for the whole chunk (parquet-mr switches mid-chunk and also drops a dictionary that does not
compress, isCompressionSatisfying), ids are written as one bit-packed run per page unless
hybrid_runs is set, statistics, page checksums, Bloom filters and the page index are opt-in.

With page_index=True (PF_ENCODE_PAGE_INDEX) every chunk gets a ColumnIndex (per data page: null_page, min, max,
null_count, and the boundary order of the pages) and an OffsetIndex (every data page's file offset, size and first
row), the structures parquet-mr's ColumnIndexFilter, Impala, Trino, Spark and DuckDB skip pages by. The lists are
built on the GPU from the page results of the statistics kernels (k_enc_pgindex) and stored between the last row
group and the Bloom filters, all ColumnIndexes before all OffsetIndexes, as parquet-mr 1.12 and pyarrow store them.
BYTE_ARRAY min and max are truncated to index_truncate bytes (0: 64, parquet-mr's
parquet.columnindex.truncate.length; -1: never) under the unsigned bytewise order; UTF-8 is not kept valid, which only
non-ASCII strings can notice. A chunk with a page of NaNs alone, or with a max that cannot be shortened, gets an
OffsetIndex only. The option is independent of statistics=True.
"""
import ctypes as C
import math

import numpy as np

from . import _native
from ._native import PfError, check, lib

BOOLEAN, INT32, INT64, INT96, FLOAT, DOUBLE, BINARY, FIXED_LEN_BYTE_ARRAY = 0, 1, 2, 3, 4, 5, 6, 7
UNCOMPRESSED, SNAPPY, ZSTD = 0, 1, 6   # pf_encode_column.codec (PF_CODEC_*): the codecs the write path has
ENCODE_DICTIONARY, ENCODE_DELTA_FALLBACK, ENCODE_HYBRID_RUNS = 1, 2, 4   # pf_encode_column.dictionary bits (PF_ENCODE_*)
ENCODE_STATISTICS, ENCODE_PAGE_CRC, ENCODE_PAGE_INDEX = 8, 16, 32
UNORDERED, ASCENDING, DESCENDING = 0, 1, 2   # pf_encoded_chunk.boundary_order
STATS_NULL_COUNT, STATS_MIN_MAX = 1, 2   # pf_encoded_chunk.stats_flags (PF_STATS_*)
BLOOM_MIN_BYTES, BLOOM_MAX_BYTES = 32, 128 << 20   # pf_encode_column.bloom_bytes: a power of two between them
_WIDTH = {BOOLEAN: 1, INT32: 4, INT64: 8, FLOAT: 4, DOUBLE: 8}
_DTYPE = {BOOLEAN: np.uint8, INT32: np.int32, INT64: np.int64, FLOAT: np.float32, DOUBLE: np.float64}
_NAMES = {BOOLEAN: "BOOLEAN", INT32: "INT32", INT64: "INT64", INT96: "INT96", FLOAT: "FLOAT", DOUBLE: "DOUBLE",
          BINARY: "BINARY", FIXED_LEN_BYTE_ARRAY: "FIXED_LEN_BYTE_ARRAY"}


class EncodeColumn(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("max_def", C.c_int32), ("num_rows", C.c_int64),
                ("values", C.c_void_p), ("validity", C.c_void_p), ("offsets", C.c_void_p), ("chars", C.c_void_p),
                ("chars_len", C.c_int64), ("dictionary", C.c_int32), ("page_rows", C.c_int32),
                ("dict_page_limit", C.c_int32), ("codec", C.c_int32), ("bloom_bytes", C.c_int32),
                ("index_truncate", C.c_int32)]


class EncodedChunk(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("size", C.c_int64), ("total_uncompressed_size", C.c_int64),
                ("num_values", C.c_int64), ("dictionary_page_offset", C.c_int64), ("data_page_offset", C.c_int64),
                ("n_data_pages", C.c_int32), ("dict_entries", C.c_int32), ("data_encoding", C.c_int32),
                ("fallback", C.c_int32), ("codec", C.c_int32), ("snappy_ms", C.c_float), ("encode_ms", C.c_float),
                ("snappy_in", C.c_int64), ("snappy_out", C.c_int64),
                ("stats_flags", C.c_int32), ("stat_min_len", C.c_int32), ("stat_max_len", C.c_int32),
                ("null_count", C.c_int64), ("stat_min", C.c_void_p), ("stat_max", C.c_void_p),
                ("bloom", C.c_void_p), ("bloom_len", C.c_int32), ("bloom_ms", C.c_float),
                ("index_pages", C.c_int32), ("page_offset", C.POINTER(C.c_int64)), ("page_size", C.POINTER(C.c_int32)),
                ("page_first_row", C.POINTER(C.c_int64)), ("column_index", C.c_int32), ("boundary_order", C.c_int32),
                ("index_null_pages", C.POINTER(C.c_uint8)), ("index_null_counts", C.POINTER(C.c_int64)),
                ("index_values", C.POINTER(C.c_uint8)), ("index_value_off", C.POINTER(C.c_uint32))]

    def page_locations(self):
        """[(offset relative to bytes, size, first row)] of the data pages (PF_ENCODE_PAGE_INDEX), or None."""
        n = self.index_pages
        if n <= 0:
            return None
        return [(self.page_offset[i], self.page_size[i], self.page_first_row[i]) for i in range(n)]

    def page_column_index(self):
        """{"null_pages", "min_values", "max_values", "boundary_order", "null_counts"} of the chunk's ColumnIndex, or
        None when it has none (column_index == 0)."""
        n = self.index_pages
        if n <= 0 or not self.column_index:
            return None
        off = [self.index_value_off[i] for i in range(2 * n + 1)]
        raw = C.string_at(self.index_values, off[-1]) if off[-1] else b""
        return {"null_pages": [bool(self.index_null_pages[i]) for i in range(n)],
                "min_values": [raw[off[2 * i]:off[2 * i + 1]] for i in range(n)],
                "max_values": [raw[off[2 * i + 1]:off[2 * i + 2]] for i in range(n)],
                "boundary_order": self.boundary_order,
                "null_counts": [self.index_null_counts[i] for i in range(n)]}

    def statistics(self):
        """(null_count or None, min bytes or None, max bytes or None) of the chunk."""
        mm = bool(self.stats_flags & STATS_MIN_MAX)
        return (self.null_count if self.stats_flags & STATS_NULL_COUNT else None,
                C.string_at(self.stat_min, self.stat_min_len) if mm else None,
                C.string_at(self.stat_max, self.stat_max_len) if mm else None)

    def bloom_filter(self):
        """The chunk's split-block Bloom filter (the bitset alone, bloom_len bytes), or None."""
        return C.string_at(self.bloom, self.bloom_len) if self.bloom_len > 0 else None


def _bloom_cap(max_bytes):
    """max_bytes as a filter size: the largest power of two not above it, within the format's 32 bytes .. 128 MiB."""
    if max_bytes < BLOOM_MIN_BYTES:
        raise ValueError("bloom max_bytes must be >= 32")
    return min(1 << (int(max_bytes).bit_length() - 1), BLOOM_MAX_BYTES)


def bloom_optimal_bytes(ndv, fpp=0.01, max_bytes=1 << 20):
    """Bytes of a split-block Bloom filter for `ndv` distinct values at false-positive probability `fpp`:
    bits = -8 ndv / ln(1 - fpp^(1/8)) (eight bits per value and block: parquet-mr BlockSplitBloomFilter.optimalNumOfBits,
    Arrow BlockSplitBloomFilter::OptimalNumOfBits), rounded up to a power of two, at least 32 bytes and at most
    max_bytes (parquet.bloom.filter.max.bytes; rounded down to a power of two)."""
    if not 0.0 < fpp < 1.0 or ndv < 0:
        raise ValueError("fpp must be in (0, 1) and ndv >= 0")
    cap = _bloom_cap(max_bytes)
    bits = int(-8.0 * ndv / math.log(1.0 - fpp ** (1.0 / 8.0)))
    bits = max(bits, BLOOM_MIN_BYTES * 8)
    if bits & (bits - 1):
        bits = 1 << bits.bit_length()
    return min(bits >> 3, cap)


class WriteField(C.Structure):
    _fields_ = [("name", C.c_char_p), ("physical_type", C.c_int32), ("optional", C.c_int32), ("utf8", C.c_int32)]


class Field:
    """One primitive field of a flat MessageType (parquet-mr Types.required/optional(...).named)."""

    def __init__(self, name, physical_type, optional=False, string=False):
        self.name, self.physical_type, self.optional, self.string = name, physical_type, optional, string


class _Builder:
    def __init__(self, physical_type, optional):
        self.t, self.opt, self.string = physical_type, optional, False

    def as_string(self):
        self.string = True
        return self

    def named(self, name):
        return Field(name, self.t, self.opt, self.string)


def required(physical_type):
    return _Builder(physical_type, False)


def optional(physical_type):
    return _Builder(physical_type, True)


class MessageType:
    def __init__(self, name, *fields):
        self.name, self.fields = name, list(fields)
        self._index = {f.name: i for i, f in enumerate(self.fields)}

    def getFieldIndex(self, name):
        if name not in self._index:
            raise KeyError(f"{name} not found in {self.name}")   # parquet-mr InvalidRecordException
        return self._index[name]


class Dehydrator:
    """Dehydrator.java: dehydrate(record, valueWriter)."""

    def dehydrate(self, record, value_writer):
        raise NotImplementedError


class ValueWriter:
    """ValueWriter.java: write(name, value)."""

    def write(self, name, value):
        raise NotImplementedError


class _RowBuffer(ValueWriter):
    """SimpleWriteSupport.writeField (ParquetWriter.java:143-160) into per-column host buffers."""

    def __init__(self, schema):
        self.schema = schema
        self.cols = [[] for _ in schema.fields]
        self.rows = 0
        self._seen = [False] * len(schema.fields)

    def write(self, name, value):
        i = self.schema.getFieldIndex(name)
        f = self.schema.fields[i]
        t = f.physical_type
        if self._seen[i]:
            raise RuntimeError(f"field {name} written twice in one record")
        if t == INT32:
            v = int(value)
        elif t == INT64:
            v = int(value)
        elif t == DOUBLE:
            v = float(value)
        elif t == BOOLEAN:
            v = bool(value)
        elif t == FLOAT:
            v = float(value)
        elif t == BINARY:
            if not f.string:
                raise NotImplementedError("We don't support writing " + str(None))
            v = str(value).encode("utf-8")
        else:
            raise NotImplementedError("We don't support writing " + _NAMES.get(t, str(t)))
        self._seen[i] = True
        self.cols[i].append(v)

    def end_record(self):
        for i, f in enumerate(self.schema.fields):
            if not self._seen[i]:
                if not f.optional:
                    raise RuntimeError(f"required field {f.name} was not written")
                self.cols[i].append(None)
            self._seen[i] = False
        self.rows += 1

    def take(self):
        cols, self.cols, n = self.cols, [[] for _ in self.schema.fields], self.rows
        self.rows = 0
        return cols, n


def column_arrays(field, values):
    """Python values (None = null) -> (values | (offsets, chars), validity or None) numpy arrays."""
    n = len(values)
    present = np.fromiter((v is not None for v in values), dtype=bool, count=n)
    validity = np.packbits(present, bitorder="little") if (field.optional and not present.all()) else None
    if field.optional and validity is None:
        validity = np.packbits(np.ones(n, bool), bitorder="little")
    if field.physical_type == BINARY:
        lens = np.fromiter((len(v) if v is not None else 0 for v in values), dtype=np.int64, count=n)
        offsets = np.zeros(n + 1, np.int32)
        np.cumsum(lens, out=offsets[1:])
        chars = np.frombuffer(b"".join(v for v in values if v is not None), dtype=np.uint8)
        return (offsets, chars), validity
    dt = _DTYPE[field.physical_type]
    arr = np.fromiter((v if v is not None else 0 for v in values), dtype=dt, count=n)
    return arr, validity


class GpuColumnEncoder:
    """pf_encode_chunk on one context: numpy column -> pf_encoded_chunk (bytes stay in the ctx)."""

    def __init__(self, decoder):
        self.dec = decoder

    def encode(self, field, data, validity, n, dictionary=True, page_rows=0, dict_page_limit=0, codec=1,
               delta_fallback=False, hybrid_runs=False, statistics=False, page_checksums=False, bloom_bytes=0,
               page_index=False, index_truncate=0):
        """page_index: PF_ENCODE_PAGE_INDEX, the chunk's ColumnIndex lists and page locations
        (EncodedChunk.page_column_index(), page_locations()); index_truncate: the longest BINARY min / max in it (0: 64,
        -1: no truncation, else 1 .. 2047).
        bloom_bytes: the chunk's split-block Bloom filter, a power of two in [32, 128 MiB] (0: none;
        EncodedChunk.bloom_filter()). delta_fallback: PF_ENCODE_DELTA_FALLBACK, DELTA_* data pages for a chunk that is not
        dictionary-encoded (INT32, INT64, BINARY). hybrid_runs: PF_ENCODE_HYBRID_RUNS, ids, definition
        levels and BOOLEAN values as parquet-mr's hybrid encoder writes them (RLE runs and bit-packed groups).
        statistics: PF_ENCODE_STATISTICS, page and chunk Statistics. page_checksums: PF_ENCODE_PAGE_CRC,
        PageHeader.crc on every page."""
        c = EncodeColumn()
        c.physical_type = field.physical_type
        c.max_def = 1 if field.optional else 0
        c.num_rows = n
        keep = []
        if field.physical_type == BINARY:
            offsets, chars = data
            offsets = np.ascontiguousarray(offsets, np.int32)
            chars = np.ascontiguousarray(chars, np.uint8)
            keep += [offsets, chars]
            c.offsets = offsets.ctypes.data
            c.chars = chars.ctypes.data if chars.size else None
            c.chars_len = chars.size
        else:
            arr = np.ascontiguousarray(data)
            if arr.dtype.itemsize != _WIDTH[field.physical_type]:
                raise ValueError(f"{field.name}: {arr.dtype} does not match {_NAMES[field.physical_type]}")
            keep.append(arr)
            c.values = arr.ctypes.data
        if validity is not None:
            v = np.ascontiguousarray(validity, np.uint8)
            keep.append(v)
            c.validity = v.ctypes.data
        c.dictionary = ((ENCODE_DICTIONARY if dictionary else 0) | (ENCODE_DELTA_FALLBACK if delta_fallback else 0) |
                        (ENCODE_HYBRID_RUNS if hybrid_runs else 0) | (ENCODE_STATISTICS if statistics else 0) |
                        (ENCODE_PAGE_CRC if page_checksums else 0) | (ENCODE_PAGE_INDEX if page_index else 0))
        c.index_truncate = index_truncate
        c.page_rows = page_rows
        c.dict_page_limit = dict_page_limit
        c.codec = codec
        c.bloom_bytes = bloom_bytes
        out = EncodedChunk()
        check(lib().pf_encode_chunk(self.dec.h, C.byref(c), 0, C.byref(out)), self.dec.h, "pf_encode_chunk")
        return out


class ParquetWriter:
    """bsp/ParquetWriter.java: writeFile(schema, file, dehydrator), write(record), close().
    row_group_rows bounds the rows buffered per row group (parquet-mr flushes by its 128 MiB
    block size; the bound here is in rows, the byte size of a row group is the caller's)."""

    def __init__(self, schema, path, dehydrator, row_group_rows=1 << 20, device=0, decoder=None, codec=SNAPPY,
                 decoders=None, delta_fallback=False, hybrid_runs=False, statistics=False, page_checksums=False,
                 bloom_filters=None, bloom_fpp=0.01, bloom_max_bytes=1 << 20, page_index=False, index_truncate=0,
                 page_rows=0):
        """page_rows: rows per data page (0: 20,000, parquet-mr's page.row.count.limit; rounded up to a multiple of 8).
        page_index: a ColumnIndex and an OffsetIndex for every chunk (see above); index_truncate: the longest BINARY
        min / max in a ColumnIndex (0: 64, -1: no truncation, else 1 .. 2047).
        bloom_filters: {field name: expected distinct count | True (bloom_max_bytes) | {"bytes": n}}, the columns
        that get a Bloom filter, sized by bloom_optimal_bytes(ndv, bloom_fpp, bloom_max_bytes) (see above); an unknown
        name is a ValueError, a BOOLEAN field gets none.
        codec: SNAPPY (the default), ZSTD or UNCOMPRESSED; any other is refused (PF_ERR_UNSUPPORTED_CODEC).
        delta_fallback: chunks that are not dictionary-encoded get DELTA_* data pages (see above).
        hybrid_runs: ids, definition levels and BOOLEAN values in parquet-mr's hybrid run shape (see above).
        statistics: page and chunk Statistics and the footer's column_orders (see above).
        page_checksums: PageHeader.crc on every page (see above).
        decoders: several contexts (GpuDecoder) to encode the columns of a row group in parallel
        (one host thread each); chunks are still appended in schema order."""
        from .decoder import GpuDecoder
        self.schema, self.dehydrator = schema, dehydrator
        self.bloom_bytes = self._bloom_sizes(schema, bloom_filters, bloom_fpp, bloom_max_bytes)
        self.row_group_rows = row_group_rows
        self._own = decoder is None and not decoders
        self.dec = decoder or (decoders[0] if decoders else GpuDecoder(device))
        self.enc = GpuColumnEncoder(self.dec)
        self.encoders = [GpuColumnEncoder(d) for d in decoders] if decoders else [self.enc]
        self.kernel_ms = {"snappy": 0.0, "encode": 0.0, "snappy_in": 0, "snappy_out": 0}
        self.codec = codec
        self.delta_fallback = delta_fallback
        self.hybrid_runs = hybrid_runs
        self.statistics = statistics
        self.page_checksums = page_checksums
        self.page_index = page_index
        self.index_truncate = index_truncate
        self.page_rows = page_rows
        self.buf = _RowBuffer(schema)
        self.last_chunks = []     # (dict_entries, data_encoding, fallback) of the last row group
        fields = (WriteField * len(schema.fields))()
        self._names = [f.name.encode() for f in schema.fields]
        for i, f in enumerate(schema.fields):
            fields[i] = WriteField(self._names[i], f.physical_type, 1 if f.optional else 0, 1 if f.string else 0)
        self.w = C.c_void_p()
        rc = lib().pf_writer_open(str(path).encode(), fields, len(schema.fields), C.byref(self.w))
        if rc != 0:
            if self._own:
                self.dec.close()
            raise PfError(rc, "pf_writer_open: " + (lib().pf_writer_last_error() or b"").decode(errors="replace"))

    @staticmethod
    def _bloom_sizes(schema, spec, fpp, max_bytes):
        """bloom_filters -> filter bytes per field of the schema (0: none)."""
        sizes = [0] * len(schema.fields)
        for name, how in (spec or {}).items():
            if name not in schema._index:
                raise ValueError(f"bloom_filters: no field {name!r} in {schema.name}")
            if how is True:     # no distinct count: the cap, as parquet-mr 1.12 sizes it
                nbytes = _bloom_cap(max_bytes)
            elif isinstance(how, dict):
                nbytes = int(how["bytes"])
                if not (BLOOM_MIN_BYTES <= nbytes <= BLOOM_MAX_BYTES) or nbytes & (nbytes - 1):
                    raise ValueError(f"bloom_filters[{name!r}]: bytes must be a power of two in [32, 128 MiB]")
            else:
                nbytes = bloom_optimal_bytes(int(how), fpp, max_bytes)
            if schema.fields[schema._index[name]].physical_type != BOOLEAN:   # parquet-mr builds none for BOOLEAN
                sizes[schema._index[name]] = nbytes
        return sizes

    @staticmethod
    def writeFile(schema, out, dehydrator, **kw):
        return ParquetWriter(schema, out, dehydrator, **kw)

    def write(self, record):
        self.dehydrator.dehydrate(record, self.buf)
        self.buf.end_record()
        if self.buf.rows >= self.row_group_rows:
            self._flush()

    def write_columns(self, columns, n):
        """Columnar fast path: {name: array | (offsets, chars) | (array, validity)} for n rows,
        one row group (buffered records are flushed first)."""
        self._flush()
        self.last_chunks = []
        work = []
        for f in self.schema.fields:
            d = columns[f.name]
            validity = None
            if isinstance(d, tuple) and len(d) == 2 and f.physical_type != BINARY:
                d, validity = d
            elif isinstance(d, tuple) and len(d) == 3:
                d, validity = (d[0], d[1]), d[2]
            if f.optional and validity is None:
                validity = np.packbits(np.ones(n, bool), bitorder="little")
            work.append((f, d, validity))
        if len(self.encoders) == 1:
            for i, (f, d, validity) in enumerate(work):
                self._encode_add(f, d, validity, n, i)
        else:
            self._encode_parallel(work, n)
        self._end_group(n)

    def _encode_parallel(self, work, n):
        """Columns encoded concurrently, one host thread per context (ctypes releases the GIL), biggest
        first; each chunk's bytes are copied out of its context before the context encodes again."""
        import threading
        size = [sum(np.asarray(x).nbytes for x in (d if isinstance(d, tuple) else (d,))) for _f, d, _v in work]
        order = sorted(range(len(work)), key=lambda i: -size[i])
        results = [None] * len(work)
        lock = threading.Lock()
        errs = []

        def worker(enc):
            try:
                while True:
                    with lock:
                        if not order:
                            return
                        i = order.pop(0)
                    f, d, validity = work[i]
                    out = enc.encode(f, d, validity, n, codec=self.codec, delta_fallback=self.delta_fallback,
                                     hybrid_runs=self.hybrid_runs, statistics=self.statistics,
                                     page_checksums=self.page_checksums, bloom_bytes=self.bloom_bytes[i],
                                     page_index=self.page_index, index_truncate=self.index_truncate, page_rows=self.page_rows)
                    keep = C.create_string_buffer(C.string_at(out.bytes, out.size), max(1, out.size))
                    cp = EncodedChunk.from_buffer_copy(out)
                    cp.bytes = C.cast(keep, C.c_void_p)
                    if out.bloom_len > 0:   # the context owns the filter too
                        bf = C.create_string_buffer(out.bloom_filter(), out.bloom_len)
                        cp.bloom = C.cast(bf, C.c_void_p)
                        keep = (keep, bf)
                    if out.stats_flags & STATS_MIN_MAX:   # the context owns min / max too
                        lo = C.create_string_buffer(C.string_at(out.stat_min, out.stat_min_len), max(1, out.stat_min_len))
                        hi = C.create_string_buffer(C.string_at(out.stat_max, out.stat_max_len), max(1, out.stat_max_len))
                        cp.stat_min, cp.stat_max = C.cast(lo, C.c_void_p), C.cast(hi, C.c_void_p)
                        keep = (keep, lo, hi)
                    if out.index_pages > 0:   # ... and the page index
                        held = [keep]
                        np_, nv = out.index_pages, (out.index_value_off[2 * out.index_pages] if out.column_index else 0)
                        for name, ct, cnt in (("page_offset", C.c_int64, np_), ("page_size", C.c_int32, np_),
                                              ("page_first_row", C.c_int64, np_), ("index_null_pages", C.c_uint8, np_),
                                              ("index_null_counts", C.c_int64, np_), ("index_values", C.c_uint8, nv),
                                              ("index_value_off", C.c_uint32, 2 * np_ + 1)):
                            src = getattr(out, name)
                            if not src:
                                continue
                            arr = (ct * max(1, cnt))()
                            C.memmove(arr, src, C.sizeof(ct) * cnt)
                            setattr(cp, name, C.cast(arr, C.POINTER(ct)))
                            held.append(arr)
                        keep = tuple(held)
                    results[i] = (cp, keep)
            except Exception as e:   # reported after the join
                errs.append(e)

        ts = [threading.Thread(target=worker, args=(e,)) for e in self.encoders]
        [t.start() for t in ts]
        [t.join() for t in ts]
        if errs:
            raise errs[0]
        for i, (cp, _keep) in enumerate(results):
            self._add(cp, i)

    def _add(self, out, i):
        self.last_chunks.append((out.dict_entries, out.data_encoding, out.fallback))
        self.kernel_ms["snappy"] += out.snappy_ms
        self.kernel_ms["encode"] += out.encode_ms
        self.kernel_ms["snappy_in"] += out.snappy_in
        self.kernel_ms["snappy_out"] += out.snappy_out
        rc = lib().pf_writer_add_chunk(self.w, i, C.byref(out))
        if rc != 0:
            raise PfError(rc, "pf_writer_add_chunk: " + (lib().pf_writer_last_error() or b"").decode(errors="replace"))

    def _encode_add(self, f, data, validity, n, i):
        out = self.enc.encode(f, data, validity, n, codec=self.codec, delta_fallback=self.delta_fallback,
                              hybrid_runs=self.hybrid_runs, statistics=self.statistics,
                              page_checksums=self.page_checksums, bloom_bytes=self.bloom_bytes[i],
                              page_index=self.page_index, index_truncate=self.index_truncate, page_rows=self.page_rows)
        self._add(out, i)
        return out

    def _end_group(self, n):
        rc = lib().pf_writer_end_row_group(self.w, n)
        if rc != 0:
            raise PfError(rc, "pf_writer_end_row_group: " + (lib().pf_writer_last_error() or b"").decode(errors="replace"))

    def _flush(self):
        if self.buf.rows == 0:
            return
        cols, n = self.buf.take()
        self.last_chunks = []
        for i, f in enumerate(self.schema.fields):
            data, validity = column_arrays(f, cols[i])
            self._encode_add(f, data, validity, n, i)
        self._end_group(n)

    def close(self):
        if not self.w:
            return
        try:
            self._flush()
        finally:
            rc = lib().pf_writer_close(self.w)
            self.w = C.c_void_p()
            if self._own:
                self.dec.close()
        if rc != 0:
            raise PfError(rc, "pf_writer_close: " + (lib().pf_writer_last_error() or b"").decode(errors="replace"))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


__all__ = ["ParquetWriter", "bloom_optimal_bytes", "MessageType", "Field", "Dehydrator", "ValueWriter", "required", "optional",
           "BOOLEAN", "INT32", "INT64", "FLOAT", "DOUBLE", "BINARY", "UNCOMPRESSED", "SNAPPY", "ZSTD", "_native"]
