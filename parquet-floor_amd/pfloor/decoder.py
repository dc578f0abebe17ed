"""Host-side driver of the HIP decoder: file metadata (pf_file_*) and GPU contexts (pf_ctx).

`ParquetFile` plays the role of parquet-mr's footer/PageHeader parse (ParquetReader.java:120,
:183); `GpuDecoder` owns one pf_ctx (one GPU, one HIP stream) and turns column chunks into
decoded columnar numpy arrays in the canonical layout of include/pfloor.h."""
import ctypes as C
import os

import numpy as np

from ._native import (ChunkDesc, ChunkRows, ColumnIndex, ColumnInfo, ColumnMeta, ColumnOut, DictInfo, PageDesc, PageLocation,
                      Predicate, RowWindow, ScanChunk, ScanResult, SelectionInfo, check, lib)

CONVERTED_UTF8, CONVERTED_ENUM, CONVERTED_JSON = 0, 4, 19
LOGICAL_STRING, LOGICAL_ENUM, LOGICAL_JSON = 1, 4, 12


class ColumnDescriptor:
    """The parts of parquet-mr's ColumnDescriptor the reference reads
    (getPath(), getMaxDefinitionLevel(), getPrimitiveType(); ParquetReader.java:126-146)."""

    def __init__(self, index, m: ColumnMeta):
        self.index = index
        self.path = m.path.decode().split(".")
        self.physical_type = m.physical_type
        self.type_length = m.type_length
        self.max_def = m.max_def
        self.max_rep = m.max_rep
        self.repeated_def = m.repeated_def
        self.list_null_def = m.list_null_def
        self.converted_type = m.converted_type
        self.logical_type = m.logical_type
        self.scale = m.scale
        self.precision = m.precision

    def getPath(self):
        return list(self.path)

    def getMaxDefinitionLevel(self):
        return self.max_def

    def getMaxRepetitionLevel(self):
        return self.max_rep

    @property
    def is_string(self):
        return (self.converted_type in (CONVERTED_UTF8, CONVERTED_ENUM, CONVERTED_JSON) or
                self.logical_type in (LOGICAL_STRING, LOGICAL_ENUM, LOGICAL_JSON))

    def __repr__(self):
        return f"ColumnDescriptor({'.'.join(self.path)}, type={self.physical_type}, def={self.max_def}, rep={self.max_rep})"


def _bloom_header(raw):
    """(numBytes, the header's length) of a Thrift compact BloomFilterHeader {1: i32 numBytes, 2: algorithm, 3: hash,
    4: compression} (the three unions hold one empty struct each); unknown fields are skipped."""
    pos = 0

    def varint():
        nonlocal pos
        v = shift = 0
        while True:
            if pos >= len(raw) or shift > 63:
                raise ValueError("BloomFilterHeader: truncated")
            b = raw[pos]
            pos += 1
            v |= (b & 0x7f) << shift
            shift += 7
            if not b & 0x80:
                return v

    def skip(t):
        nonlocal pos
        if t in (1, 2):
            return
        if t == 3:
            pos += 1
        elif t in (4, 5, 6):
            varint()
        elif t == 7:
            pos += 8
        elif t == 8:
            pos += varint()
        elif t == 12:
            struct(None)
        else:
            raise ValueError(f"BloomFilterHeader: unexpected Thrift type {t}")

    def struct(out):
        nonlocal pos
        fid = 0
        while True:
            if pos >= len(raw):
                raise ValueError("BloomFilterHeader: truncated")
            b = raw[pos]
            pos += 1
            if b == 0:
                return
            t = b & 0x0f
            fid = fid + (b >> 4) if b >> 4 else ((lambda z: (z >> 1) ^ -(z & 1))(varint()))
            if out is not None and fid == 1 and t == 5:
                z = varint()
                out.append((z >> 1) ^ -(z & 1))
            else:
                skip(t)
    found = []
    struct(found)
    if not found or found[0] <= 0:
        raise ValueError("BloomFilterHeader: no numBytes")
    return found[0], pos


class ParquetFile:
    def __init__(self, path):
        L = lib()
        self.path = str(path)
        self.h = C.c_void_p()
        check(L.pf_file_open(self.path.encode(), C.byref(self.h)), None, f"open {self.path}")
        n = C.c_int()
        check(L.pf_file_num_row_groups(self.h, C.byref(n)))
        self.num_row_groups = n.value
        check(L.pf_file_num_columns(self.h, C.byref(n)))
        self.num_columns = n.value
        r = C.c_int64()
        check(L.pf_file_num_rows(self.h, C.byref(r)))
        self.num_rows = r.value
        self.columns = []
        for i in range(self.num_columns):
            m = ColumnMeta()
            check(L.pf_file_column_meta(self.h, i, C.byref(m)))
            self.columns.append(ColumnDescriptor(i, m))
        self.created_by = (L.pf_file_created_by(self.h) or b"").decode(errors="replace")

    def close(self):
        if self.h:
            lib().pf_file_close(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def row_group_rows(self, rg):
        r = C.c_int64()
        check(lib().pf_file_row_group_rows(self.h, rg, C.byref(r)))
        return r.value

    def chunk_range(self, rg, col):
        s, n = C.c_uint64(), C.c_uint64()
        check(lib().pf_file_chunk_range(self.h, rg, col, C.byref(s), C.byref(n)))
        return s.value, n.value

    def chunk_desc(self, rg, col, offset_in_buffer):
        d = ChunkDesc()
        check(lib().pf_file_chunk_desc(self.h, rg, col, offset_in_buffer, C.byref(d)), None, f"pages rg{rg} c{col}")
        return d

    def chunk_desc_rows(self, rg, col, lo, hi, offset_in_buffer):
        """(ChunkDesc, ChunkRows) for rows [lo, hi) of a row group (pf_file_chunk_desc_rows): the data pages the
        OffsetIndex selects and the dictionary page, laid out as one buffer range that starts at offset_in_buffer;
        {skip_rows, take_rows} is the window GpuDecoder.decode takes. Every page of a chunk without an OffsetIndex."""
        d, r = ChunkDesc(), ChunkRows()
        check(lib().pf_file_chunk_desc_rows(self.h, rg, col, lo, hi, offset_in_buffer, C.byref(d), C.byref(r)), None,
              f"pages rg{rg} c{col} rows [{lo}, {hi})")
        return d, r

    def plan_rows(self, rg, columns, lo, hi, align=256):
        """Rows [lo, hi) of row group rg: every chunk's two file ranges (dictionary page, selected data pages) laid
        out back to back in one buffer. Returns ([(col, ChunkDesc, ChunkRows, offset_in_buffer)], total bytes,
        windows [(skip, take)]); read [dict_start, +dict_size) to offset_in_buffer and [data_start, +data_size)
        directly behind it (read_rows does)."""
        items, windows = [], []
        off = 0
        for col in columns:
            d, r = self.chunk_desc_rows(rg, col, lo, hi, off)
            items.append((col, d, r, off))
            windows.append((r.skip_rows, r.take_rows))
            off += (r.dict_size + r.data_size + align - 1) // align * align
        return items, off, windows

    def read_rows(self, items, base_ptr):
        """The file ranges of plan_rows' items into the buffer at base_ptr. Returns the bytes read."""
        n = 0
        for _col, _d, r, off in items:
            if r.dict_size:
                self.read_into(r.dict_start, r.dict_size, base_ptr + off)
            if r.data_size:
                self.read_into(r.data_start, r.data_size, base_ptr + off + r.dict_size)
            n += r.dict_size + r.data_size
        return n

    def candidate_rows(self, rg, col, lo=None, hi=None):
        """The ascending, disjoint, merged (row_lo, row_hi) ranges of the data pages that may hold a value v with
        lo <= v <= hi (None: unbounded), from the page index alone. A page is dropped only if it is a null page, or
        its max < lo, or its min > hi. INT32 / INT64 compare as signed integers (lo, hi: int); BYTE_ARRAY compares
        unsigned bytewise, a proper prefix first (lo, hi: bytes) -- truncated bounds are still bounds. Other types
        raise ValueError. [(0, rows)] for a chunk without a ColumnIndex or without an OffsetIndex."""
        pt = self.columns[col].physical_type
        if pt not in (1, 2, 6):
            raise ValueError(f"candidate_rows: unsupported physical type {pt}")
        rows = self.row_group_rows(rg)
        px = self.page_index(rg, col)
        oi, ci = px["offset_index"], px["column_index"]
        if oi is None or ci is None or len(oi) != len(ci["null_pages"]):
            return [(0, rows)]
        if pt == 6:
            def key(b):
                return bytes(b)   # Python compares bytes unsigned bytewise, a proper prefix first
        else:
            def key(b):
                return int.from_bytes(b, "little", signed=True)
        lo = None if lo is None else (bytes(lo) if pt == 6 else int(lo))
        hi = None if hi is None else (bytes(hi) if pt == 6 else int(hi))
        out = []
        for p, (_off, _size, first) in enumerate(oi):
            if ci["null_pages"][p]:
                continue
            if lo is not None and key(ci["max_values"][p]) < lo:
                continue
            if hi is not None and key(ci["min_values"][p]) > hi:
                continue
            end = oi[p + 1][2] if p + 1 < len(oi) else rows
            if out and out[-1][1] == first:
                out[-1] = (out[-1][0], end)
            else:
                out.append((first, end))
        return out

    def bloom_probe(self, rg, col, plain_bytes):
        """True: the value (its PLAIN bytes; BYTE_ARRAY without the length prefix) may be in the chunk; False: it is
        not; None: the chunk has no Bloom filter. Host only: pf_file_chunk_bloom, pf_file_read, pf_xxh64 and
        pf_bloom_check; the BloomFilterHeader is read for numBytes (and for its own length when the footer gives none)."""
        L = lib()
        off, length = C.c_int64(), C.c_int32()
        check(L.pf_file_chunk_bloom(self.h, rg, col, C.byref(off), C.byref(length)), None, f"bloom rg{rg} c{col}")
        if off.value < 0:
            return None
        head = (C.c_uint8 * 64)()
        file_size = os.path.getsize(self.path)
        n_head = min(64, file_size - off.value)
        self.read_into(off.value, n_head, C.addressof(head))
        num_bytes, header_len = _bloom_header(bytes(head[:n_head]))
        start = off.value + (length.value - num_bytes if length.value >= 0 else header_len)
        bits = (C.c_uint8 * max(1, num_bytes))()
        self.read_into(start, num_bytes, C.addressof(bits))
        self.bloom_bytes_read = getattr(self, "bloom_bytes_read", 0) + n_head + num_bytes
        raw = bytes(plain_bytes)
        buf = C.create_string_buffer(raw, max(1, len(raw)))
        rc = L.pf_bloom_check(bits, num_bytes, L.pf_xxh64(buf, len(raw), 0))
        if rc < 0:
            check(rc, None, f"bloom rg{rg} c{col}: a bitset of {num_bytes} bytes")
        return bool(rc)

    def prune_row_group(self, rg, preds, lo=0, hi=None):
        """What of rows [lo, hi) of a row group a conjunction of pfloor.predicate predicates can match, from the page
        index and the Bloom filters alone: None to skip the row group, or (row_lo, row_hi). Every Range / Eq on an INT32,
        INT64 or BYTE_ARRAY column contributes the hull of candidate_rows (no candidate page: skip); every Eq on a chunk
        with a Bloom filter is probed (a negative probe: skip); everything else leaves the range whole."""
        return self._prune(rg, preds, lo, hi)[0]

    def _prune(self, rg, preds, lo=0, hi=None):
        """(prune_row_group's result, "index" | "bloom" | None: what skipped the row group)."""
        from .predicate import Eq, Range, resolve
        hi = self.row_group_rows(rg) if hi is None else hi
        bound = []
        for p in preds:
            if isinstance(p, Range):
                col = resolve(self.columns, p.column)
                pt = self.columns[col].physical_type
                if pt in (1, 2, 6):
                    a, b = p.bounds(pt)
                    bound.append((p, col, pt, a, b))
        for p, col, pt, a, b in bound:
            def value(x):
                return None if x is None else (x if pt == 6 else int.from_bytes(x, "little", signed=True))
            cand = self.candidate_rows(rg, col, value(a), value(b))
            if not cand:
                return None, "index"
            lo, hi = max(lo, cand[0][0]), min(hi, cand[-1][1])
            if lo >= hi:
                return None, "index"
        for p, col, pt, a, b in bound:
            if isinstance(p, Eq) and self.bloom_probe(rg, col, a) is False:
                return None, "bloom"
        return (lo, hi), None

    def index_ranges(self, rg, col):
        """((column_index_offset, length) or None, (offset_index_offset, length) or None) of a chunk."""
        co, oo, cl, ol = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        check(lib().pf_file_chunk_index_ranges(self.h, rg, col, C.byref(co), C.byref(cl), C.byref(oo), C.byref(ol)),
              None, f"index ranges rg{rg} c{col}")
        return ((co.value, cl.value) if co.value >= 0 else None, (oo.value, ol.value) if oo.value >= 0 else None)

    def page_index(self, rg, col):
        """The chunk's page index as the file holds it: {"offset_index": [(offset, compressed_page_size,
        first_row_index)] or None, "column_index": {"null_pages": [bool], "min_values": [bytes], "max_values":
        [bytes], "boundary_order": 0 UNORDERED | 1 ASCENDING | 2 DESCENDING, "null_counts": [int] or None} or None}
        (pf_file_offset_index, pf_file_column_index; values are PLAIN bytes, possibly truncated bounds)."""
        ci_range, oi_range = self.index_ranges(rg, col)
        out = {"offset_index": None, "column_index": None}
        if oi_range:
            n = C.c_int()
            rc = lib().pf_file_offset_index(self.h, rg, col, None, 0, C.byref(n))
            if rc != -6:   # PF_ERR_CAPACITY reports the count
                check(rc, None, f"offset index rg{rg} c{col}")
            locs = (PageLocation * max(1, n.value))()
            check(lib().pf_file_offset_index(self.h, rg, col, locs, n.value, C.byref(n)), None, f"offset index rg{rg} c{col}")
            out["offset_index"] = [(locs[i].offset, locs[i].compressed_page_size, locs[i].first_row_index)
                                   for i in range(n.value)]
        if ci_range:
            ci = ColumnIndex()
            check(lib().pf_file_column_index(self.h, rg, col, C.byref(ci)), None, f"column index rg{rg} c{col}")
            n = ci.n_pages
            off = [ci.value_off[i] for i in range(2 * n + 1)]
            raw = C.string_at(ci.values, off[-1])
            out["column_index"] = {
                "null_pages": [bool(ci.null_pages[i]) for i in range(n)],
                "min_values": [raw[off[2 * i]:off[2 * i + 1]] for i in range(n)],
                "max_values": [raw[off[2 * i + 1]:off[2 * i + 2]] for i in range(n)],
                "boundary_order": ci.boundary_order,
                "null_counts": [ci.null_counts[i] for i in range(n)] if ci.null_counts else None}
        return out

    def read_into(self, offset, size, dst_ptr):
        check(lib().pf_file_read(self.h, offset, size, C.c_void_p(dst_ptr)))

    def plan(self, row_groups, columns, align=256):
        """Chunk byte ranges + descriptors laid out back to back in one buffer."""
        items = []
        off = 0
        for rg in row_groups:
            for col in columns:
                s, n = self.chunk_range(rg, col)
                items.append((rg, col, s, n, off))
                off += (n + align - 1) // align * align
        return items, off


class PinnedBuffer:
    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.ptr = C.c_void_p()
        self.nbytes = max(1, int(nbytes))
        check(lib().pf_host_alloc(ctx, self.nbytes, C.byref(self.ptr)), ctx, "pf_host_alloc")

    def array(self, dtype=np.uint8, n=None):
        n = self.nbytes // np.dtype(dtype).itemsize if n is None else n
        return np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(self.nbytes,)).view(dtype)[:n]

    def free(self):
        if self.ptr:
            lib().pf_host_free(self.ctx, self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _pack_predicates(predicates):
    """[(chunk, op, lo, hi)] as a ctypes Predicate array, and the bounds' buffers, which must stay alive over the call
    (the library copies them before it returns)."""
    preds = (Predicate * max(1, len(predicates)))()
    alive = []
    for i, (chunk, op, lo, hi) in enumerate(predicates):
        preds[i].chunk, preds[i].op = int(chunk), int(op)
        for side, b in (("lo", lo), ("hi", hi)):
            if b is not None:
                raw = C.create_string_buffer(bytes(b), max(1, len(b)))
                alive.append(raw)
                setattr(preds[i], side, C.addressof(raw))
                setattr(preds[i], side + "_len", len(b))
    return preds, alive


class GpuDecoder:
    """One pf_ctx = one GPU + one HIP stream."""

    def __init__(self, device=0, share=None):
        """share: another GpuDecoder whose HIP stream this context enqueues onto
        (pf_ctx_create_shared: pipelined decodes of consecutive batches)."""
        L = lib()
        self.h = C.c_void_p()
        if share is not None:
            check(L.pf_ctx_create_shared(share.h, C.byref(self.h)), None, "pf_ctx_create_shared")
            device = share.device
        else:
            check(L.pf_ctx_create(device, C.byref(self.h)), None, f"pf_ctx_create({device})")
        self.device = device
        self._staging = None
        self.n_chunks = 0

    def close(self):
        if self.h:
            if self._staging:
                self._staging.free()
                self._staging = None
            lib().pf_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def staging(self, nbytes):
        if self._staging is None or self._staging.nbytes < nbytes:
            if self._staging:
                self._staging.free()
            self._staging = PinnedBuffer(self.h, max(nbytes, 1 << 20))
        return self._staging

    def decode(self, descs, buf_ptr, nbytes, on_device=False, windows=None, predicates=None, keep=None):
        """descs: ChunkDesc list, or a prebuilt ctypes ChunkDesc array (no per-call copy). windows: one (skip_rows,
        take_rows) per chunk (take -1: to the end): the results are cut to those rows on the GPU
        (pf_decode_row_group_rows); None: pf_decode_row_group. predicates: a list of (chunk, op, lo, hi) -- chunk an
        index into descs, op a PF_PRED_* code, lo / hi the PLAIN bytes of a bound or None (pfloor.predicate.bind makes
        them): a conjunction evaluated on the GPU, every chunk compacted to the matching rows
        (pf_decode_row_group_filter; selection() has the row numbers). None: no filter. keep: one bool per chunk
        (pf_decode_row_group_dict): a chunk that is dictionary-encoded throughout comes back as indices + dictionary
        (fetch, materialize), any other as ever; not together with windows or predicates (ValueError)."""
        if keep is not None and (windows is not None or predicates is not None):
            raise ValueError("keep= takes no windows and no predicates")
        if keep is not None and len(keep) != len(descs):
            raise ValueError("one keep flag per chunk")
        arr = descs if isinstance(descs, C.Array) else (ChunkDesc * max(1, len(descs)))(*descs)
        self._keep = arr
        if keep is not None:
            flags = (C.c_uint8 * max(1, len(keep)))(*[1 if k else 0 for k in keep])
            check(lib().pf_decode_row_group_dict(self.h, arr, len(descs), flags, C.c_void_p(buf_ptr), nbytes, 1 if on_device else 0),
                  self.h, "pf_decode_row_group_dict")
        elif predicates is not None:
            if windows is not None and len(windows) != len(descs):
                raise ValueError("one window per chunk")
            win = None if windows is None else (RowWindow * max(1, len(windows)))(*[RowWindow(int(s), int(t)) for s, t in windows])
            preds, _alive = _pack_predicates(predicates)
            check(lib().pf_decode_row_group_filter(self.h, arr, len(descs), win, preds, len(predicates), C.c_void_p(buf_ptr), nbytes,
                                                   1 if on_device else 0), self.h, "pf_decode_row_group_filter")
        elif windows is None:
            check(lib().pf_decode_row_group(self.h, arr, len(descs), C.c_void_p(buf_ptr), nbytes, 1 if on_device else 0),
                  self.h, "pf_decode_row_group")
        else:
            if len(windows) != len(descs):
                raise ValueError("one window per chunk")
            win = (RowWindow * max(1, len(windows)))(*[RowWindow(int(s), int(t)) for s, t in windows])
            check(lib().pf_decode_row_group_rows(self.h, arr, len(descs), win, C.c_void_p(buf_ptr), nbytes,
                                                 1 if on_device else 0), self.h, "pf_decode_row_group_rows")
        self.n_chunks = len(descs)

    def decode_kept(self, descs, buf_ptr, nbytes, on_device=False, keep=None, windows=None, predicates=None):
        """decode() with keep flags that go together with windows and predicates (pf_decode_row_group_dict_filter): a
        chunk that is dictionary-encoded throughout comes back as the indices of the window's / the selection's rows +
        its whole dictionary (fetch, materialize); a predicate on such a chunk is matched once per dictionary entry.
        keep=None: decode(windows=, predicates=); no windows and no predicates: decode(keep=). info, dict_info, fetch,
        selection and materialize work on the result; fetch_batch only after a decode without windows and predicates."""
        n = len(descs)
        for name, v in (("keep flag", keep), ("window", windows)):
            if v is not None and len(v) != n:
                raise ValueError(f"one {name} per chunk")
        arr = descs if isinstance(descs, C.Array) else (ChunkDesc * max(1, n))(*descs)
        self._keep = arr
        flags = None if keep is None else (C.c_uint8 * max(1, n))(*[1 if k else 0 for k in keep])
        win = None if windows is None else (RowWindow * max(1, n))(*[RowWindow(int(s), int(t)) for s, t in windows])
        preds, _alive = _pack_predicates(predicates or [])
        check(lib().pf_decode_row_group_dict_filter(self.h, arr, n, flags, win, preds if predicates else None, len(predicates or []),
                                                    C.c_void_p(buf_ptr), nbytes, 1 if on_device else 0), self.h,
              "pf_decode_row_group_dict_filter")
        self.n_chunks = n

    def selection(self):
        """(rows_in, the selected row numbers as np.int32, ascending, counted from the window's first row) of the last
        filtered decode, after wait()."""
        si = self.selection_info()
        rows = np.zeros(si.rows_selected, np.int32)
        check(lib().pf_copy_selection(self.h, rows.ctypes.data if rows.size else None, rows.nbytes), self.h, "pf_copy_selection")
        return si.rows_in, rows

    def selection_info(self):
        si = SelectionInfo()
        check(lib().pf_selection_info_get(self.h, C.byref(si)), self.h, "pf_selection_info_get")
        return si

    def filter_ms(self):
        """Time of the filter kernels of the last decode (HIP events, ms; 0 without predicates or timing)."""
        ms = C.c_float()
        check(lib().pf_debug_filter(self.h, C.byref(ms)), self.h, "pf_debug_filter")
        return ms.value

    def window_ms(self):
        """Time of the window kernels of the last decode (HIP events, ms; 0 without windows or timing)."""
        return self._debug_window()[0]

    def chars_reruns(self):
        """How often the last decode's wait ran the batch again because the chars arena overflowed (0 or 1)."""
        return self._debug_window()[1]

    def _debug_window(self):
        ms, reruns = C.c_float(), C.c_int()
        check(lib().pf_debug_window(self.h, C.byref(ms), C.byref(reruns)), self.h, "pf_debug_window")
        return ms.value, reruns.value

    def wait(self):
        return lib().pf_wait(self.h)

    def error(self):
        return (lib().pf_last_error(self.h) or b"").decode(errors="replace")

    def info(self, i):
        ci = ColumnInfo()
        check(lib().pf_column_info_get(self.h, i, C.byref(ci)), self.h, "pf_column_info_get")
        return ci

    def dict_info(self, i):
        """pf_dict_info of chunk i of the last decode, after wait(): .kept is 0 unless the chunk's dictionary was kept."""
        di = DictInfo()
        check(lib().pf_dict_info_get(self.h, i, C.byref(di)), self.h, "pf_dict_info_get")
        return di

    def snappy_decompress(self, data: bytes, cap=None):
        """Raw Snappy buffer -> bytes on the GPU (K1 kernels). Returns (bytes, used_fallback)."""
        L = lib()
        src = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
        out_len = C.c_size_t()
        cap = cap if cap is not None else max(1, 64 * len(data) + 64)
        dst = np.zeros(cap, dtype=np.uint8)
        rc = L.pf_snappy_decompress(self.h, src.ctypes.data, len(data), dst.ctypes.data, cap, C.byref(out_len))
        if rc != 0:
            return rc, None
        return dst[:out_len.value].tobytes(), L.pf_snappy_last_fallback(self.h)

    def zstd_decompress(self, data: bytes, size: int):
        """ZSTD frames -> bytes on the GPU (k_zstd). size: the uncompressed length, as a page header
        states it. Returns the bytes, or a negative status: -2 when the frames are damaged or do not
        produce exactly size bytes."""
        src = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
        out_len = C.c_size_t()
        dst = np.zeros(max(1, size), dtype=np.uint8)
        rc = lib().pf_zstd_decompress(self.h, src.ctypes.data, len(data), dst.ctypes.data, size, C.byref(out_len))
        if rc != 0:
            return rc
        return dst[:size].tobytes() if out_len.value == size else -2

    def lz4_decompress(self, data: bytes, size: int):
        """One raw LZ4 block (codec LZ4_RAW) -> bytes on the GPU (k_lz4). size: the uncompressed length, as a
        page header states it. Returns the bytes, or a negative status: -2 when the block is damaged or
        does not produce exactly size bytes."""
        src = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
        out_len = C.c_size_t()
        dst = np.zeros(max(1, size), dtype=np.uint8)
        rc = lib().pf_lz4_decompress(self.h, src.ctypes.data, len(data), dst.ctypes.data, size, C.byref(out_len))
        if rc != 0:
            return rc
        return dst[:size].tobytes() if out_len.value == size else -2

    def zstd_compress(self, data: bytes, cap=None):
        """bytes -> one ZSTD frame, compressed on the GPU (k_zstd_compress). Returns the frame, or a negative
        status (-6: cap is too small). cap: the destination's size (default: what always suffices)."""
        src = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
        out_len = C.c_size_t()
        cap = cap if cap is not None else 12 + len(data) + 3 * (len(data) // 8192 + 1)
        dst = np.zeros(max(1, cap), dtype=np.uint8)
        rc = lib().pf_zstd_compress(self.h, src.ctypes.data, len(data), dst.ctypes.data, cap, C.byref(out_len))
        if rc != 0:
            return rc
        return dst[:out_len.value].tobytes()

    def scan_pages(self, data, chunks, verify_crc=False, page_cap=4096):
        """GPU page-header scan (pf_scan_pages) of column chunks in one host buffer.
        chunks: [(chunk_offset, chunk_size, num_values)]. Returns (rc, [(status, err_page, crc_pages,
        [page dicts])] per chunk)."""
        L = lib()
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        n = len(chunks)
        sc = (ScanChunk * max(n, 1))()
        for i, (off, size, nv) in enumerate(chunks):
            sc[i] = ScanChunk(off, size, nv, i * page_cap, page_cap)
        pages = (PageDesc * max(1, n * page_cap))()
        res = (ScanResult * max(n, 1))()
        rc = L.pf_scan_pages(self.h, sc, n, buf.ctypes.data, len(data), 0, int(verify_crc), pages, res)
        out = []
        for i in range(n):
            r = res[i]
            pg = [{f: getattr(pages[i * page_cap + k], f) for f, _ in PageDesc._fields_} for k in range(r.n_pages)]
            out.append((r.status, r.err_page, r.crc_pages, pg))
        return rc, out

    def set_timing(self, on):
        check(lib().pf_ctx_set_timing(self.h, 1 if on else 0), self.h, "pf_ctx_set_timing")

    def timing(self):
        buf = (C.c_float * 16)()
        n = C.c_int()
        check(lib().pf_last_timing(self.h, buf, 16, C.byref(n)), self.h, "pf_last_timing")
        names = ["h2d", "snappy_parse", "snappy_exec", "dict", "delta", "levels", "count", "scan", "flat", "decode"]
        return dict(zip(names, list(buf)[:n.value]))

    def fetch_batch(self, chunk_types, pageable=False):
        """All chunks of the last decode with ONE D2H per output arena (pf_copy_batch_async), then
        per chunk the canonical arrays cut from the host copy (pf_column_info_host).
        chunk_types: [(physical_type, max_def, max_rep)] per chunk. pageable: an ordinary host array
        instead of a mapped pinned buffer (the library's SDMA copy path instead of its download kernel)."""
        L = lib()
        n = C.c_size_t()
        check(L.pf_batch_bytes(self.h, C.byref(n)), self.h, "pf_batch_bytes")
        if pageable:
            class _Host:   # (same interface as PinnedBuffer for the code below)
                def __init__(self, nbytes):
                    self.arr = np.zeros(nbytes + 256, np.uint8)
                    a = self.arr.ctypes.data
                    self.off = (-a) % 256
                    self.ptr = C.c_void_p(a + self.off)
                    self.nbytes = nbytes

                def array(self):
                    return self.arr[self.off:self.off + self.nbytes]

                def free(self):
                    self.arr = None
            buf = _Host(max(1, n.value))
        else:
            buf = PinnedBuffer(self.h, max(1, n.value))
        try:
            check(L.pf_copy_batch_async(self.h, buf.ptr, buf.nbytes), self.h, "pf_copy_batch_async")
            check(L.pf_sync(self.h), self.h, "pf_sync")
            host = buf.array()
            base = buf.ptr.value
            out = []
            for i, (ptype, max_def, max_rep) in enumerate(chunk_types):
                ci = ColumnInfo()
                check(L.pf_column_info_host(self.h, i, buf.ptr, C.byref(ci)), self.h, "pf_column_info_host")
                g = {"status": ci.status, "num_entries": ci.num_entries, "num_slots": ci.num_slots,
                     "num_values": ci.num_values, "num_rows": ci.num_rows, "num_chars": ci.num_chars, "width": ci.width}
                if ci.status == 0:
                    ns, nr, ne = ci.num_slots, ci.num_rows, ci.num_entries

                    def cut(ptr, nbytes, dtype=np.uint8):
                        if not ptr:
                            raise AssertionError("array missing from the batch copy")
                        o = ptr - base
                        return host[o:o + nbytes].copy().view(dtype)
                    di = DictInfo()
                    check(L.pf_dict_info_host(self.h, i, buf.ptr, C.byref(di)), self.h, "pf_dict_info_host")
                    if di.kept:
                        g["indices"] = (cut(ci.d_values, ns * ci.width, INDEX_DTYPES[ci.width]) if ns
                                        else np.zeros(0, INDEX_DTYPES[ci.width]))
                        d = {"n_entries": di.n_entries, "width": di.width}
                        if di.width:
                            dict_bytes = di.n_entries * di.width
                            d["values"] = cut(di.d_values, dict_bytes) if dict_bytes else np.zeros(0, np.uint8)
                        else:
                            d["offsets"] = cut(di.d_offsets, 4 * (di.n_entries + 1), np.int32)
                            d["chars"] = cut(di.d_chars, di.num_chars) if di.num_chars else np.zeros(0, np.uint8)
                        g["dictionary"] = d
                    elif ptype == 6:
                        g["offsets"] = cut(ci.d_offsets, 4 * (ns + 1), np.int32)
                        g["chars"] = cut(ci.d_chars, ci.num_chars) if ci.num_chars else np.zeros(0, np.uint8)
                    else:
                        g["values"] = cut(ci.d_values, ns * ci.width) if ns * ci.width else np.zeros(0, np.uint8)
                    if max_def > 0:
                        g["validity"] = cut(ci.d_validity, (ns + 7) // 8)
                    if max_rep == 1:
                        g["list_offsets"] = cut(ci.d_list_offsets, 4 * (nr + 1), np.int32)
                        g["list_validity"] = cut(ci.d_list_validity, (nr + 7) // 8)
                    if max_rep > 0:
                        g["def_levels"] = cut(ci.d_def_levels, ne)
                        g["rep_levels"] = cut(ci.d_rep_levels, ne)
                out.append(g)
            return out
        finally:
            buf.free()

    def fetch(self, i, physical_type, max_def, max_rep):
        """Copy chunk i's decoded arrays to host numpy (canonical layout)."""
        ci = self.info(i)
        out = {"status": ci.status, "num_entries": ci.num_entries, "num_slots": ci.num_slots,
               "num_values": ci.num_values, "num_rows": ci.num_rows, "num_chars": ci.num_chars, "width": ci.width}
        if ci.status != 0:
            return out
        ns, nr, ne = ci.num_slots, ci.num_rows, ci.num_entries
        arrs = {}
        o = ColumnOut()

        def want(name, n, dtype=np.uint8):
            a = np.zeros(max(n, 0), dtype=dtype)
            arrs[name] = a
            setattr(o, name, a.ctypes.data if a.size else None)
            setattr(o, name + "_cap", a.nbytes)

        di = self.dict_info(i)
        if di.kept:   # indices (in `values`) + the dictionary's own arrays
            want("values", ns, INDEX_DTYPES[ci.width])
            d, do = {"n_entries": di.n_entries, "width": di.width}, ColumnOut()

            def dwant(name, n, dtype=np.uint8):
                a = np.zeros(max(n, 0), dtype=dtype)
                d[name] = a
                setattr(do, name, a.ctypes.data if a.size else None)
                setattr(do, name + "_cap", a.nbytes)
            if di.width:
                dwant("values", di.n_entries * di.width)
            else:
                dwant("offsets", di.n_entries + 1, np.int32)
                dwant("chars", di.num_chars)
            check(lib().pf_copy_dictionary(self.h, i, C.byref(do)), self.h, "pf_copy_dictionary")
            if max_def > 0:
                want("validity", (ns + 7) // 8)
            check(lib().pf_copy_column(self.h, i, C.byref(o)), self.h, "pf_copy_column")
            arrs["indices"] = arrs.pop("values")
            out.update(arrs)
            out["dictionary"] = d
            return out
        if physical_type == 6:
            want("offsets", ns + 1, np.int32)
            want("chars", ci.num_chars)
        else:
            want("values", ns * ci.width)
        if max_def > 0:
            want("validity", (ns + 7) // 8)
        if max_rep == 1:
            want("list_offsets", nr + 1, np.int32)
            want("list_validity", (nr + 7) // 8)
        if max_rep > 0:
            want("def_levels", ne)
            want("rep_levels", ne)
        check(lib().pf_copy_column(self.h, i, C.byref(o)), self.h, "pf_copy_column")
        out.update(arrs)
        return out


INDEX_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def materialize(arrays, physical_type):
    """A kept chunk (fetch / fetch_batch: "indices" + "dictionary") expanded on the host into the canonical arrays of
    include/pfloor.h: values[s] = dictionary[indices[s]] where the validity bit is set, zero bytes (a zero-length
    string) where it is not; BYTE_ARRAY offsets and chars are rebuilt in slot order. numpy only. Arrays of a chunk
    that was not kept are returned as they are."""
    if "indices" not in arrays:
        return arrays
    out = {k: v for k, v in arrays.items() if k not in ("indices", "dictionary")}
    d = arrays["dictionary"]
    idx = np.asarray(arrays["indices"]).astype(np.int64)
    ns = len(idx)
    v = arrays.get("validity")
    valid = np.unpackbits(np.asarray(v, np.uint8), bitorder="little")[:ns].astype(bool) if v is not None else np.ones(ns, bool)
    n_entries = int(d["n_entries"])
    if valid.any() and (n_entries == 0 or int(idx[valid].max()) >= n_entries):
        raise ValueError("materialize: an index outside the dictionary")
    if physical_type == 6:
        doffs = np.asarray(d["offsets"], np.int64)
        dchars = np.asarray(d["chars"], np.uint8)
        lens = np.zeros(ns, np.int64)
        lens[valid] = (doffs[1:] - doffs[:-1])[idx[valid]]
        offs = np.zeros(ns + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        if offs[-1] > 0x7fffffff:
            raise ValueError("materialize: more than 2^31 - 1 chars")
        starts = np.zeros(ns, np.int64)
        starts[valid] = doffs[:-1][idx[valid]]
        src = np.repeat(starts - offs[:-1], lens) + np.arange(int(offs[-1]), dtype=np.int64)
        out["offsets"] = offs.astype(np.int32)
        out["chars"] = dchars[src] if len(src) else np.zeros(0, np.uint8)
        out["num_chars"] = int(offs[-1])
        out["width"] = 0
    else:
        w = int(d["width"])
        dv = np.asarray(d["values"], np.uint8).reshape(n_entries, w)
        vals = np.zeros((ns, w), np.uint8)
        vals[valid] = dv[idx[valid]]
        out["values"] = vals.ravel()
        out["num_chars"] = 0
        out["width"] = w
    return out


def decode_file(path, row_groups=None, columns=None, device=0, decoder=None, rows=None, where=None, dictionaries=False):
    """Decode the selected chunks of a file on the GPU: {(rg, col): arrays}. One batch.
    rows=(lo, hi): rows [lo, hi) of ONE row group (row_groups names it; default 0), counted within it: only the
    pages its OffsetIndex selects are read and uploaded, and the arrays are cut to the rows on the GPU.
    where=[pfloor.predicate ...]: a conjunction, also over ONE row group (after rows, if given): the page index and the
    Bloom filters prune first (ParquetFile.prune_row_group), the predicates are evaluated on the GPU and the arrays
    hold the matching rows only. "_selection" = (rows_in, row numbers within the row group as np.int64), "_range" =
    the rows that were decoded, None when the row group was skipped (no chunk is returned then). A predicate column
    outside `columns` is decoded and not returned.
    dictionaries=True: every chunk that is dictionary-encoded throughout comes back as "indices" + "dictionary"
    (GpuDecoder.decode(keep=...); with rows= or where=, GpuDecoder.decode_kept: the indices of the window's or the
    selection's rows and the whole dictionary); materialize() expands one on the host."""
    with ParquetFile(path) as pf:
        rgs = list(range(pf.num_row_groups)) if row_groups is None else list(row_groups)
        cols = list(range(pf.num_columns)) if columns is None else list(columns)
        dec = decoder or GpuDecoder(device)
        try:
            if rows is not None or where is not None:
                rg = 0 if row_groups is None else rgs[0]
                if row_groups is not None and len(rgs) != 1:
                    raise ValueError("rows=(lo, hi) and where= read one row group")
                lo, hi = (0, pf.row_group_rows(rg)) if rows is None else (int(rows[0]), int(rows[1]))
                batch, preds = list(cols), None
                if where is not None:
                    from .predicate import bind, resolve
                    batch += [c for c in dict.fromkeys(resolve(pf.columns, p.column) for p in where) if c not in cols]
                    preds = bind(where, pf.columns, {c: i for i, c in enumerate(batch)})
                    span = pf.prune_row_group(rg, where, lo, hi)
                    if span is None:
                        return {"_status": 0, "_error": "", "_selection": (0, np.zeros(0, np.int64)), "_range": None}
                    lo, hi = span
                items, total, windows = pf.plan_rows(rg, batch, lo, hi)
                buf = dec.staging(total)
                pf.read_rows(items, buf.ptr.value)
                extra = {} if preds is None else {"predicates": preds}
                descs = [d for _c, d, _r, _o in items]
                if dictionaries:
                    dec.decode_kept(descs, buf.ptr.value, max(total, 1), keep=[True] * len(descs), windows=windows, **extra)
                else:
                    dec.decode(descs, buf.ptr.value, max(total, 1), windows=windows, **extra)
                rc = dec.wait()
                out = {}
                for i, col in enumerate(cols):
                    c = pf.columns[col]
                    out[(rg, col)] = dec.fetch(i, c.physical_type, c.max_def, c.max_rep)
                if where is not None:
                    rows_in, sel = dec.selection()
                    out["_selection"] = (rows_in, sel.astype(np.int64) + lo)
                    out["_range"] = (lo, hi)
                out["_status"] = rc
                out["_error"] = dec.error() if rc else ""
                return out
            items, total = pf.plan(rgs, cols)
            buf = dec.staging(total)
            descs = []
            for rg, col, s, n, off in items:
                if n:
                    pf.read_into(s, n, buf.ptr.value + off)
                descs.append(pf.chunk_desc(rg, col, off))
            extra = {"keep": [True] * len(descs)} if dictionaries else {}
            dec.decode(descs, buf.ptr.value, max(total, 1), **extra)
            rc = dec.wait()
            out = {}
            for i, (rg, col, *_r) in enumerate(items):
                c = pf.columns[col]
                out[(rg, col)] = dec.fetch(i, c.physical_type, c.max_def, c.max_rep)
            out["_status"] = rc
            out["_error"] = dec.error() if rc else ""
            return out
        finally:
            if decoder is None:
                dec.close()
