"""Host-side mirror of parquet-floor's read API over the HIP decoder.

Mirrors src/main/java/blue/strategic/parquet/ParquetReader.java (names, argument meaning,
call order, error behaviour), Hydrator.java and HydratorSupplier.java:
  * streamContent(file, hydratorSupplier[, columns]) -> a closeable row stream   (:47-61)
  * spliterator(...) / stream(reader) / readMetadata(file) / streamContentToStrings (:63-117)
  * columns filtered by path[0] in schema order                                  (:126-128)
  * per row: hydrator.start(); for each column in order: add(record, path[0], readValue);
    consume; a non-zero next repetition level raises "Unexpected repetition"      (:196-203)
  * readValue: def == maxDef -> typed value (BINARY/FLBA/INT96 through the column's
    stringifier), else None                                                      (:141-168)
  * any failure while iterating -> RuntimeError("Failed to read parquet") from the cause (:209-211)
  * trySplit() -> None, estimateSize() = total rows, characteristics ORDERED|NONNULL|DISTINCT
Decoding happens per row group on the GPU (one batch of the selected column chunks);
only the row assembly loop (a1) runs on the host, as the Java adapter would. With several
devices (`devices=[...]`) row groups are dealt round-robin to per-device contexts and decoded
ahead of the row loop (north_star: row groups sharded across the GPUs of a node, no collective);
rows still come out in file order, as the reference's single ORDERED stream delivers them
(ParquetReader.java:176-212, :225-227).
"""
import collections
import struct
import uuid as _uuid

import numpy as np

from .decoder import GpuDecoder, ParquetFile

ORDERED, DISTINCT, NONNULL = 0x00000010, 0x00000001, 0x00000100


class Hydrator:
    """Creates and hydrates a rich domain object from a Parquet row (Hydrator.java:6-28)."""

    def start(self):
        raise NotImplementedError

    def add(self, target, heading, value):
        raise NotImplementedError

    def finish(self, target):
        raise NotImplementedError


class HydratorSupplier:
    """Supplies a hydrator for the selected columns (HydratorSupplier.java:10-19)."""

    def __init__(self, fn):
        self._fn = fn

    def get(self, columns):
        return self._fn(columns)

    @staticmethod
    def constantly(hydrator):
        return HydratorSupplier(lambda columns: hydrator)


class IllegalStateException(Exception):
    pass


class IllegalArgumentException(Exception):
    pass


_HEX = "0123456789ABCDEF"
BINARY_INVALID = "<INVALID>"
# SchemaElement.converted_type ids / LogicalType union member ids (parquet-format)
CT_UTF8, CT_ENUM, CT_DECIMAL, CT_JSON, CT_BSON, CT_INTERVAL = 0, 4, 5, 19, 20, 21
LT_STRING, LT_ENUM, LT_DECIMAL, LT_JSON, LT_BSON, LT_UUID = 1, 4, 5, 12, 13, 14


def _default_stringify(b: bytes) -> str:
    """PrimitiveStringifier.DEFAULT_STRINGIFIER for a Binary: "0x" + upper-case hex."""
    return "0x" + "".join(_HEX[(x >> 4) & 15] + _HEX[x & 15] for x in b)


def _utf8_stringify(b: bytes) -> str:
    """UTF8_STRINGIFIER: Binary.toStringUsingUTF8 (malformed input -> U+FFFD; the replacement
    count for malformed sequences follows Python's decoder: parity unpinned)."""
    return bytes(b).decode("utf-8", errors="replace")


def java_big_decimal_str(unscaled: int, scale: int) -> str:
    """java.math.BigDecimal(BigInteger unscaled, int scale).toString(): plain notation when
    scale >= 0 and the adjusted exponent >= -6, otherwise scientific ("1E-7", "1.23E+5")."""
    neg = unscaled < 0
    coeff = str(-unscaled if neg else unscaled)
    adjusted = -scale + (len(coeff) - 1)
    if scale == 0:
        body = coeff
    elif scale > 0 and adjusted >= -6:
        pad = scale - len(coeff)
        body = "0." + "0" * pad + coeff if pad >= 0 else coeff[:-scale] + "." + coeff[-scale:]
    else:
        body = coeff[0] + ("." + coeff[1:] if len(coeff) > 1 else "")
        if adjusted != 0:
            body += "E" + ("+" if adjusted > 0 else "") + str(adjusted)
    return ("-" if neg else "") + body


def _decimal_stringifier(scale):
    """PrimitiveStringifier.createDecimalStringifier(scale) for a Binary: two's-complement
    big-endian unscaled value (new BigInteger(bytes)); empty -> NumberFormatException ->
    "<INVALID>"."""
    def f(b: bytes) -> str:
        if len(b) == 0:
            return BINARY_INVALID
        return java_big_decimal_str(int.from_bytes(bytes(b), "big", signed=True), scale)
    return f


def _interval_stringify(b: bytes) -> str:
    """INTERVAL_STRINGIFIER: 12 bytes = three little-endian unsigned 32-bit ints."""
    if len(b) != 12:
        return BINARY_INVALID
    m, d, ms = struct.unpack("<III", bytes(b))
    return f"interval({m} months, {d} days, {ms} millis)"


def _uuid_stringify(b: bytes) -> str:
    """UUID_STRINGIFIER: lower-case 8-4-4-4-12 hex of the 16 bytes."""
    return str(_uuid.UUID(bytes=bytes(b)))


def stringifier(col):
    """PrimitiveType.stringifier() for BINARY / FIXED_LEN_BYTE_ARRAY / INT96, restating upstream
    parquet-mr 1.12.2 (PrimitiveType.stringifier -> LogicalTypeAnnotation.valueStringifier, the
    annotation taken from LogicalType, else from the converted type):
      STRING / ENUM / JSON   -> UTF8_STRINGIFIER
      DECIMAL(scale)         -> createDecimalStringifier(scale)
      UUID (FLBA 16)         -> UUID_STRINGIFIER
      INTERVAL (FLBA 12)     -> INTERVAL_STRINGIFIER
      BSON / none (incl. INT96, unannotated BINARY / FLBA) -> DEFAULT_STRINGIFIER ("0x" + hex)
    Pinned by the reference's own test only for UTF8 (ParquetReadWriteTest.java:66-82); the other
    branches are parity unpinned (no parquet-mr in this image)."""
    lt, ct = col.logical_type, col.converted_type
    if lt in (LT_STRING, LT_ENUM, LT_JSON) or (lt == 0 and ct in (CT_UTF8, CT_ENUM, CT_JSON)):
        return _utf8_stringify
    if lt == LT_DECIMAL or (lt == 0 and ct == CT_DECIMAL):
        return _decimal_stringifier(getattr(col, "scale", 0))
    if lt == LT_UUID:
        return _uuid_stringify
    if lt == 0 and ct == CT_INTERVAL:
        return _interval_stringify
    return _default_stringify


_UNSET = object()


class _ColumnCursor:
    """ColumnReader over one decoded chunk: current definition/repetition level, value, consume(). Over a kept chunk
    ("indices" + "dictionary", GpuDecoder.decode(keep=...)) every dictionary entry is converted once, when a row first
    uses it, and a row costs one list lookup."""

    def __init__(self, col, arrays):
        self.col = col
        self.a = arrays
        self.e = 0                    # current level entry
        self.slot = 0                 # slot index of the current entry (if it is a slot)
        nested = col.max_rep > 0
        self.n = arrays["num_entries"]
        if nested:
            self.defs = arrays["def_levels"]
            self.reps = arrays["rep_levels"]
        else:
            self.defs = None
            v = arrays.get("validity")
            self.valid = (np.unpackbits(v, bitorder="little")[:self.n].astype(bool) if v is not None
                          else np.ones(self.n, bool))
        pt = col.physical_type
        self.indices = arrays.get("indices")
        if self.indices is not None:
            d = arrays["dictionary"]
            self.dict_n, self.dict_width = int(d["n_entries"]), int(d["width"])
            if pt == 6:
                self.dict_offsets = d["offsets"]
                self.dict_chars = d["chars"].tobytes()
            else:
                self.dict_values = d["values"]
            self.converted = [_UNSET] * self.dict_n
        elif pt in (6,):
            self.offsets = arrays["offsets"]
            self.chars = arrays["chars"].tobytes()
        else:
            self.values = arrays["values"]
        fmt = {1: "<i", 2: "<q", 4: "<f", 5: "<d"}.get(pt)
        self.fmt = fmt
        self.strf = stringifier(col) if pt in (3, 6, 7) else None

    def definition_level(self):
        if self.defs is not None:
            return int(self.defs[self.e])
        return self.col.max_def if self.valid[self.e] else self.col.max_def - 1

    def repetition_level(self):
        if self.defs is None or self.e >= self.n:
            return 0
        return int(self.reps[self.e])

    def _raw(self, s):
        pt = self.col.physical_type
        if pt == 6:
            return self.chars[self.offsets[s]:self.offsets[s + 1]]
        w = self.a["width"]
        return self.values[s * w:(s + 1) * w].tobytes()

    def _dict_raw(self, i):
        if self.col.physical_type == 6:
            return self.dict_chars[self.dict_offsets[i]:self.dict_offsets[i + 1]]
        w = self.dict_width
        return self.dict_values[i * w:(i + 1) * w].tobytes()

    def _convert(self, raw):
        pt = self.col.physical_type
        if pt in (6, 7, 3):
            return self.strf(raw)
        if pt == 0:
            return bool(raw[0])
        if self.fmt:
            return struct.unpack(self.fmt, raw)[0]
        raise IllegalArgumentException(f"Unsupported type: {self.col}")

    def read_value(self):
        """ParquetReader.readValue (ParquetReader.java:141-168)."""
        col = self.col
        if self.definition_level() == col.max_def:
            if self.indices is not None:
                i = int(self.indices[self.slot])
                v = self.converted[i]
                if v is _UNSET:
                    v = self.converted[i] = self._convert(self._dict_raw(i))
                return v
            return self._convert(self._raw(self.slot))
        return None

    def consume(self):
        is_slot = self.defs is None or self.defs[self.e] >= self.col.repeated_def
        if is_slot:
            self.slot += 1
        self.e += 1


class RowGroupPipeline:
    """Row groups decoded ahead of the consumer on one or more devices, delivered in file order.

    Row group g goes to device slot g % G (G = len(devices)); each device has `depth` contexts
    on one HIP stream (pf_ctx_create_shared), so up to G * depth row groups are in flight: the
    chunk bytes of g are read into its context's pinned staging buffer and the decode enqueued
    (pf_decode_row_group is asynchronous); `take(g)` waits for g (pf_wait) and copies its columns
    to the host. A context is reused only after its previous row group was taken, so its staging
    buffer and output arenas are never overwritten while in use.

    windows: per entry of row_groups None (the whole row group, the path above) or (lo, hi), rows within that row
    group: only the pages its OffsetIndex selects are read and uploaded (ParquetFile.plan_rows) and the columns are cut
    to the rows on the GPU before they cross the link (GpuDecoder.decode(windows=...)).

    where: a conjunction of pfloor.predicate predicates. Every row group then goes through plan_rows over its window (or
    all of it) and GpuDecoder.decode(windows=, predicates=): the predicates are evaluated on the GPU and the columns come
    back compacted to the matching rows. A predicate column that is not among `columns` is decoded and not returned.
    `selections[i]` = (rows_in, rows_selected) of row_groups[i] once taken; `bytes_read` counts the chunk bytes read."""

    def __init__(self, reader, columns, row_groups, devices=(0,), depth=2, windows=None, where=None, dictionaries=False):
        self.dictionaries = bool(dictionaries)   # every row group keeps its eligible chunks' dictionaries
        if not devices:
            raise ValueError("devices must not be empty")
        self.reader = reader
        self.columns = columns
        self.row_groups = list(row_groups)
        self.windows = list(windows) if windows is not None else [None] * len(self.row_groups)
        if len(self.windows) != len(self.row_groups):
            raise ValueError("one window (or None) per row group")
        self.where = list(where) if where else None
        self.selections = {}
        self.bytes_read = 0
        self._batch = [c.index for c in columns]
        self._preds = None
        if self.where:
            from .predicate import bind, resolve
            extra = dict.fromkeys(resolve(reader.columns, p.column) for p in self.where)
            self._batch += [c for c in extra if c not in self._batch]
            self._preds = bind(self.where, reader.columns, {c: i for i, c in enumerate(self._batch)})
        self.depth = max(1, int(depth))
        self.decs = []   # [device slot][k]
        self.inflight = collections.OrderedDict()   # position in row_groups -> decoder, or the enqueue error
        self.next_enqueue = 0
        try:
            for d in devices:
                slot = []
                self.decs.append(slot)   # registered before its contexts exist: close() frees a partial slot
                slot.append(GpuDecoder(d))
                for _ in range(self.depth - 1):
                    slot.append(GpuDecoder(share=slot[0]))
        except Exception:
            self.close()   # the contexts created so far; the device error propagates
            raise

    def _decoder(self, i):
        g = len(self.decs)
        return self.decs[i % g][(i // g) % self.depth]

    def _enqueue(self, i):
        rg = self.row_groups[i]
        dec = self._decoder(i)
        try:
            idx = [c.index for c in self.columns]
            if self.windows[i] is not None or self._preds is not None:
                lo, hi = self.windows[i] if self.windows[i] is not None else (0, self.reader.row_group_rows(rg))
                items, total, wins = self.reader.plan_rows(rg, self._batch, lo, hi)
                buf = dec.staging(total)
                self.bytes_read += self.reader.read_rows(items, buf.ptr.value)
                extra = {} if self._preds is None else {"predicates": self._preds}
                descs = [d for _c, d, _r, _o in items]
                if self.dictionaries:   # windowed and filtered row groups keep their dictionaries too
                    dec.decode_kept(descs, buf.ptr.value, max(total, 1), keep=[True] * len(descs), windows=wins, **extra)
                else:
                    dec.decode(descs, buf.ptr.value, max(total, 1), windows=wins, **extra)
                self.inflight[i] = dec
                return
            items, total = self.reader.plan([rg], idx)
            buf = dec.staging(total)
            descs = []
            for _rg, col, s, n, off in items:
                if n:
                    self.reader.read_into(s, n, buf.ptr.value + off)
                descs.append(self.reader.chunk_desc(rg, col, off))
            extra = {"keep": [True] * len(descs)} if self.dictionaries else {}
            dec.decode(descs, buf.ptr.value, max(total, 1), **extra)
            self.inflight[i] = dec
        except Exception as e:   # surfaces when row group i is reached, as readNextRowGroup would raise it
            self.inflight[i] = e

    def take(self, i):
        """Decoded columns of row_groups[i] (list of per-column array dicts); i must be taken in order."""
        window = len(self.decs) * self.depth
        while self.next_enqueue < len(self.row_groups) and self.next_enqueue < i + window:
            self._enqueue(self.next_enqueue)
            self.next_enqueue += 1
        dec = self.inflight.pop(i)
        if isinstance(dec, Exception):
            raise dec
        rc = dec.wait()
        if rc != 0:
            raise RuntimeError(dec.error())
        if self._preds is not None:
            si = dec.selection_info()
            self.selections[i] = (si.rows_in, si.rows_selected)
        return [dec.fetch(k, c.physical_type, c.max_def, c.max_rep) for k, c in enumerate(self.columns)]

    def close(self):
        for dec in self.inflight.values():
            if not isinstance(dec, Exception):
                dec.wait()
        self.inflight.clear()
        for slot in self.decs:
            for dec in reversed(slot):   # shared contexts before the stream's owner
                dec.close()
        self.decs = []


class ParquetReader:
    """Spliterator-like reader (ParquetReader.java:34-260)."""

    # --- static factories (ParquetReader.java:47-84) ---
    @staticmethod
    def streamContent(file, hydratorSupplier, columns=None, device=0, devices=None, rows=None, where=None, dictionaries=False):
        return ParquetReader.stream(ParquetReader.spliterator(file, hydratorSupplier, columns, device, devices, rows, where,
                                                              dictionaries))

    @staticmethod
    def spliterator(file, hydratorSupplier, columns=None, device=0, devices=None, rows=None, where=None, dictionaries=False):
        """devices: GPUs to deal the row groups over (default [device]); rows stay in file order.
        rows=(lo, hi): only rows lo .. hi-1 of the file (0 <= lo <= hi <= num_rows): row groups wholly outside are
        neither read nor decoded, the two edge row groups are read by page and cut on the GPU, inner ones as ever.
        where=[pfloor.predicate ...]: only the rows that match the conjunction. After `rows`, the page index and the
        Bloom filters prune every row group (ParquetFile.prune_row_group: a skipped one is neither read nor decoded);
        the rest are read by page over what remains, filtered on the GPU and compacted there, so only matching rows
        cross the link. A predicate column outside `columns` is decoded and never passed to the Hydrator. A projected
        or predicate column with repetition is an IllegalArgumentException. `filter_stats` counts what happened.
        dictionaries=True: every row group, windowed and filtered ones included, keeps the dictionary of every chunk
        that is dictionary-encoded throughout: indices and dictionary cross the link instead of expanded values, and
        each dictionary entry is converted once per row group. Rows, call order and exceptions are those of the default."""
        column_set = frozenset() if columns is None else frozenset(columns)
        return ParquetReader(str(file), column_set, hydratorSupplier, device, devices, rows, where, dictionaries)

    @staticmethod
    def stream(reader):
        return _RowStream(reader)

    @staticmethod
    def streamContentToStrings(file, device=0):
        """ParquetReader.java:86-107, including its behaviour: `pos` is shared across rows, so a
        second row indexes past the array, and a null value fails on value.toString()."""
        def supplier(columns):
            pos = [0]

            class _H(Hydrator):
                def start(self):
                    return [None] * len(columns)

                def add(self, target, heading, value):
                    i = pos[0]
                    pos[0] += 1
                    if i >= len(target):
                        raise IndexError(f"Index {i} out of bounds for length {len(target)}")
                    if value is None:
                        raise AttributeError("NullPointerException: value.toString()")
                    target[i] = f"{heading}={value}"
                    return target

                def finish(self, target):
                    return target
            return _H()
        return ParquetReader.stream(ParquetReader.spliterator(file, HydratorSupplier(supplier), None, device))

    @staticmethod
    def readMetadata(file):
        """Footer only (ParquetReader.java:109-117): a ParquetFile with schema + row groups."""
        f = ParquetFile(str(file))
        return f

    # --- instance (ParquetReader.java:119-131) ---
    def __init__(self, path, column_names, hydrator_supplier, device=0, devices=None, rows=None, where=None, dictionaries=False):
        self._dictionaries = bool(dictionaries)
        try:
            self.reader = ParquetFile(path)
        except Exception as e:
            raise IOError(str(e)) from e
        self.columns = [c for c in self.reader.columns if not column_names or c.path[0] in column_names]
        self.hydrator = hydrator_supplier.get(self.columns)
        self.finished = False
        self.current_rg = -1
        self.current_row_group_size = -1
        self.current_row_index = -1
        self.cursors = None
        self._devices = list(devices) if devices else [device]
        self._pipe = None
        # the row groups to visit, in order: (row group, None = all of it | (lo, hi) within it)
        if rows is None:
            self._visits = [(rg, None) for rg in range(self.reader.num_row_groups)]
        else:
            lo, hi = int(rows[0]), int(rows[1])
            if not 0 <= lo <= hi <= self.reader.num_rows:
                self.reader.close()
                raise IllegalArgumentException(f"rows {rows} outside [0, {self.reader.num_rows}]")
            self._visits = []
            start = 0
            for rg in range(self.reader.num_row_groups):
                n = self.reader.row_group_rows(rg)
                a, b = max(lo - start, 0), min(hi - start, n)
                if a < b:
                    self._visits.append((rg, None if (a, b) == (0, n) else (a, b)))
                start += n
        self._where = list(where) if where else None
        self.filter_stats = {"row_groups_skipped_index": 0, "row_groups_skipped_bloom": 0, "bytes_read": 0, "rows_decoded": 0,
                             "rows_selected": 0}
        if self._where:
            try:
                self._prune_visits()
            except Exception:
                self.reader.close()
                raise
        self._pos = -1

    def _prune_visits(self):
        """where=: refuse repetition, then narrow or drop every visit by the page index and the Bloom filters."""
        from .predicate import resolve
        try:
            pred_cols = [self.reader.columns[resolve(self.reader.columns, p.column)] for p in self._where]
        except ValueError as e:
            raise IllegalArgumentException(str(e)) from e
        for c in list(self.columns) + pred_cols:
            if c.max_rep > 0:
                raise IllegalArgumentException(f"where=: column {'.'.join(c.path)} has repetition")
        kept = []
        for rg, win in self._visits:
            n = self.reader.row_group_rows(rg)
            lo, hi = win if win is not None else (0, n)
            try:
                span, why = self.reader._prune(rg, self._where, lo, hi)
            except ValueError as e:
                raise IllegalArgumentException(str(e)) from e
            if span is None:
                self.filter_stats["row_groups_skipped_" + why] += 1
            else:
                kept.append((rg, span))
        self._visits = kept

    def _read_next_row_group(self):
        self._pos += 1
        if self._pos >= len(self._visits):
            self.current_rg = self.reader.num_row_groups
            return False
        rg, win = self._visits[self._pos]
        self.current_rg = rg
        if self.reader.row_group_rows(rg) == 0:
            # parquet-mr 1.12.2 ParquetFileReader.readNextRowGroup [upstream, restated]
            raise RuntimeError("Illegal row group of 0 rows")
        if self._pipe is None:
            self._pipe = RowGroupPipeline(self.reader, self.columns, [v[0] for v in self._visits], self._devices,
                                          windows=[v[1] for v in self._visits], where=self._where,
                                          dictionaries=self._dictionaries)
        arrays = self._pipe.take(self._pos)
        self.cursors = [_ColumnCursor(c, a) for c, a in zip(self.columns, arrays)]
        self.current_row_group_size = self.reader.row_group_rows(rg) if win is None else win[1] - win[0]
        self.current_row_index = 0
        if self._where:
            rows_in, selected = self._pipe.selections.pop(self._pos)
            self.filter_stats["rows_decoded"] += rows_in
            self.filter_stats["rows_selected"] += selected
            self.filter_stats["bytes_read"] = self._pipe.bytes_read + getattr(self.reader, "bloom_bytes_read", 0)
            self.current_row_group_size = selected
            if selected == 0:   # nothing of this row group matches: on to the next
                return self._read_next_row_group()
        return True

    def tryAdvance(self, action):
        """ParquetReader.tryAdvance (ParquetReader.java:176-212)."""
        try:
            if self.finished:
                return False
            if self.current_row_index == self.current_row_group_size:
                if not self._read_next_row_group():
                    self.finished = True
                    return False
            record = self.hydrator.start()
            for cur in self.cursors:
                record = self.hydrator.add(record, cur.col.path[0], cur.read_value())
                cur.consume()
                if cur.repetition_level() != 0:
                    raise IllegalStateException("Unexpected repetition")
            action(self.hydrator.finish(record))
            self.current_row_index += 1
            return True
        except Exception as e:
            raise RuntimeError("Failed to read parquet") from e

    def trySplit(self):
        return None

    def estimateSize(self):
        return self.reader.num_rows

    def characteristics(self):
        return ORDERED | NONNULL | DISTINCT

    def metaData(self):
        return self.reader

    def close(self):
        if self._pipe is not None:
            self._pipe.close()
            self._pipe = None
        self.reader.close()


class _RowStream:
    """Sequential stream over tryAdvance; closing it closes the reader (ParquetReader.java:80-84)."""

    def __init__(self, reader):
        self.reader = reader

    def __iter__(self):
        out = []
        while True:
            out.clear()
            if not self.reader.tryAdvance(out.append):
                return
            yield out[0]

    def collect(self):
        return list(iter(self))

    def close(self):
        try:
            self.reader.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
