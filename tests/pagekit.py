"""Test-only Parquet page and footer assembler (pure Python + numpy; TEST INFRASTRUCTURE ONLY).

Builds column chunks page by page in the layouts parquet-mr 1.12.2 reads but no other writer here
emits (id width 0 and non-minimal id widths, BIT_PACKED levels, PLAIN_DICTIONARY pages, v2 pages
with is_compressed = false inside a Snappy chunk, FLBA of any width, ...) and wraps them in a Thrift
compact FileMetaData. Neither the product's writer (pf_write.cpp) nor its encoders are involved.
Every builder also returns the expected decoded arrays in the canonical layout of include/pfloor.h
(values with zeroed null slots, validity, offsets, chars, list offsets, levels), computed from the
inputs and never by decoding.

Values travel as `vals`: a uint8 array [n_present, width] for fixed-width types (BOOLEAN: width 1,
bytes 0/1), a list of bytes objects for BYTE_ARRAY."""
import numpy as np

BOOLEAN, INT32, INT64, INT96, FLOAT, DOUBLE, BYTE_ARRAY, FLBA = range(8)
PLAIN, PLAIN_DICTIONARY, RLE, BIT_PACKED, DELTA_BINARY_PACKED, DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY, \
    RLE_DICTIONARY, BYTE_STREAM_SPLIT = 0, 2, 3, 4, 5, 6, 7, 8, 9
UNCOMPRESSED, SNAPPY = 0, 1
STYLES = ("mr", "rle", "mixed")


def width_of(ptype, type_length=0):
    return {BOOLEAN: 1, INT32: 4, INT64: 8, INT96: 12, FLOAT: 4, DOUBLE: 8, BYTE_ARRAY: 0, FLBA: type_length}[ptype]


# ---------------------------------------------------------------- varints, DELTA_BINARY_PACKED
def _uvarint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _zz(v):
    return (v << 1) ^ (v >> 63)


def _wrap(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _dbp(values, block, nmini, junk_tail=False, bad_block=None, bits=64):
    """parquet-mr's DeltaBinaryPackingValuesWriter[ForLong] layout; bits=32 is the INT32 writer:
    deltas and (delta - min_delta) wrap mod 2^32, as its int arithmetic does."""
    vpm = block // nmini
    out = bytearray(_uvarint(block) + _uvarint(nmini) + _uvarint(len(values)) + _uvarint(_zz(int(values[0])) & (2**64 - 1)))
    deltas = [_wrap(int(values[i]) - int(values[i - 1]), bits) for i in range(1, len(values))]
    for b0 in range(0, len(deltas), block):
        d = deltas[b0:b0 + block]
        mn = min(d)
        out += _uvarint(_zz(mn) & (2**64 - 1))
        rel = [(x - mn) & ((1 << bits) - 1) for x in d]
        widths, data = [], bytearray()
        for m in range(nmini):
            chunk = rel[m * vpm:(m + 1) * vpm]
            w = max((x.bit_length() for x in chunk), default=0)
            if not chunk:
                widths.append(200 if junk_tail else 0)   # unconsumed miniblock: its width is never checked
                continue
            if bad_block is not None and b0 // block == bad_block and m == 0:
                w = bits + 1                                # a width no reader of this type accepts
            widths.append(w)
            if w > bits:
                data += bytes((vpm * 64 + 7) // 8)
                continue
            chunk = chunk + [0] * (vpm - len(chunk))
            acc = 0
            for i, x in enumerate(chunk):
                acc |= x << (i * w)
            data += acc.to_bytes((vpm * w + 7) // 8, "little")
        out += bytes(widths) + data
    return bytes(out)


def dbp(values, bits=64, block=128, nmini=4):
    """DELTA_BINARY_PACKED stream of `values`; an empty list is a header with a zero count."""
    if len(values) == 0:
        return _uvarint(block) + _uvarint(nmini) + _uvarint(0) + _uvarint(0)
    return _dbp([int(v) for v in values], block, nmini, bits=bits)


# ---------------------------------------------------------------- bit packing, hybrid, levels
def _pack_le(v, bw):
    """LSB-first bit packing of v (len a multiple of 8) at bw bits each."""
    if bw == 0 or len(v) == 0:
        return b""
    v = np.asarray(v, np.uint64)
    bits = ((v[:, None] >> np.arange(bw, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits.ravel(), bitorder="little").tobytes()


def _packed_runs(v, bw, max_groups=63):
    """Bit-packed runs over all of v, the last group zero-padded to 8 values."""
    out = bytearray()
    n = len(v)
    pad = (-n) % 8
    if pad:
        v = np.concatenate([np.asarray(v, np.uint64), np.zeros(pad, np.uint64)])
    for i in range(0, len(v), 8 * max_groups):
        part = v[i:i + 8 * max_groups]
        out += _uvarint(((len(part) // 8) << 1) | 1) + _pack_le(part, bw)
    return bytes(out)


def _run_left(v):
    """left[i] = how many entries from i on (i included) repeat v[i]."""
    n = len(v)
    if n == 0:
        return np.zeros(0, np.int64)
    brk = np.flatnonzero(np.diff(v) != 0) + 1
    ends = np.concatenate([brk, [n]])
    starts = np.concatenate([[0], brk])
    end_of = np.repeat(ends, ends - starts)
    return end_of - np.arange(n)


def hybrid(v, bw, style="mr", rng=None):
    """RunLengthBitPackingHybrid runs (no width byte, no length prefix) of v at width bw.
    mr: parquet-mr's writer shape, RLE runs of >= 8 repeats and bit-packed groups otherwise;
    rle: RLE runs only (runs of 1 included); mixed: RLE runs of 1-3 values and 1-group packed runs."""
    v = np.asarray(v, np.uint64)
    n = len(v)
    nb = (bw + 7) // 8
    left = _run_left(v)
    out = bytearray()
    if style == "rle":
        i = 0
        while i < n:
            c = int(left[i])
            out += _uvarint(c << 1) + int(v[i]).to_bytes(nb, "little")
            i += c
        return bytes(out)
    if style == "mixed":
        rng = rng or np.random.default_rng(n + bw)
        i = 0
        coin = rng.random(n + 1)
        size = rng.integers(1, 4, n + 1)
        while i < n:
            if coin[i] < 0.25 or (n - i < 8 and coin[i] < 0.6):
                part = v[i:i + 8]
                if len(part) < 8:
                    part = np.concatenate([part, np.zeros(8 - len(part), np.uint64)])
                out += b"\x03" + _pack_le(part, bw)
                i += 8
            else:
                c = min(int(size[i]), int(left[i]))
                out += _uvarint(c << 1) + int(v[i]).to_bytes(nb, "little")
                i += c
        return bytes(out)
    assert style == "mr", style
    i = 0
    long_starts = np.flatnonzero(left >= 8)
    while i < n:
        if left[i] >= 8:
            c = int(left[i])
            out += _uvarint(c << 1) + int(v[i]).to_bytes(nb, "little")
            i += c
            continue
        # bit-packed groups up to the next run worth an RLE run (whole groups: the packed run may eat
        # the head of that run, and the rest of it is RLE only if 8 or more repeats remain)
        k = np.searchsorted(long_starts, i)
        j = int(long_starts[k]) if k < len(long_starts) else n
        j = min(n, i + (j - i + 7) // 8 * 8)
        out += _packed_runs(v[i:j], bw)
        i = j
    return bytes(out)


def bitpacked_be(v, bw):
    """Deprecated BIT_PACKED levels: big-endian bit order, ceil(n * bw / 8) bytes, no prefix."""
    v = np.asarray(v, np.uint64)
    if bw == 0 or len(v) == 0:
        return b""
    bits = ((v[:, None] >> np.arange(bw - 1, -1, -1, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits.ravel(), bitorder="big").tobytes()


def _bw(max_level):
    return int(max_level).bit_length()


# ---------------------------------------------------------------- value encoders
def plain(ptype, vals):
    if ptype == BYTE_ARRAY:
        return b"".join(len(x).to_bytes(4, "little") + x for x in vals)
    if ptype == BOOLEAN:
        return np.packbits(np.asarray(vals, np.uint8).ravel(), bitorder="little").tobytes()
    return np.ascontiguousarray(vals, np.uint8).tobytes()


def rle_boolean(vals, style="mr", rng=None):
    body = hybrid(np.asarray(vals, np.uint8).ravel(), 1, style, rng)
    return len(body).to_bytes(4, "little") + body


def delta_length(vals):
    return dbp([len(x) for x in vals], bits=32) + b"".join(vals)


def delta_byte_array(vals):
    """Prefix lengths + DELTA_LENGTH suffixes; vals: list of bytes (FLBA rows as bytes too)."""
    pre, suf, prev = [], [], b""
    for x in vals:
        k, m = 0, min(len(prev), len(x))
        while k < m and prev[k] == x[k]:
            k += 1
        pre.append(k)
        suf.append(x[k:])
        prev = x
    return dbp(pre, bits=32) + delta_length(suf)


def byte_stream_split(vals):
    a = np.ascontiguousarray(vals, np.uint8)
    return a.T.tobytes()


def dict_indices(ids, bw, style="mr", rng=None):
    return bytes([bw]) + hybrid(ids, bw, style, rng)


def as_rows(vals):
    """Fixed-width vals as a list of bytes rows (for delta_byte_array)."""
    a = np.ascontiguousarray(vals, np.uint8)
    return [a[i].tobytes() for i in range(len(a))]


# ---------------------------------------------------------------- Thrift compact
class _T:
    """Minimal Thrift compact struct writer."""

    def __init__(self):
        self.b = bytearray()
        self.last = [0]

    def _hdr(self, fid, t):
        d = fid - self.last[-1]
        if 0 < d <= 15:
            self.b.append((d << 4) | t)
        else:
            self.b.append(t)
            self.b += _uvarint((fid << 1) ^ (fid >> 15))
        self.last[-1] = fid

    def i32(self, fid, v):
        self._hdr(fid, 5)
        self.b += _uvarint(((v << 1) ^ (v >> 31)) & 0xFFFFFFFF)
        return self

    def i64(self, fid, v):
        self._hdr(fid, 6)
        self.b += _uvarint(((v << 1) ^ (v >> 63)) & (2**64 - 1))
        return self

    def boolean(self, fid, v):
        self._hdr(fid, 1 if v else 2)
        return self

    def string(self, fid, s):
        self._hdr(fid, 8)
        s = s.encode() if isinstance(s, str) else s
        self.b += _uvarint(len(s)) + s
        return self

    def begin(self, fid):
        self._hdr(fid, 12)
        self.last.append(0)
        return self

    def end(self):
        self.b.append(0)
        self.last.pop()
        return self

    def list_hdr(self, fid, etype, n):
        self._hdr(fid, 9)
        if n < 15:
            self.b.append((n << 4) | etype)
        else:
            self.b.append(0xF0 | etype)
            self.b += _uvarint(n)
        return self

    def elem_begin(self):
        self.last.append(0)
        return self

    def elem_i32(self, v):
        self.b += _uvarint(((v << 1) ^ (v >> 31)) & 0xFFFFFFFF)
        return self

    def elem_string(self, s):
        s = s.encode()
        self.b += _uvarint(len(s)) + s
        return self

    def done(self):
        self.b.append(0)
        return bytes(self.b)


def dict_page_header(n, encoding, usize, csize):
    return _T().i32(1, 2).i32(2, usize).i32(3, csize).begin(7).i32(1, n).i32(2, encoding).end().done()


def v1_page_header(n, encoding, def_enc, rep_enc, usize, csize):
    return (_T().i32(1, 0).i32(2, usize).i32(3, csize)
            .begin(5).i32(1, n).i32(2, encoding).i32(3, def_enc).i32(4, rep_enc).end().done())


def v2_page_header(n, nulls, rows, encoding, def_bytes, rep_bytes, is_compressed, usize, csize):
    t = _T().i32(1, 3).i32(2, usize).i32(3, csize).begin(8)
    t.i32(1, n).i32(2, nulls).i32(3, rows).i32(4, encoding).i32(5, def_bytes).i32(6, rep_bytes)
    if is_compressed is not None:
        t.boolean(7, is_compressed)
    return t.end().done()


# ---------------------------------------------------------------- pages and chunks
class Layout:
    """A page layout: (a) v1 RLE levels uncompressed, (b) v1 BIT_PACKED levels Snappy, (c) v2 Snappy,
    (d) v2 in a Snappy chunk with is_compressed = false, (e) v2 uncompressed."""

    def __init__(self, name, v2, codec, level_enc=RLE, is_compressed=None):
        self.name, self.v2, self.codec, self.level_enc, self.is_compressed = name, v2, codec, level_enc, is_compressed


LAYOUTS = {
    "a": Layout("a", False, UNCOMPRESSED),
    "b": Layout("b", False, SNAPPY, level_enc=BIT_PACKED),
    "c": Layout("c", True, SNAPPY, is_compressed=True),
    "d": Layout("d", True, SNAPPY, is_compressed=False),
    "e": Layout("e", True, UNCOMPRESSED),
}


class Chunk:
    """One column chunk under construction: schema of its leaf, its page bytes, its expected arrays."""

    def __init__(self, name, ptype, type_length=0, optional=False, nested=False, layout=LAYOUTS["a"], compress=None):
        self.name, self.ptype, self.type_length = name, ptype, type_length
        self.optional, self.nested, self.layout, self.compress = optional or nested, nested, layout, compress
        self.width = width_of(ptype, type_length)
        self.max_def = 3 if nested else int(self.optional)
        self.max_rep = int(nested)
        self.dict = b""
        self.pages = []          # page bytes (header + body)
        self.value_spans = []    # per data page: (offset of the stored value section within self.pages[i], its length)
        self.encodings = set()
        self.num_entries = 0
        self.usize = 0
        # expected
        self._slots_valid, self._slot_vals, self._defs, self._reps = [], [], [], []

    def _z(self, raw):
        return self.compress(raw) if self.layout.codec == SNAPPY else raw

    def set_dictionary(self, vals, encoding=PLAIN):
        raw = plain(self.ptype, vals)
        body = self._z(raw)
        self.dict = dict_page_header(len(vals), encoding, len(raw), len(body)) + body
        self.usize += len(self.dict) - len(body) + len(raw)
        self.encodings.add(encoding)

    def add_page(self, encoding, value_bytes, present=None, defs=None, reps=None, vals=None, style="mr", rng=None):
        """One data page. Flat: `present` (bool per entry, None = REQUIRED). Nested: defs / reps per
        entry (max_def 3: 0 null list, 1 empty list, 2 null element, 3 value). `vals` are the page's
        non-null values (for the expected arrays); value_bytes their encoding."""
        L = self.layout
        if self.nested:
            defs = np.asarray(defs, np.uint8)
            reps = np.asarray(reps, np.uint8)
            n = len(defs)
            nulls = int((defs != self.max_def).sum())
            rows = int((reps == 0).sum())
        else:
            n = len(present) if present is not None else len(vals)
            defs = np.asarray(present, np.uint8) if self.optional else None
            if self.optional:
                assert present is not None
            nulls = int(n - defs.sum()) if self.optional else 0
            rows = n
        lv = []
        for levels, mx in ((reps if self.nested else None, self.max_rep), (defs, self.max_def)):
            if levels is None or mx == 0:
                lv.append(b"")
                continue
            bw = _bw(mx)
            if L.v2:
                lv.append(hybrid(levels, bw, style, rng))
            elif L.level_enc == BIT_PACKED:
                lv.append(bitpacked_be(levels, bw))
            else:
                h = hybrid(levels, bw, style, rng)
                lv.append(len(h).to_bytes(4, "little") + h)
        rep_b, def_b = lv
        if L.v2:
            stored = self._z(value_bytes) if (L.codec == SNAPPY and L.is_compressed is not False) else value_bytes
            body = rep_b + def_b + stored
            usize = len(rep_b) + len(def_b) + len(value_bytes)
            hdr = v2_page_header(n, nulls, rows, encoding, len(def_b), len(rep_b), L.is_compressed, usize, len(body))
            span = (len(hdr) + len(rep_b) + len(def_b), len(stored))
        else:
            raw = rep_b + def_b + value_bytes
            body = self._z(raw)
            usize = len(raw)
            lenc = L.level_enc
            hdr = v1_page_header(n, encoding, lenc, lenc, usize, len(body))
            span = (len(hdr) + (0 if L.codec == SNAPPY else len(rep_b) + len(def_b)),
                    len(body) if L.codec == SNAPPY else len(value_bytes))
        self.pages.append(hdr + body)
        self.value_spans.append(span)
        self.usize += len(hdr) + usize
        self.encodings.update({encoding, RLE if L.v2 else L.level_enc})
        self.num_entries += n
        # expected arrays
        if self.nested:
            self._defs.append(defs)
            self._reps.append(reps)
            self._slots_valid.append(defs[defs >= 2] == 3)
        else:
            self._slots_valid.append(np.asarray(present, bool) if present is not None else np.ones(n, bool))
        assert len(vals) == int(self._slots_valid[-1].sum()), (len(vals), int(self._slots_valid[-1].sum()))
        self._slot_vals.append(vals)

    def expected(self):
        valid = np.concatenate(self._slots_valid) if self._slots_valid else np.zeros(0, bool)
        ns = len(valid)
        out = {"num_entries": self.num_entries, "num_slots": ns, "num_values": int(valid.sum())}
        if self.ptype == BYTE_ARRAY:
            allv = [x for v in self._slot_vals for x in v]
            lens = np.zeros(ns, np.int64)
            lens[valid] = [len(x) for x in allv]
            offs = np.zeros(ns + 1, np.int32)
            np.cumsum(lens, out=offs[1:])
            out["offsets"] = offs
            out["chars"] = np.frombuffer(b"".join(allv), np.uint8)
        else:
            v = np.zeros((ns, self.width), np.uint8)
            parts = [np.ascontiguousarray(x, np.uint8).reshape(-1, self.width) for x in self._slot_vals if len(x)]
            if parts:
                v[valid] = np.concatenate(parts)
            out["values"] = v.ravel()
        if self.max_def > 0:
            out["validity"] = np.packbits(valid, bitorder="little")
        if self.nested:
            defs, reps = np.concatenate(self._defs), np.concatenate(self._reps)
            first = reps == 0
            out["num_rows"] = int(first.sum())
            row_of = np.cumsum(first) - 1
            slots_per_row = np.bincount(row_of[defs >= 2], minlength=out["num_rows"])
            lo = np.zeros(out["num_rows"] + 1, np.int32)
            np.cumsum(slots_per_row, out=lo[1:])
            out["list_offsets"] = lo
            out["list_validity"] = np.packbits(defs[first] >= 1, bitorder="little")
            out["def_levels"], out["rep_levels"] = defs, reps
        else:
            out["num_rows"] = self.num_entries
        return out


def build_file(chunks, num_rows):
    """PAR1 + the chunks of one row group + FileMetaData. Returns (file bytes, info) where
    info[i] = {"offset": chunk start, "pages": [file offset of each page incl. the dictionary page],
    "values": [(file offset, length) of each data page's stored value section]}."""
    out = bytearray(b"PAR1")
    info, metas = [], []
    for ch in chunks:
        start = len(out)
        out += ch.dict
        data_off = len(out)
        pages, spans = ([start] if ch.dict else []), []
        for pg, (so, sl) in zip(ch.pages, ch.value_spans):
            pages.append(len(out))
            spans.append((len(out) + so, sl))
            out += pg
        info.append({"offset": start, "pages": pages, "values": spans})
        metas.append((ch, start, data_off, len(out) - start))
    t = _T().i32(1, 1)
    n_elems = 1 + sum(3 if ch.nested else 1 for ch in chunks)
    t.list_hdr(2, 12, n_elems)
    t.elem_begin().string(4, "schema").i32(5, len(chunks)).end()
    for ch in chunks:
        if ch.nested:   # optional group <name> (LIST) { repeated group list { optional <type> element; } }
            t.elem_begin().i32(3, 1).string(4, ch.name).i32(5, 1).i32(6, 3).end()
            t.elem_begin().i32(3, 2).string(4, "list").i32(5, 1).end()
        t.elem_begin().i32(1, ch.ptype)
        if ch.ptype == FLBA:
            t.i32(2, ch.type_length)
        t.i32(3, 1 if ch.optional else 0).string(4, "element" if ch.nested else ch.name).end()
    t.i64(3, num_rows)
    t.list_hdr(4, 12, 1)
    t.elem_begin()
    t.list_hdr(1, 12, len(chunks))
    for ch, start, data_off, size in metas:
        t.elem_begin().i64(2, start)
        t.begin(3).i32(1, ch.ptype)
        encs = sorted(ch.encodings)
        t.list_hdr(2, 5, len(encs))
        for e in encs:
            t.elem_i32(e)
        path = [ch.name, "list", "element"] if ch.nested else [ch.name]
        t.list_hdr(3, 8, len(path))
        for s in path:
            t.elem_string(s)
        t.i32(4, ch.layout.codec).i64(5, ch.num_entries).i64(6, ch.usize).i64(7, size).i64(9, data_off)
        if ch.dict:
            t.i64(11, start)
        t.end().end()
    t.i64(2, sum(m[0].usize for m in metas)).i64(3, num_rows).end()
    t.string(6, "pagekit (test assembler)")
    footer = t.done()
    out += footer + len(footer).to_bytes(4, "little") + b"PAR1"
    return bytes(out), info
