"""Page / chunk statistics and page CRCs of the write path (PF_ENCODE_STATISTICS, PF_ENCODE_PAGE_CRC):
the reference the tests compare with, a Thrift compact reader for page headers and footers, and the cases.

The reference (ref_stats) states the write rules of parquet-format's ColumnOrder TYPE_ORDER value by value, in
Python, from the present values alone; test_write_stats_cpu.py pins it to pyarrow's writer. No product code here."""
import struct

import numpy as np

import pagekit as K

TILE = 4096          # ST_TILE of csrc/pf_enc_tables.h: dense values of one workgroup (test_write_stats_cpu.py pins it)
LIMIT = 4096         # len(min) + len(max) at or above it: no Statistics struct
DEFAULT_PAGE_ROWS = 20000
_FMT = {K.INT32: "<i", K.INT64: "<q", K.FLOAT: "<f", K.DOUBLE: "<d"}
_DT = {K.BOOLEAN: np.uint8, K.INT32: np.int32, K.INT64: np.int64, K.FLOAT: np.float32, K.DOUBLE: np.float64}


# ---------------------------------------------------------------- the reference
def ref_stats(ptype, values, nulls):
    """Statistics of the present `values` (a list of Python ints / floats / bools / bytes) with `nulls` null rows:
    {"null_count", "min", "max" (PLAIN bytes or None), "legacy" (the fields 1 / 2 are written too)}, or None when
    the struct is not written at all (size limit)."""
    lo = hi = None
    if ptype == K.BYTE_ARRAY:
        for v in values:                       # Python compares bytes unsigned, a proper prefix first
            lo = v if lo is None or v < lo else lo
            hi = v if hi is None or v > hi else hi
        if lo is not None and len(lo) + len(hi) >= LIMIT:
            return None
        legacy = lo is not None and lo == hi
    elif ptype == K.BOOLEAN:
        for v in values:
            b = b"\x01" if v else b"\x00"
            lo = b if lo is None or b < lo else lo
            hi = b if hi is None or b > hi else hi
        legacy = True
    elif ptype in (K.INT32, K.INT64):
        for v in values:
            lo = v if lo is None or v < lo else lo
            hi = v if hi is None or v > hi else hi
        if lo is not None:
            lo, hi = struct.pack(_FMT[ptype], lo), struct.pack(_FMT[ptype], hi)
        legacy = True
    else:
        for v in values:
            if v != v:                         # NaN of either sign, any payload
                continue
            lo = v if lo is None or v < lo else lo
            hi = v if hi is None or v > hi else hi
        if lo is not None:
            lo = -0.0 if lo == 0 else lo       # a zero min is written -0.0, a zero max +0.0
            hi = 0.0 if hi == 0 else hi
            lo, hi = struct.pack(_FMT[ptype], lo), struct.pack(_FMT[ptype], hi)
        legacy = True
    return {"null_count": nulls, "min": lo, "max": hi, "legacy": legacy and lo is not None}


def expected_fields(ref):
    """The Statistics struct as the header reader returns it ({field id: value}), or None."""
    if ref is None:
        return None
    out = {3: ref["null_count"]}
    if ref["min"] is not None:
        out[5], out[6] = ref["max"], ref["min"]
        if ref["legacy"]:
            out[1], out[2] = ref["max"], ref["min"]
    return out


# ---------------------------------------------------------------- Thrift compact
def _uvarint(b, pos):
    v = s = 0
    while True:
        c = b[pos]
        pos += 1
        v |= (c & 0x7f) << s
        s += 7
        if c < 0x80:
            return v, pos


def _zigzag(b, pos):
    v, pos = _uvarint(b, pos)
    return (v >> 1) ^ -(v & 1), pos


def _value(b, pos, t):
    if t in (1, 2):
        return t == 1, pos
    if t == 3:
        return struct.unpack_from("<b", b, pos)[0], pos + 1
    if t in (4, 5, 6):
        return _zigzag(b, pos)
    if t == 7:
        return struct.unpack_from("<d", b, pos)[0], pos + 8
    if t == 8:
        n, pos = _uvarint(b, pos)
        return bytes(b[pos:pos + n]), pos + n
    if t in (9, 10):
        hb = b[pos]
        pos += 1
        n, et = hb >> 4, hb & 15
        if n == 15:
            n, pos = _uvarint(b, pos)
        out = []
        for _ in range(n):
            if et in (1, 2):
                out.append(b[pos] == 1)
                pos += 1
            else:
                v, pos = _value(b, pos, et)
                out.append(v)
        return out, pos
    if t == 12:
        return read_struct(b, pos)
    raise ValueError(f"thrift type {t}")


def read_struct(b, pos=0):
    """A Thrift compact struct at b[pos:] -> ({field id: value}, end); structs nest as dicts, lists as lists."""
    out, last = {}, 0
    while True:
        c = b[pos]
        pos += 1
        if c == 0:
            return out, pos
        if c >> 4:
            fid = last + (c >> 4)
        else:
            fid, pos = _zigzag(b, pos)
        last = fid
        out[fid], pos = _value(b, pos, c & 15)


def footer(path):
    """FileMetaData of a file as nested {field id: value}."""
    with open(path, "rb") as f:
        raw = f.read()
    n = struct.unpack("<I", raw[-8:-4])[0]
    return read_struct(raw[-8 - n:-8])[0]


def page_headers(path, col, rg=0):
    """Every page of a chunk, by its PageHeader alone: [{"type", "uncompressed", "compressed", "crc" (uint32 or None),
    "v2" (DataPageHeaderV2 fields or None), "stats" (Statistics fields or None), "body" (file offset), "page" (index)}]."""
    fm = footer(path)
    md = fm[4][rg][1][col][3]
    start = md[11] if 11 in md and 0 < md[11] < md[9] else md[9]
    size, total = md[7], md[5]
    with open(path, "rb") as f:
        f.seek(start)
        raw = f.read(size)
    out, pos, seen = [], 0, 0
    while pos < size and seen < total:
        h, end = read_struct(raw, pos)
        v2 = h.get(8)
        out.append({"type": h[1], "uncompressed": h[2], "compressed": h[3], "crc": (h[4] & 0xffffffff) if 4 in h else None,
                    "v2": v2, "stats": v2.get(8) if v2 else None, "body": start + end, "page": len(out)})
        if v2:
            seen += v2[1]
        pos = end + h[3]
    assert pos == size, (path, col, pos, size)
    return out


# ---- writers of the same structs, for the hand-built chunks of test_write_stats_cpu.py
def w_uvarint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def w_zz(v):
    return w_uvarint((v << 1) ^ (v >> 63))


def w_statistics(st):
    """{field id: bytes | int} -> the struct's bytes (fields in ascending order)."""
    out, last = bytearray(), 0
    for fid in sorted(st):
        v = st[fid]
        if isinstance(v, bytes):
            out += bytes([(fid - last) << 4 | 8]) + w_uvarint(len(v)) + v
        else:
            out += bytes([(fid - last) << 4 | 6]) + w_zz(v)
        last = fid
    return bytes(out) + b"\x00"


def w_page_header_v2(n, nulls, enc, def_bytes, values_bytes, crc=None, stats=None):
    """PageHeader{1 type=3, 2, 3, [4 crc], 8 DataPageHeaderV2{1..7, [8 statistics]}} of an uncompressed page."""
    size = def_bytes + values_bytes
    h = bytearray(bytes([0x15]) + w_zz(3) + bytes([0x15]) + w_zz(size) + bytes([0x15]) + w_zz(size))
    if crc is not None:
        h += bytes([0x15]) + w_zz(crc - (1 << 32) if crc >= 1 << 31 else crc)
        h += bytes([0x4c])   # field 8 (delta 4), struct
    else:
        h += bytes([0x5c])   # field 8 (delta 5), struct
    for v in (n, nulls, n, enc, def_bytes, 0):
        h += bytes([0x15]) + w_zz(v)
    h += bytes([0x12])       # field 7 bool false (is_compressed)
    if stats is not None:
        h += bytes([0x1c]) + w_statistics(stats)
    return bytes(h) + b"\x00\x00"


# ---------------------------------------------------------------- cases
def _rng(*key):
    return np.random.default_rng(sum(ord(c) * (i + 7) for i, c in enumerate("/".join(map(str, key)))))


def _null_fill(ptype, k):
    """What a null row holds in the encoder's input: bit patterns (strings: bytes) that would win a compare."""
    if ptype == K.BYTE_ARRAY:
        return (b"", b"\xff\xff\xff\xff\xff\xff\xff\xff\xff\xff")[k % 2]
    if ptype == K.BOOLEAN:
        return k % 2
    if ptype in (K.INT32, K.INT64):
        ii = np.iinfo(_DT[ptype])
        return (ii.min, ii.max)[k % 2]
    return (-np.inf, np.inf)[k % 2]


class Case:
    """One column chunk: `dense` present values (numpy array, or a list of bytes), `present` row mask (None:
    REQUIRED), rows per page."""

    def __init__(self, name, ptype, dense, present=None, page_rows=DEFAULT_PAGE_ROWS):
        self.name, self.ptype, self.page_rows = name, ptype, page_rows
        self.present = None if present is None else np.asarray(present, bool)
        self.dense = list(dense) if ptype == K.BYTE_ARRAY else np.asarray(dense, _DT[ptype])
        self.rows = len(self.dense) if self.present is None else len(self.present)
        assert len(self.dense) == (self.rows if self.present is None else int(self.present.sum())), name

    @property
    def optional(self):
        return self.present is not None

    def mask(self):
        return np.ones(self.rows, bool) if self.present is None else self.present

    def values(self, d0, d1):
        """Present values [d0, d1) as the reference takes them."""
        if self.ptype == K.BYTE_ARRAY:
            return self.dense[d0:d1]
        if self.ptype == K.BOOLEAN:
            return self.dense[d0:d1].astype(bool).tolist()
        if self.ptype == K.FLOAT:   # float32 -> Python float is exact, and back
            return [float(v) for v in self.dense[d0:d1]]
        return self.dense[d0:d1].tolist()

    def page_refs(self):
        """ref_stats of every data page, and of the chunk."""
        mask, out, d = self.mask(), [], 0
        for r0 in range(0, max(self.rows, 1), self.page_rows):
            pm = mask[r0:r0 + self.page_rows]
            cnt = int(pm.sum())
            out.append(ref_stats(self.ptype, self.values(d, d + cnt), len(pm) - cnt))
            d += cnt
        return out, ref_stats(self.ptype, self.values(0, len(self.dense)), self.rows - len(self.dense))

    def row_arrays(self):
        """The column as the encoder takes it: (values | (offsets, chars), validity or None); null rows hold
        values that would win the compare."""
        mask = self.mask()
        validity = np.packbits(mask, bitorder="little") if self.optional else None
        nulls = np.flatnonzero(~mask)
        if self.ptype == K.BYTE_ARRAY:
            vals, it = [], iter(self.dense)
            for r, p in enumerate(mask):
                vals.append(next(it) if p else _null_fill(self.ptype, r))
            offsets = np.zeros(self.rows + 1, np.int32)
            np.cumsum([len(v) for v in vals], out=offsets[1:])
            return (offsets, np.frombuffer(b"".join(vals), np.uint8)), validity
        v = np.zeros(self.rows, _DT[self.ptype])
        v[mask] = self.dense
        for k in (0, 1):
            v[nulls[nulls % 2 == k]] = _null_fill(self.ptype, k)
        return v, validity

    def expected(self):
        """The decoded chunk in the canonical layout of include/pfloor.h (null slots zero / empty)."""
        mask = self.mask()
        out = {"num_entries": self.rows, "num_slots": self.rows, "num_values": int(mask.sum()), "num_rows": self.rows}
        if self.ptype == K.BYTE_ARRAY:
            lens = np.zeros(self.rows, np.int64)
            lens[mask] = [len(v) for v in self.dense]
            out["offsets"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            out["chars"] = np.frombuffer(b"".join(self.dense), np.uint8)
        else:
            v = np.zeros(self.rows, _DT[self.ptype])
            v[mask] = self.dense
            out["values"] = v.view(np.uint8)
        if self.optional:
            out["validity"] = np.packbits(mask, bitorder="little")
        return out

    def arrow(self):
        """The column as a pyarrow array of its physical type (nulls where the mask says so)."""
        import pyarrow as pa
        mask = self.mask()
        if self.ptype == K.BYTE_ARRAY:
            it = iter(self.dense)
            return pa.array([next(it) if p else None for p in mask], pa.binary())
        v = np.zeros(self.rows, _DT[self.ptype])
        v[mask] = self.dense
        if self.ptype == K.BOOLEAN:
            v = v.astype(bool)
        return pa.array(v, mask=~mask) if self.optional else pa.array(v)


TYPES = (("i32", K.INT32), ("i64", K.INT64), ("f32", K.FLOAT), ("f64", K.DOUBLE), ("b", K.BOOLEAN), ("s", K.BYTE_ARRAY))


def _random_dense(ptype, n, key):
    rng = _rng("dense", ptype, n, key)
    if ptype == K.BYTE_ARRAY:
        return [bytes(rng.integers(98, 122, int(rng.integers(1, 12)), dtype=np.uint8)) for _ in range(n)]   # 'b'..'y'
    if ptype == K.BOOLEAN:
        return rng.integers(0, 2, n).astype(np.uint8)
    if ptype in (K.INT32, K.INT64):
        return rng.integers(-1000, 1001, n)
    return (rng.random(n) * 2000 - 1000).astype(_DT[ptype])


def _extreme(ptype, lo, k):
    """A value beyond _random_dense's range: the smaller (lo) or larger, more so with k."""
    if ptype == K.BYTE_ARRAY:
        if k >= 3000:
            return b"a!" if lo else b"z~~"
        return (b"a" + bytes([121 - k % 20]) * 3) if lo else (b"z" + bytes([98 + k % 20]) * 3)
    if ptype == K.BOOLEAN:
        return 0 if lo else 1
    return (-5000 - k) if lo else (5000 + k)


# present values of the pages of the "counts" file: 0 between two normal pages, the lane, wave, workgroup and tile
# edges, and the same around two tiles
COUNTS = (300, 0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 500)
COUNTS_PAGE_ROWS = 2 * TILE + 8


def _counts_cases():
    """OPTIONAL columns whose page k holds COUNTS[k] present values among COUNTS_PAGE_ROWS rows. The extremes of a
    page sit, by k mod 4: first / last value (0: min first, 2: max first) -- so the odd pages between them have a
    more extreme value right before their first and right after their last value -- or inside (1, 3): at the ends of
    a wave, a workgroup stride and a tile, whichever the page is large enough for."""
    out = []
    inner = (63, 64, 255, 256, TILE - 1, TILE, 2 * TILE - 1)
    for tname, ptype in TYPES:
        rng = _rng("counts", tname)
        present = np.zeros(len(COUNTS) * COUNTS_PAGE_ROWS, bool)
        dense = []
        for k, cnt in enumerate(COUNTS):
            rows = np.sort(rng.choice(COUNTS_PAGE_ROWS, cnt, replace=False))
            present[k * COUNTS_PAGE_ROWS + rows] = True
            v = list(_random_dense(ptype, cnt, k))
            if cnt >= 2 and k % 2 == 0:
                first_lo = k % 4 == 0
                v[0], v[-1] = _extreme(ptype, first_lo, 3000 + k), _extreme(ptype, not first_lo, 3000 + k)
            elif cnt >= 2:
                spots = [p for p in inner if p < cnt] or [0]
                pmin, pmax = spots[k % len(spots)], spots[(k // 2 + 1) % len(spots)]
                if pmin == pmax:
                    pmax = (pmin + 1) % cnt
                v[pmin], v[pmax] = _extreme(ptype, True, k), _extreme(ptype, False, k)
            dense += v
        out.append(Case(f"{tname}_counts", ptype, dense, present=present, page_rows=COUNTS_PAGE_ROWS))
    return out


def _r20001_cases():
    """One chunk of 20,001 rows over 20,000-row pages, per type: REQUIRED, 30 % nulls, OPTIONAL without nulls."""
    out, n = [], 20001
    for tname, ptype in TYPES:
        out.append(Case(f"{tname}_req", ptype, _random_dense(ptype, n, "req")))
        m = _rng("r20001", tname).random(n) >= 0.3
        m[-1] = True
        out.append(Case(f"{tname}_nulls", ptype, _random_dense(ptype, int(m.sum()), "nulls"), present=m))
        out.append(Case(f"{tname}_opt", ptype, _random_dense(ptype, n, "opt"), present=np.ones(n, bool)))
    return out


def _with_nulls(name, ptype, dense, page_rows, key):
    """The case REQUIRED, and OPTIONAL with about 30 % null rows between the same values."""
    n = len(dense)
    m = np.zeros(n + (n * 3) // 7 + 1, bool)
    m[np.sort(_rng("nulls", name, key).choice(len(m), n, replace=False))] = True
    return [Case(name, ptype, dense, page_rows=page_rows), Case(name + "_nulls", ptype, dense, present=m, page_rows=page_rows)]


def _int_cases():
    out = []
    for tname, ptype in (("i32", K.INT32), ("i64", K.INT64)):
        ii = np.iinfo(_DT[ptype])
        rng = _rng("ints", tname)
        n = 1000
        both = rng.integers(-50, 50, n)
        both[[17, 500]] = ii.min, ii.max
        out += _with_nulls(f"{tname}_type_min_max", ptype, both, 136, 1)
        out += _with_nulls(f"{tname}_all_negative", ptype, -rng.integers(1, 1 << 30, n), 136, 2)
        out += _with_nulls(f"{tname}_minus1_0", ptype, np.where(rng.random(n) < 0.5, -1, 0), 136, 3)
        out += _with_nulls(f"{tname}_constant", ptype, np.full(n, -77), 136, 4)
        wide = rng.integers(ii.min, ii.max, n, dtype=_DT[ptype])
        out += _with_nulls(f"{tname}_full_range", ptype, wide, 136, 5)
    return out


def _float_cases():
    """Four pages of 64 values; `nan` builds NaNs of both signs with payloads from raw bits."""
    out = []
    for tname, ptype in (("f32", K.FLOAT), ("f64", K.DOUBLE)):
        dt, ut = _DT[ptype], (np.uint32 if ptype == K.FLOAT else np.uint64)
        bits = 32 if ptype == K.FLOAT else 64
        mant = 23 if ptype == K.FLOAT else 52
        exp_all = ((1 << (bits - 1 - mant)) - 1) << mant

        def nan(neg, payload):
            return np.array([(int(neg) << (bits - 1)) | exp_all | payload], ut).view(dt)[0]

        rng = _rng("floats", tname)
        base = (rng.random(256) * 200 - 100).astype(dt)
        v = base.copy()
        for p in range(4):
            v[64 * p], v[64 * p + 63] = nan(p % 2, 1 + p), nan((p + 1) % 2, 1 << (mant - 1))
        out += _with_nulls(f"{tname}_nan_first_last", ptype, v, 64, 1)
        v = base.copy()
        v[64:128] = [nan(k % 2, 1 + k) for k in range(64)]
        out += _with_nulls(f"{tname}_nan_page", ptype, v, 64, 2)
        out += _with_nulls(f"{tname}_all_nan", ptype, np.array([nan(k % 3 == 0, 1 + k) for k in range(256)], dt), 64, 3)
        v = base.copy()
        v[rng.choice(256, 90, replace=False)] = nan(1, 5)
        out += _with_nulls(f"{tname}_negative_nan", ptype, v, 64, 4)
        v = base.copy()
        v[[3, 70, 130]], v[[9, 100, 200]] = -np.inf, np.inf
        out += _with_nulls(f"{tname}_inf", ptype, v, 64, 5)
        tiny = np.array([1, 2, 7, (1 << mant) - 1], ut)
        sub = np.concatenate([tiny, tiny | ut(1 << (bits - 1))]).view(dt)
        v = sub[rng.integers(0, len(sub), 256)]
        v[128:192] = np.abs(v[128:192])          # a page of positive subnormals only
        out += _with_nulls(f"{tname}_subnormal", ptype, v, 64, 6)
        z = np.zeros(256, dt)
        z[64:128] = -0.0
        z[128:192] = np.where(rng.random(64) < 0.4, 0.0, np.where(rng.random(64) < 0.5, -0.0, 1.0 + rng.random(64))).astype(dt)
        z[192:256] = np.where(rng.random(64) < 0.4, 0.0, np.where(rng.random(64) < 0.5, -0.0, -1.0 - rng.random(64))).astype(dt)
        out += _with_nulls(f"{tname}_zeros", ptype, z, 64, 7)
    return out


def _bool_cases():
    out, n = [], 1000
    out += _with_nulls("b_all_true", K.BOOLEAN, np.ones(n, np.uint8), 136, 1)
    out += _with_nulls("b_all_false", K.BOOLEAN, np.zeros(n, np.uint8), 136, 2)
    out += _with_nulls("b_mixed", K.BOOLEAN, _rng("bmix").integers(0, 2, n), 136, 3)
    v = np.zeros(n, np.uint8)
    v[136:272] = 1                                # a page of true between pages of false
    out += _with_nulls("b_page_of_true", K.BOOLEAN, v, 136, 4)
    return out


def _string_cases():
    """512 values over pages of 64."""
    out, n = [], 512
    rng = _rng("strings")

    def pick(vals, key):
        return [vals[i] for i in _rng("pick", key).integers(0, len(vals), n)]

    chain = [b"", b"a", b"a\x00", b"b", b"\xc3\xa9", b"\xff"]
    v = pick(chain, "chain")
    for p in range(6):                             # page p lacks chain[p], so the pages' extremes differ
        v[64 * p:64 * p + 64] = [x if x != chain[p] else chain[(p + 1) % 6] for x in v[64 * p:64 * p + 64]]
    out += _with_nulls("s_chain", K.BYTE_ARRAY, v, 64, 1)
    for at in (9, 64, 1000):                       # equal up to byte `at`, which differs
        head = b"prefix8!" + b"\x80" * (at - 9)
        vals = [head + bytes([c]) + tail for c in (0, 1, 0x7f, 0x80, 0xff) for tail in (b"", b"x", b"\x00")]
        out += _with_nulls(f"s_tie_at_{at}", K.BYTE_ARRAY, pick(vals, at), 64, at)
    for k in (7, 8, 9):                            # a value that is a k-byte prefix of the others
        long = b"abcdefghijkl"
        vals = [long[:k], long[:k] + b"\x00", long, long[:k] + b"\xff"]
        v = pick(vals, k)
        v[64:128] = [x if x != long[:k] else long for x in v[64:128]]   # a page without the prefix itself
        out += _with_nulls(f"s_prefix_{k}", K.BYTE_ARRAY, v, 64, k)
    out += _with_nulls("s_empty_alone", K.BYTE_ARRAY, [b""] * n, 64, 2)
    v = [bytes(rng.integers(0x80, 0x100, int(rng.integers(0, 20)), dtype=np.uint8)) for _ in range(n)]
    out += _with_nulls("s_high_bytes", K.BYTE_ARRAY, v, 64, 3)
    v = [bytes(rng.integers(0, 3, int(rng.integers(0, 14)), dtype=np.uint8)) for _ in range(n)]
    out += _with_nulls("s_embedded_zeros", K.BYTE_ARRAY, v, 64, 4)
    v = pick([b"left", b"right", b"middle"], "eq")
    v[128:192] = [b"all the same"] * 64
    out += _with_nulls("s_equal_page", K.BYTE_ARRAY, v, 64, 5)
    for size in (2047, 2048):                      # the first page holds the long values; the others keep statistics
        v = pick([b"m", b"n", b"o"], size)
        v[5], v[40] = b"a" * size, b"z" * size
        out += _with_nulls(f"long_{size}", K.BYTE_ARRAY, v, 64, size)
    return out


def _size_cases():
    """Pages of 8 rows whose values sections are exactly 0, 1, 8,191, 8,192, 8,193 and 16,385 bytes -- the job
    boundaries of the compressor -- as PLAIN (one BYTE_ARRAY value of that size less 4; BOOLEAN for 1; an all-null
    page for 0), with the same values as dictionaries of those sizes."""
    sizes = (8191, 8192, 8193, 16385)
    present = np.zeros(8 * 6, bool)
    present[[8 + 3, 16, 24 + 7, 32 + 1]] = True    # page 0 and page 5: all null
    vals = [bytes([65 + k]) * (s - 4) for k, s in enumerate(sizes)]
    out = [Case("s_sizes", K.BYTE_ARRAY, vals, present=present, page_rows=8)]
    bp = np.zeros(48, bool)
    bp[[8, 9, 10, 16, 40, 41, 42, 43, 44, 45, 46, 47]] = True
    out.append(Case("b_sizes", K.BOOLEAN, np.arange(12) % 2, present=bp, page_rows=8))
    for k, s in enumerate(sizes):                  # a dictionary page of exactly s bytes: one value, 48 times
        out.append(Case(f"s_dict_{s}", K.BYTE_ARRAY, [bytes([97 + k]) * (s - 4)] * 24, present=np.arange(48) % 2 == 0, page_rows=8))
    return out


_BUILDERS = {"counts": _counts_cases, "r20001": _r20001_cases, "ints": _int_cases, "floats": _float_cases,
             "bools": _bool_cases, "strings": _string_cases, "sizes": _size_cases}
STAT_FILE_IDS = ("counts", "r20001", "ints", "floats", "bools", "strings")
_CACHE = {}


def file_groups(fid):
    """[(rows, cases)] of a test id: one file per row count of its cases (a row group's chunks have the same rows).
    Built once and shared (callers must not modify the arrays)."""
    if fid not in _CACHE:
        cases = _BUILDERS[fid]()
        assert len({c.name for c in cases}) == len(cases), fid
        groups = {}
        for c in cases:
            groups.setdefault(c.rows, []).append(c)
        _CACHE[fid] = sorted(groups.items())
    return _CACHE[fid]


# dictionary bits of pf_encode_column besides 8 | 16, by route
ROUTES = {"dictionary": dict(dictionary=True),
          "plain_fallback": dict(dictionary=True, dict_page_limit=1),   # every dictionary is over the limit
          "delta_fallback": dict(dictionary=False, delta_fallback=True),
          "hybrid_runs": dict(dictionary=True, hybrid_runs=True),
          "all_bits": dict(dictionary=True, delta_fallback=True, hybrid_runs=True)}
