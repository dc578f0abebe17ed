"""Reference and case generator of the default write route's byte-exact tests (TEST INFRASTRUCTURE ONLY; pure
Python + numpy, no product code): what pf_encode_chunk writes with no opt-in bit, stated from the inputs alone.
Shared by test_write_cases_cpu.py (the reference pages, wrapped in files and read back by the oracle and pyarrow)
and test_gpu_write_bytes.py (the GPU encoder against those bytes).

The route:
  dictionary page   PLAIN of the distinct present values in order of first occurrence. Identity is by raw bits:
                    -0.0 and +0.0 are two entries, two NaN payloads are two entries (parquet-mr canonicalises NaN;
                    this writer keeps the bits -- a divergence test_write_config4_shape pins as well).
  data page values  RLE_DICTIONARY: one byte bw = max(1, bit_length(D - 1)), then, if the page has a present value,
                    varint((groups << 1) | 1) and groups * bw bytes: the ids LSB-first, the last group padded with
                    zeros. PLAIN: per the format; BOOLEAN bit-packed LSB-first.
  levels            OPTIONAL: varint((groups << 1) | 1) and the page's validity bytes, bits past the last row
                    cleared; none for a page of zero rows.
  fallback          BOOLEAN never has a dictionary (3); a dictionary over dict_page_limit bytes (fixed width D * w,
                    BYTE_ARRAY sum of 4 + len) turns the whole chunk PLAIN (1); a chunk without a present value
                    has no dictionary and is PLAIN (0).
  pages             page_rows rounded up to a multiple of 8 (20,000 by default); a chunk of no rows is one empty page.

The ids are packed value by value (pagekit._pack_le: every value's bits in turn), not in the 64-bit words of
k_enc_pages. A case is one column: its present values, the rows they sit in and the encoder's settings. The rows
under nulls hold garbage that occurs nowhere among the present values: it must reach neither the dictionary nor
the pages. Cases of equal row count share a file (`file_cases`)."""
import numpy as np

import hybrid_cases as HC
import pagekit as K

DEFAULT_PAGE_ROWS = 20000
DEFAULT_DICT_LIMIT = 1 << 20
PAGE_DATA_V2, PAGE_DICTIONARY = 3, 2
_DTYPE = {K.BOOLEAN: np.uint8, K.INT32: np.int32, K.INT64: np.int64, K.FLOAT: np.float32, K.DOUBLE: np.float64}
_BITS = {K.BOOLEAN: np.uint8, K.INT32: np.uint32, K.INT64: np.uint64, K.FLOAT: np.uint32, K.DOUBLE: np.uint64}
# bit patterns of the garbage under nulls, + row: far negative integers, large finite floats
_GARBAGE = {K.INT32: 0x80000000, K.INT64: 0x8000000000000000, K.FLOAT: 0x7f000000, K.DOUBLE: 0x7fe0000000000000}


def id_width(d):
    """Bit width of the ids of a d-entry dictionary on this route: never 0."""
    return max(1, int(d - 1).bit_length())


def packed_ids(ids, bw):
    """One bit-packed run of all ids: varint((groups << 1) | 1), then the ids LSB-first, zero padding."""
    groups = (len(ids) + 7) // 8
    v = np.zeros(groups * 8, np.uint64)
    v[:len(ids)] = ids
    return K._uvarint((groups << 1) | 1) + K._pack_le(v, bw)


class Case:
    """One column chunk. dense: its present values (numpy array of the type's dtype; BYTE_ARRAY: list of bytes);
    present: bool per row (None: no nulls); optional: max_def = 1 (default: present is given); send_validity=False:
    an OPTIONAL column passed without a validity array (all present)."""

    def __init__(self, name, ptype, dense, present=None, optional=None, page_rows=0, dictionary=True, dict_page_limit=0,
                 send_validity=True):
        self.name, self.ptype, self.page_rows = name, ptype, page_rows
        self.dictionary, self.dict_page_limit, self.send_validity = dictionary, dict_page_limit, send_validity
        self.present = None if present is None else np.asarray(present, bool)
        self.optional = (present is not None) if optional is None else optional
        assert self.optional or self.present is None, name
        assert send_validity or self.present is None, name
        if ptype == K.BYTE_ARRAY:
            self.dense = [bytes(x) for x in dense]
        else:
            self.dense = np.ascontiguousarray(dense, _DTYPE[ptype])
        self.rows = len(self.dense) if self.present is None else len(self.present)
        assert len(self.dense) == int(self.mask().sum()), name
        self._plan = None

    # ---- inputs
    def mask(self):
        return np.ones(self.rows, bool) if self.present is None else self.present

    def keys(self):
        """The present values as what the dictionary tells apart: raw bits, or the bytes themselves."""
        if self.ptype == K.BYTE_ARRAY:
            k = np.empty(len(self.dense), object)
            k[:] = self.dense
            return k
        return self.dense.view(_BITS[self.ptype])

    def row_arrays(self):
        """The column as the encoder takes it: (values | (offsets, chars), validity or None). Null rows hold
        garbage that differs from row to row and from every present value."""
        mask = self.mask()
        validity = np.packbits(mask, bitorder="little") if (self.optional and self.send_validity) else None
        nulls = np.flatnonzero(~mask)
        if self.ptype == K.BYTE_ARRAY:
            rows = [b"\xffnull-%d" % r for r in range(self.rows)]
            assert not set(rows) & set(self.dense), self.name
            for r, x in zip(np.flatnonzero(mask), self.dense):
                rows[r] = x
            offsets = np.zeros(self.rows + 1, np.int32)
            np.cumsum([len(x) for x in rows], out=offsets[1:])
            return (offsets, np.frombuffer(b"".join(rows), np.uint8)), validity
        bits = _BITS[self.ptype]
        v = np.zeros(self.rows, bits)
        v[mask] = self.keys()
        if self.ptype == K.BOOLEAN:
            v[nulls] = (nulls * 7 // 3) % 2             # (a BOOLEAN has no value to spare)
        else:
            v[nulls] = (np.uint64(_GARBAGE[self.ptype]) + nulls.astype(np.uint64)).astype(bits)
            assert not np.isin(v[nulls], self.keys()).any(), self.name
        return v.view(_DTYPE[self.ptype]), validity

    # ---- the reference
    def plan(self):
        """{"fallback", "dict": values or None, "dict_bytes", "bw", "encoding", "pages": [{"rows", "nulls", "levels",
        "values"}]} of the chunk."""
        if self._plan is not None:
            return self._plan
        mask, keys, m = self.mask(), self.keys(), len(self.dense)
        w = K.width_of(self.ptype)
        fallback, dvals, ids = 0, None, None
        if self.dictionary and self.ptype == K.BOOLEAN:
            fallback = 3
        elif self.dictionary and m > 0:
            ids, dvals = HC.first_occurrence_ids(keys)
            size = sum(4 + len(x) for x in dvals) if self.ptype == K.BYTE_ARRAY else len(dvals) * w
            if size > (self.dict_page_limit or DEFAULT_DICT_LIMIT):
                fallback, dvals, ids = 1, None, None
        p = {"fallback": fallback, "dict": dvals, "dict_bytes": None, "bw": None,
             "encoding": K.PLAIN if dvals is None else K.RLE_DICTIONARY, "pages": []}
        if dvals is not None:
            p["bw"] = id_width(len(dvals))
            p["dict_bytes"] = K.plain(self.ptype, list(dvals) if self.ptype == K.BYTE_ARRAY else
                                      np.ascontiguousarray(dvals).view(np.uint8).reshape(len(dvals), w))
        pr = ((self.page_rows or DEFAULT_PAGE_ROWS) + 7) // 8 * 8
        d = 0
        for r0 in range(0, max(self.rows, 1), pr):
            pm = mask[r0:r0 + pr]
            rows, cnt = len(pm), int(pm.sum())
            levels = b""
            if self.optional and rows:
                levels = K._uvarint((((rows + 7) // 8) << 1) | 1) + np.packbits(pm, bitorder="little").tobytes()
            if dvals is not None:
                values = bytes([p["bw"]]) + (packed_ids(ids[d:d + cnt], p["bw"]) if cnt else b"")
            elif self.ptype == K.BYTE_ARRAY:
                values = K.plain(self.ptype, self.dense[d:d + cnt])
            else:
                values = K.plain(self.ptype, keys[d:d + cnt] if self.ptype == K.BOOLEAN else
                                 np.ascontiguousarray(keys[d:d + cnt]).view(np.uint8))
            p["pages"].append({"rows": rows, "nulls": rows - cnt, "levels": levels, "values": values, "d0": d, "cnt": cnt})
            d += cnt
        assert d == m
        self._plan = p
        return p

    # ---- what readers must return
    def expected(self):
        """The decoded chunk in the canonical layout of include/pfloor.h (what golden_util compares)."""
        mask = self.mask()
        out = {"num_entries": self.rows, "num_slots": self.rows, "num_values": int(mask.sum()), "num_rows": self.rows}
        if self.ptype == K.BYTE_ARRAY:
            lens = np.zeros(self.rows, np.int64)
            lens[mask] = [len(x) for x in self.dense]
            out["offsets"] = np.zeros(self.rows + 1, np.int32)
            np.cumsum(lens, out=out["offsets"][1:])
            out["chars"] = np.frombuffer(b"".join(self.dense), np.uint8)
        else:
            v = np.zeros(self.rows, _BITS[self.ptype])
            v[mask] = self.keys()
            out["values"] = v.view(np.uint8)
        if self.optional:
            out["validity"] = np.packbits(mask, bitorder="little")
        return out

    def check_arrow(self, col, label):
        """A pyarrow ChunkedArray of the column holds the inputs: validity, and the present values bit for bit."""
        arr = col.combine_chunks() if hasattr(col, "combine_chunks") else col
        mask = self.mask()
        assert len(arr) == self.rows, label
        assert np.array_equal(arr.is_valid().to_numpy(zero_copy_only=False), mask), f"{label}: validity"
        if self.ptype in (K.BYTE_ARRAY, K.BOOLEAN):
            got = [x for x in arr.to_pylist() if x is not None]
            want = self.dense if self.ptype == K.BYTE_ARRAY else self.dense.astype(bool).tolist()
            assert got == want, f"{label}: values"
            return
        raw = np.frombuffer(arr.buffers()[1], _BITS[self.ptype])[arr.offset:arr.offset + self.rows]
        assert np.array_equal(raw[mask], self.keys()), f"{label}: values"


def reference_chunk(case):
    """The case's reference pages as an uncompressed pagekit chunk (v2 pages; pagekit writes the headers)."""
    p = case.plan()
    ch = K.Chunk(case.name, case.ptype, optional=case.optional, layout=K.LAYOUTS["e"])
    if p["dict"] is not None:
        raw = p["dict_bytes"]
        ch.dict = K.dict_page_header(len(p["dict"]), K.PLAIN, len(raw), len(raw)) + raw
        ch.usize += len(ch.dict)
        ch.encodings.add(K.PLAIN)
    for pg in p["pages"]:
        body = pg["levels"] + pg["values"]
        hdr = K.v2_page_header(pg["rows"], pg["nulls"], pg["rows"], p["encoding"], len(pg["levels"]), 0, None, len(body), len(body))
        ch.pages.append(hdr + body)
        ch.value_spans.append((len(hdr) + len(pg["levels"]), len(pg["values"])))
        ch.usize += len(hdr) + len(body)
        ch.encodings.update({p["encoding"], K.RLE})
        ch.num_entries += pg["rows"]
    return ch


# ---------------------------------------------------------------- a reader of page headers (Thrift compact)
def _uv(buf, pos):
    v, sh = 0, 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << sh
        sh += 7
        if not b & 0x80:
            return v, pos


def _value(buf, pos, t):
    if t in (1, 2):
        return t == 1, pos
    if t == 3:
        return buf[pos], pos + 1
    if t in (4, 5, 6):
        z, pos = _uv(buf, pos)
        return (z >> 1) ^ -(z & 1), pos
    if t == 7:
        return bytes(buf[pos:pos + 8]), pos + 8
    if t == 8:
        n, pos = _uv(buf, pos)
        return bytes(buf[pos:pos + n]), pos + n
    if t in (9, 10):
        h = buf[pos]
        pos += 1
        n, et = h >> 4, h & 15
        if n == 15:
            n, pos = _uv(buf, pos)
        out = []
        for _ in range(n):
            if et in (1, 2):
                v, pos = buf[pos] == 1, pos + 1
            else:
                v, pos = _value(buf, pos, et)
            out.append(v)
        return out, pos
    if t == 12:
        return _struct(buf, pos)
    raise ValueError(f"Thrift compact type {t}")


def _struct(buf, pos):
    out, last = {}, 0
    while True:
        b = buf[pos]
        pos += 1
        if b == 0:
            return out, pos
        t, delta = b & 15, b >> 4
        if delta:
            fid = last + delta
        else:
            z, pos = _uv(buf, pos)
            fid = (z >> 1) ^ -(z & 1)
        last = fid
        out[fid], pos = _value(buf, pos, t)


def read_pages(chunk):
    """The pages of a column chunk's bytes: [{"at", "header_len", "type", "usize", "csize", "body", and of a v2 data
    page "num_values", "num_nulls", "num_rows", "encoding", "def_bytes", "rep_bytes", "is_compressed", of a dictionary
    page "num_values", "encoding", and "crc" / "statistics" where the header has them}]."""
    pages, pos = [], 0
    while pos < len(chunk):
        h, body_at = _struct(chunk, pos)
        pg = {"at": pos, "header_len": body_at - pos, "type": h[1], "usize": h[2], "csize": h[3],
              "body": bytes(chunk[body_at:body_at + h[3]]), "crc": h.get(4)}
        assert body_at + h[3] <= len(chunk), "page body runs past the chunk"
        if h[1] == PAGE_DICTIONARY:
            pg.update(num_values=h[7][1], encoding=h[7][2])
        elif h[1] == PAGE_DATA_V2:
            v2 = h[8]
            pg.update(num_values=v2[1], num_nulls=v2[2], num_rows=v2[3], encoding=v2[4], def_bytes=v2[5], rep_bytes=v2[6],
                      is_compressed=v2.get(7, True), statistics=v2.get(8))
        else:
            raise ValueError(f"page type {h[1]}")
        pages.append(pg)
        pos = body_at + h[3]
    return pages


# ---------------------------------------------------------------- cases
def _rng(*key):
    return np.random.default_rng(sum(ord(c) * (i + 7) for i, c in enumerate("/".join(map(str, key)))))


def _distinct_int32(d):
    return (np.arange(d, dtype=np.int64) * 2654435761 % (1 << 31)).astype(np.int32)      # odd multiplier mod 2^31: distinct


def _shuffled_with_repeats(pool_size, m, rng):
    """m picks of 0..pool_size-1: every one at least once, shuffled, the rest random repeats."""
    assert m >= pool_size
    picks = np.concatenate([np.arange(pool_size), rng.integers(0, pool_size, m - pool_size)])
    rng.shuffle(picks)
    return picks


def _sweep_case(d):
    """INT32, exactly d distinct present values (ids of id_width(d) bits), pages of 1,000 rows with a few nulls
    each, so that pages end with 1..7 ids in their last group."""
    rng = _rng("sweep", d)
    rows = 5000 if d <= 1025 else int(d * 1.13) + 1000
    present = rng.random(rows) >= (0.1 if d <= 1025 else 0.05)
    m = int(present.sum())
    dense = _distinct_int32(d)[_shuffled_with_repeats(d, m, rng)]
    return Case(f"sweep_d{d}", K.INT32, dense, present=present, page_rows=1000, dict_page_limit=(4 << 20) if d > (1 << 18) else 0)


SWEEP_D = [1, 2, 3, 4, 5] + [x for k in range(3, 18) for x in (1 << k, (1 << k) + 1)] + [(1 << 18) + 1, (1 << 19) + 1]


def _pool(ptype, key):
    """The values of a type that dictionaries get wrong."""
    if ptype == K.INT32:
        return np.array([0, -1, 1, -2**31 + 5000000, 2**31 - 1, -1000, 1000, 255, 256, -256, 65536, -65536], np.int32)
    if ptype == K.INT64:
        hi = [(k << 32) | 5 for k in range(1, 9)]                 # differ only in the high 32 bits
        lo = [(9 << 32) | k for k in range(8)]                    # differ only in the low 32 bits
        return np.array(hi + lo + [0, -1, 5, 2**63 - 1, -2**62], np.int64)
    if ptype in (K.FLOAT, K.DOUBLE):
        f32 = ptype == K.FLOAT
        nans = [0x7fc00001, 0x7fc00002, 0xffc00000] if f32 else [0x7ff8000000000001, 0x7ff8000000000002, 0xfff8000000000000]
        plain = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1.5, 3.25], np.float32 if f32 else np.float64)
        return np.concatenate([plain, np.array(nans, np.uint32 if f32 else np.uint64).view(plain.dtype)])
    if ptype == K.BOOLEAN:
        return np.array([0, 1], np.uint8)
    assert ptype == K.BYTE_ARRAY
    big = bytes(_rng("big", key).integers(0, 256, 100_000, dtype=np.uint8))
    return [b"", b"a", b"ab", b"abc", b"abcd", b"c", b"bc", b"a\x00", b"a\x00b", b"\x00", b"\x00\x00", b"same-length-0",
            b"same-length-1", b"x" * 300, b"x" * 299 + b"y", big]


def _values(ptype, m, key):
    """m present values over the type's pool: each at least once where m allows, shuffled, with repeats."""
    pool = _pool(ptype, key)
    rng = _rng("values", ptype, m, key)
    if ptype == K.BYTE_ARRAY and m > 40:
        # "ab","c" next to "a","bc" (the same bytes, cut differently), the 100 KB string twice, the others as often as it takes
        k = m - 4
        picks = np.concatenate([np.arange(len(pool)), [len(pool) - 1], rng.integers(0, len(pool) - 1, k - len(pool) - 1)])
        rng.shuffle(picks)
        return [b"ab", b"c", b"a", b"bc"] + [pool[i] for i in picks]
    if m >= len(pool):
        picks = _shuffled_with_repeats(len(pool), m, rng)
    else:
        picks = rng.integers(0, len(pool) - (1 if ptype == K.BYTE_ARRAY else 0), m)
    return [pool[i] for i in picks] if ptype == K.BYTE_ARRAY else pool[picks]


TYPES = {"bool": K.BOOLEAN, "i32": K.INT32, "i64": K.INT64, "f32": K.FLOAT, "f64": K.DOUBLE, "ba": K.BYTE_ARRAY}
N_ROWS, PAGE = 3003, 1000          # three pages of 1,000 rows and a last page of 3


def _patterns(rows=N_ROWS):
    rng = _rng("patterns", rows)
    ones = np.ones(rows, bool)
    out = {"alternating": np.arange(rows) % 2 == 0, "nulls30": rng.random(rows) >= 0.3, "allnull": np.zeros(rows, bool)}
    for name, (a, b) in {"firstpagenull": (0, PAGE), "middlepagenull": (PAGE, 2 * PAGE), "trailingnulls": (2 * PAGE + 500, rows)}.items():
        out[name] = ones.copy()
        out[name][a:b] = False
    return out


def _typed(tname, pattern, mask, **kw):
    ptype = TYPES[tname]
    route = "plain" if kw.get("dictionary") is False else "dict"
    name = f"{tname}_{route}_{pattern}"
    if pattern == "required":
        return Case(name, ptype, _values(ptype, N_ROWS, name), page_rows=PAGE, **kw)
    if pattern == "novalidity":
        return Case(name, ptype, _values(ptype, N_ROWS, name), optional=True, send_validity=False, page_rows=PAGE, **kw)
    return Case(name, ptype, _values(ptype, int(mask.sum()), name), present=mask, page_rows=PAGE, **kw)


def _type_cases():
    out = []
    pats = dict(_patterns(), required=None, novalidity=None)
    for tname in TYPES:                               # every type through the dictionary, every null pattern on both routes
        for pattern, mask in pats.items():
            if tname in ("i32", "f64", "ba", "bool") or pattern in ("required", "nulls30"):
                out.append(_typed(tname, pattern, mask))
            out.append(_typed(tname, pattern, mask, dictionary=False))
    return out


def _edge_cases():
    out = []
    for tname, ptype in TYPES.items():                # n = 0 and n = 1, present and null
        for route, kw in (("dict", {}), ("plain", {"dictionary": False})):
            one = _values(ptype, 1, "one")
            out.append(Case(f"{tname}_{route}_n0_required", ptype, one[:0], **kw))
            out.append(Case(f"{tname}_{route}_n0_optional", ptype, one[:0], present=np.zeros(0, bool), **kw))
            out.append(Case(f"{tname}_{route}_n1_required", ptype, one, **kw))
            out.append(Case(f"{tname}_{route}_n1_present", ptype, one, present=np.ones(1, bool), **kw))
            out.append(Case(f"{tname}_{route}_n1_null", ptype, one[:0], present=np.zeros(1, bool), **kw))
    # page_rows 8, 1001 (pages of 1,008 rows) and the default (one page here, three in r45000)
    mask = _patterns()["nulls30"]
    for pr in (8, 1001, 0):
        for tname in ("i32", "ba"):
            out.append(Case(f"{tname}_pagerows{pr}", TYPES[tname], _values(TYPES[tname], int(mask.sum()), f"pr{pr}"), present=mask, page_rows=pr))
    rng = _rng("r45000")
    mask = rng.random(45000) >= 0.3
    out.append(Case("i32_default_pages", K.INT32, _distinct_int32(700)[rng.integers(0, 700, int(mask.sum()))], present=mask))
    out.append(Case("f32_default_pages_plain", K.FLOAT, rng.random(int(mask.sum())).astype(np.float32), present=mask, dictionary=False))
    # dict_page_limit: the dictionary's own size stays a dictionary, one byte less is PLAIN
    for tname in ("i32", "i64", "ba"):
        ptype = TYPES[tname]
        dense = _values(ptype, 2000, "limit")
        size = Case("probe", ptype, dense).plan()
        size = len(size["dict_bytes"])
        w = K.width_of(ptype)
        assert size == (len(_pool(ptype, "limit")) * w if w else sum(4 + len(x) for x in set(dense)))
        for name, limit in (("at", size), ("under", size - 1)):
            out.append(Case(f"{tname}_limit_{name}", ptype, dense, present=np.ones(2000, bool), page_rows=PAGE, dict_page_limit=limit))
            assert out[-1].plan()["fallback"] == (0 if name == "at" else 1)
    return out


_CACHE = {}


def _all():
    if "files" not in _CACHE:
        files = {}
        for c in [_sweep_case(d) for d in SWEEP_D] + _type_cases() + _edge_cases():
            files.setdefault(f"r{c.rows}", []).append(c)
        for fid, cases in files.items():
            assert len({c.name for c in cases}) == len(cases), fid
        _CACHE["files"] = files
    return _CACHE["files"]


def file_cases(fid):
    """(rows, cases) of a file; built once and shared (callers must not modify the arrays)."""
    return int(fid[1:]), _all()[fid]


FILE_IDS = tuple(sorted(_all(), key=lambda f: int(f[1:])))
