"""Hand-assembled Thrift compact PageHeaders and the column-chunk cases built with them (pure Python +
numpy; TEST INFRASTRUCTURE ONLY).

Every other page header of the suite comes out of a writer (pyarrow, pagekit, the product's own), which
emits the fields in one order, in short form, as i32, with no unknown fields. Here a header is an explicit
field tree (F): any order, short or long field headers, integers as i8 / i16 / i32 / i64, padded varints,
unknown fields of every Thrift type. No product code and no parser is involved in an expectation: a case
carries the pf_page_desc records (include/pfloor.h) or the (status, err_page) that follow from how it was
put together. test_scan_headers.py asks the host walk (pf_file_chunk_desc), the oracle (pfo_chunk_pages)
and the GPU scan (pf_scan_pages) for the same.

The constants a case guards are named next to it (SCAN_STG, SCAN_MARGIN of csrc/pf_scan.hip,
PF_THRIFT_MAX_NESTING of pfloor.h: today's values, a retune moves the case with the constant).

valid_cases() / invalid_cases() / huge_count_cases() return Case lists; mutants(case) the one-byte damages
of a valid case. Nothing that goes to the GPU carries a container count above MAX_GPU_COUNT: container_counts()
reparses a chunk with this module's own reader and the case tables and mutants() assert the bound, so no
wave can be kept busy beyond microseconds whatever a parser does. Counts near 2^63 are in huge_count_cases()
only, which are CPU cases (gpu = False)."""
import functools
import struct
import zlib

import numpy as np

from pagekit import _T, _uvarint

OK, CORRUPT, CAPACITY = 0, -2, -6            # PF_OK, PF_ERR_CORRUPT_PAGE, PF_ERR_CAPACITY
PAGE_FIELDS = ("offset", "compressed_size", "uncompressed_size", "page_type", "encoding", "def_encoding",
               "rep_encoding", "num_values", "num_nulls", "num_rows", "def_bytes", "rep_bytes", "is_compressed")
SCAN_STG, SCAN_MARGIN = 512, 16              # csrc/pf_scan.hip
MAX_NEST = 16                                # PF_THRIFT_MAX_NESTING (pfloor.h)
MAX_GPU_COUNT = 1 << 16
MUTANT_MAX_CHUNK = 4096                      # larger chunks (the 64 KiB CRC bodies) get no mutants
FILL = 0xA5                                  # long binary payloads are runs of this byte (see _opaque)
DATA, INDEX, DICT, DATA_V2 = 0, 1, 2, 3
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- value encoders
def uvarint(v, pad=0):
    """LEB128 of v; pad > 0: exactly `pad` bytes (redundant continuation bytes, as 0x85 0x80 0x00 for 5)."""
    out = bytearray(_uvarint(v))
    if pad:
        assert len(out) <= pad
        while len(out) < pad:
            out[-1] |= 0x80
            out.append(0)
    return bytes(out)


def zz(v):
    return ((v << 1) ^ (v >> 63)) & M64


def e_int(v, t=5, pad=0):
    """An integer of compact type 3 (one byte) or 4 / 5 / 6 (zigzag varint)."""
    assert t in (3, 4, 5, 6)
    if t == 3:
        assert -128 <= v <= 127
        return bytes([v & 0xFF])
    return uvarint(zz(v), pad)


def e_bin(data, pad=0):
    return uvarint(len(data), pad) + data


def e_bool(v):
    """A bool inside a list, set or map: one byte (libthrift writeBool outside a field header)."""
    return b"\x01" if v else b"\x02"


def e_double(x):
    return struct.pack("<d", x)


def e_list(et, elems, long=False, count=None):
    """A list / set of element type et; short header below 15 elements unless long. count: the count
    written, when it is not len(elems)."""
    n = len(elems) if count is None else count
    hdr = bytes([(n << 4) | et]) if n < 15 and not long else bytes([0xF0 | et]) + uvarint(n)
    return hdr + b"".join(elems)


def e_map(kt, vt, pairs, count=None):
    """A map; the empty map is its count alone, without the key / value type byte."""
    n = len(pairs) if count is None else count
    if n == 0:
        return b"\x00"
    return uvarint(n) + bytes([(kt << 4) | vt]) + b"".join(k + v for k, v in pairs)


class TW(_T):
    """pagekit's struct writer with explicit field-header form and every value type."""

    def _hdr(self, fid, t, long=False):
        d = fid - self.last[-1]
        if not long and 0 < d <= 15:
            self.b.append((d << 4) | t)
        else:
            self.b.append(t)
            self.b += uvarint(zz(fid) & 0xFFFFFFFF)
        self.last[-1] = ((fid + 0x8000) & 0xFFFF) - 0x8000      # a reader keeps the id as i16

    def field(self, fid, t, payload=b"", long=False):
        self._hdr(fid, t, long)
        self.b += payload
        return self

    def integer(self, fid, v, t=5, pad=0, long=False):
        return self.field(fid, t, e_int(v, t, pad), long)

    def double(self, fid, x, long=False):
        return self.field(fid, 7, e_double(x), long)

    def binary(self, fid, data, pad=0, long=False):
        return self.field(fid, 8, e_bin(data, pad), long)

    def list_(self, fid, et, elems, long=False, set_=False):
        return self.field(fid, 10 if set_ else 9, e_list(et, elems, long))

    def map_(self, fid, kt, vt, pairs):
        return self.field(fid, 11, e_map(kt, vt, pairs))

    def struct(self, fid, fields, long=False):
        return self.field(fid, 12, e_struct(fields), long)


class F:
    """One field of a struct under construction: an integer (val, written as type t, varint padded to
    pad bytes), a struct (sub: its fields), or anything else as its encoded payload."""

    def __init__(self, fid, t, payload=b"", val=None, sub=None, long=False, pad=0):
        self.fid, self.t, self.payload, self.val, self.sub, self.long, self.pad = fid, t, payload, val, sub, long, pad

    def emit(self, w):
        if self.sub is not None:
            p = e_struct(self.sub)
        elif self.val is not None:
            p = e_int(self.val, self.t, self.pad)
        else:
            p = self.payload
        w.field(self.fid, self.t, p, self.long)


def e_struct(fields):
    w = TW()
    for f in fields:
        f.emit(w)
    return w.done()


def I(fid, v, t=5, pad=0):
    return F(fid, t, val=v, pad=pad)


def B(fid, data, pad=0):
    return F(fid, 8, e_bin(data, pad))


def S(fid, fields):
    return F(fid, 12, sub=list(fields))


def nest(d):
    """A struct value with d containers open at its deepest point (itself included): structs in field 1."""
    return b"\x1c" * (d - 1) + b"\x00" * d


def nest_mixed(d):
    """A list value with d containers open at its deepest point: list<struct{1: list<struct{...}>}>."""
    if d == 1:
        return e_list(5, [e_int(7)])
    if d == 2:
        return b"\x1c" + b"\x00"
    return b"\x1c" + b"\x19" + nest_mixed(d - 2) + b"\x00"


# ---------------------------------------------------------------- unknown fields of every type
def _unknown_kinds():
    i32s = [e_int(x) for x in (1, -1, 300, 2**31 - 1, -2**31)]
    return [
        ("true", 1, b""), ("false", 2, b""), ("byte", 3, b"\x9c"), ("i16", 4, e_int(-1234)),
        ("i32", 5, e_int(2**31 - 1)), ("i64", 6, e_int(-2**62)), ("double", 7, e_double(-0.5)),
        ("bin0", 8, e_bin(b"")), ("bin1", 8, e_bin(b"\x00")), ("bin600", 8, e_bin(bytes([FILL]) * 600)),
        ("list_i32_3", 9, e_list(5, i32s[:3])), ("list_i32_3_long", 9, e_list(5, i32s[:3], long=True)),
        ("list_i32_20", 9, e_list(5, i32s * 4)),
        ("list_bool", 9, e_list(1, [e_bool(1), e_bool(0), b"\x00", e_bool(1)])),
        ("list_bool2", 9, e_list(2, [e_bool(0), e_bool(1)])),
        ("list_struct", 9, e_list(12, [e_struct([I(1, 7), B(2, b"ab")]), e_struct([]), e_struct([F(3, 1)])])),
        ("list_list_bin", 9, e_list(9, [e_list(8, [e_bin(b"x"), e_bin(b"")]), e_list(8, [])])),
        ("set_i64", 10, e_list(6, [e_int(2**62), e_int(-1), e_int(0)])),
        ("map_i32_bin", 11, e_map(5, 8, [(e_int(1), e_bin(b"one")), (e_int(-2), e_bin(b""))])),
        ("map_empty", 11, e_map(5, 8, [])),
        # bool bytes other than 1 / 2 are still one byte each (libthrift: readByte() == 1); a 0x00 among them
        # reads as STOP to a parser that skipped nothing
        ("map_bool_bool", 11, e_map(1, 1, [(e_bool(1), e_bool(0)), (b"\x00", e_bool(1)), (e_bool(0), b"\x1c")])),
        ("map_bool_i32", 11, e_map(2, 5, [(e_bool(1), e_int(300)), (e_bool(0), e_int(-1)), (b"\x00", e_int(0))])),
        ("map_i32_bool", 11, e_map(5, 1, [(e_int(5), e_bool(1)), (e_int(6), b"\x00")])),
        ("struct", 12, e_struct([I(1, 5), S(2, [B(1, b"q")]), F(3, 2)])),
        ("nest_limit", 12, nest(MAX_NEST)),
        ("nest_mixed_limit", 9, nest_mixed(MAX_NEST)),
    ]


UNKNOWN = _unknown_kinds()
# where an unknown field goes: the first id parquet.thrift leaves free in each struct, and ids further out
UNKNOWN_IDS = {"page": (9, 100, 6), "v1": (6, 17, 300), "v2": (9, 40, 2000), "dict": (4, 21, 130), "stats": (7, 9, 32767)}


# ---------------------------------------------------------------- pages
class Page:
    """A page: header fields (F tree), body bytes, and the descriptor the walk must produce for it
    (desc, without `offset`; None for a page the walk skips)."""

    def __init__(self, fields, body, desc, has_crc=False, nv=0):
        self.fields, self.body, self.desc, self.has_crc, self.nv = fields, body, desc, has_crc, nv

    def sub(self, fid=None):
        """The fields of the page's type-specific header struct."""
        for f in self.fields:
            if f.sub is not None and (fid is None or f.fid == fid):
                return f.sub
        raise KeyError(fid)

    def header(self):
        return e_struct(self.fields)


def _desc(ptype, usize, csize, nv, enc, def_enc=0, rep_enc=0, nulls=-1, rows=0, defb=0, repb=0, comp=1):
    return dict(compressed_size=csize & 0xFFFFFFFF, uncompressed_size=usize & 0xFFFFFFFF, page_type=ptype, encoding=enc,
                def_encoding=def_enc, rep_encoding=rep_enc, num_values=nv, num_nulls=nulls, num_rows=rows,
                def_bytes=defb, rep_bytes=repb, is_compressed=comp)


def _crc_field(crc, crc_t):
    """PageHeader.crc (field 4): the CRC32 as a signed i32, so values >= 2^31 are negative."""
    return I(4, crc - (1 << 32) if crc >= 1 << 31 else crc, t=crc_t)


def _top(ptype, body, usize, csize, crc, crc_t):
    csize = len(body) if csize is None else csize
    usize = len(body) + 7 if usize is None else usize
    f = ([] if ptype is None else [I(1, ptype)]) + [I(2, usize), I(3, csize)]
    if crc is not None:
        crc = zlib.crc32(body) if crc is True else crc
        f.append(_crc_field(crc, crc_t))
    return f, usize, csize, crc is not None and crc_t == 5


def dict_page(body, n, enc=0, usize=None, csize=None, crc=None, crc_t=5):
    f, usize, csize, has = _top(DICT, body, usize, csize, crc, crc_t)
    f.append(S(7, [I(1, n), I(2, enc), F(3, 2)]))
    return Page(f, body, _desc(DICT, usize, csize, n, enc), has)


def v1_page(body, nv, enc=0, def_enc=3, rep_enc=4, stats=None, nulls=-1, usize=None, csize=None, crc=None, crc_t=5):
    """stats: the fields of DataPageHeader.statistics (field 5); nulls: the num_nulls they amount to."""
    f, usize, csize, has = _top(DATA, body, usize, csize, crc, crc_t)
    sub = [I(1, nv), I(2, enc), I(3, def_enc), I(4, rep_enc)]
    if stats is not None:
        sub.append(S(5, stats))
    f.append(S(5, sub))
    return Page(f, body, _desc(DATA, usize, csize, nv, enc, def_enc, rep_enc, nulls), has, nv)


def v2_page(body, nv, nulls=0, rows=None, enc=0, defb=0, repb=0, comp=None, stats=None, usize=None, csize=None, crc=None,
            crc_t=5):
    f, usize, csize, has = _top(DATA_V2, body, usize, csize, crc, crc_t)
    rows = nv if rows is None else rows
    sub = [I(1, nv), I(2, nulls), I(3, rows), I(4, enc), I(5, defb), I(6, repb)]
    if comp is not None:
        sub.append(F(7, 1 if comp else 2))
    if stats is not None:
        sub.append(S(8, stats))
    f.append(S(8, sub))
    return Page(f, body, _desc(DATA_V2, usize, csize, nv, enc, 0, 0, nulls, rows, defb, repb, 1 if comp is None else int(comp)),
                has, nv)


def skipped_page(body, ptype, sub_id=None, sub=(), crc=None):
    """A page the walk passes over: INDEX_PAGE, an unknown type, or no type field at all (ptype None)."""
    f, _, _, _ = _top(ptype, body, None, None, crc, 5)
    if sub_id is not None:
        f.append(S(sub_id, sub))
    return Page(f, body, None)


# ---------------------------------------------------------------- transforms of a field tree
def each_struct(fields, fn):
    """fn(list of F) on the struct and on every struct below it."""
    fn(fields)
    for f in fields:
        if f.sub is not None:
            each_struct(f.sub, fn)


def reorder(page, how, rng=None):
    """Reverse or shuffle the fields of the header and of every struct in it."""
    def go(fs):
        if how == "reverse":
            fs.reverse()
        else:
            fs[:] = [fs[i] for i in rng.permutation(len(fs))]
    each_struct(page.fields, go)
    return page


def force_long(page):
    def go(fs):
        for f in fs:
            f.long = True
    each_struct(page.fields, go)
    return page


def retype(page, t, pad=0, keep=()):
    """Write every integer field as type t (varints padded to pad bytes), except PageHeader ids in keep."""
    def go(fs, top):
        for f in fs:
            if f.val is not None and not (top and f.fid in keep):
                f.t, f.pad = t, pad
            if f.sub is not None:
                go(f.sub, False)
    go(page.fields, True)
    return page


def insert(fields, at, f):
    fields.insert(min(at, len(fields)), f)


# ---------------------------------------------------------------- cases
class Case:
    """One column chunk. pages: the descriptors of the pages found before the walk ends (all of them when
    status is OK). With verify_crc, status / err_page are crc_status / crc_err_page when those are set."""

    def __init__(self, group, name, pages, num_values=None, trailing=b"", status=OK, err_page=-1, page_cap=None,
                 gpu=True, crc_bad=None, cut=None):
        self.group, self.name, self.gpu = group, name, gpu
        data = bytearray()
        self.pages, self.has_crc, self.headers = [], [], []
        nv = 0
        for p in pages:
            h = p.header()
            self.headers.append((len(data), len(data) + len(h)))
            data += h
            if p.desc is not None:
                self.pages.append(dict(p.desc, offset=len(data)))
                self.has_crc.append(int(p.has_crc))
                nv += p.nv
            data += p.body
        if cut is not None:
            data = data[:cut]
        self.data = bytes(data) + trailing
        self.num_values = nv if num_values is None else num_values
        self.status, self.err_page = status, err_page
        if status != OK:
            self.pages, self.has_crc = self.pages[:self.n_found()], self.has_crc[:self.n_found()]
        self.page_cap = len(self.pages) + (status != OK) if page_cap is None else page_cap
        self.crc_status, self.crc_err_page = (CORRUPT, crc_bad) if crc_bad is not None else (status, err_page)

    def n_found(self):
        """Header, bounds and capacity errors stop the walk at the page they name."""
        return self.err_page if self.status != OK else len(self.pages)

    @property
    def n_pages(self):
        return len(self.pages)

    def crc_pages(self):
        return sum(self.has_crc)

    def __repr__(self):
        return f"{self.group}/{self.name}"


def _body(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _trio(rng, crc=True):
    """The base layout: a dictionary page, a v1 page with statistics and a v2 page."""
    stats = [B(1, b"zz"), B(2, b"aa"), I(3, 4, t=6), I(4, 9, t=6)]
    return [dict_page(_body(rng, 40), 10, enc=2, crc=crc),
            v1_page(_body(rng, 61), 50, enc=8, stats=stats, nulls=4, crc=crc),
            v2_page(_body(rng, 90), 33, nulls=5, rows=30, enc=8, defb=6, repb=3, comp=True, crc=crc)]


def _valid_order(rng):
    out = [Case("order", "natural", _trio(rng))]
    out.append(Case("order", "reversed", [reorder(p, "reverse") for p in _trio(rng)]))
    for seed in (1, 2, 3):
        r = np.random.default_rng(seed)
        out.append(Case("order", f"shuffled{seed}", [reorder(p, "shuffle", r) for p in _trio(rng)]))
    out.append(Case("order", "long_form", [force_long(p) for p in _trio(rng)]))
    out.append(Case("order", "long_form_reversed", [force_long(reorder(p, "reverse")) for p in _trio(rng)]))
    return out


def _valid_ints(rng):
    """type, sizes, num_values (and every other integer but crc, which counts only as i32) as i8 / i16 / i32 /
    i64, varints minimal and padded to 5 and 10 bytes. Bodies and counts below 120 so that i8 holds them."""
    out = []
    for t in (3, 4, 5, 6):
        for pad in ((0,) if t == 3 else (0, 5, 10)):
            stats = [I(3, 17)]
            pages = [v1_page(_body(rng, 20), 100, enc=0, stats=stats, nulls=17, usize=99),
                     v2_page(_body(rng, 113), 27, nulls=3, rows=20, enc=5, defb=9, repb=2, comp=False, usize=120),
                     v1_page(_body(rng, 3), 1, usize=3)]
            out.append(Case("ints", f"t{t}_pad{pad}", [retype(p, t, pad) for p in pages]))
    # negative values survive every width: encodings are not validated by the walk
    pages = [v1_page(_body(rng, 9), 5, enc=-1, def_enc=-128, rep_enc=127)]
    out.append(Case("ints", "negative_i8", [retype(p, 3) for p in pages]))
    return out


def _unknown_page(rng, where, kind, k):
    name, t, payload = kind
    fid = UNKNOWN_IDS[where][k % 3]
    if where == "page" and fid == 6 and t != 12:
        fid = 9                                     # field 6 is index_page_header: only a struct goes there
    u = F(fid, t, payload)
    if where == "v2":
        p = v2_page(_body(rng, 30 + k), 10 + k, nulls=1, defb=2, repb=1, stats=[B(1, b"m"), I(3, 77, t=6)])
        insert(p.sub(8), k % 8, u)
    elif where == "dict":
        p = dict_page(_body(rng, 30 + k), 10 + k)
        insert(p.sub(7), k % 4, u)
    else:
        p = v1_page(_body(rng, 30 + k), 10 + k, stats=[B(2, b"lo"), I(3, k, t=6), B(1, b"hi")], nulls=k)
        if where == "page":
            insert(p.fields, k % 5, u)
        elif where == "v1":
            insert(p.sub(5), k % 6, u)
        else:
            insert([f for f in p.sub(5) if f.fid == 5][0].sub, k % 4, u)
    return p


def _valid_unknown(rng):
    """An unknown field of every type in PageHeader, DataPageHeader, DataPageHeaderV2, DictionaryPageHeader and
    v1 Statistics, at every position among the known fields (so ids go down as well as up)."""
    out = []
    for where in ("page", "v1", "v2", "stats"):
        for g in range(0, len(UNKNOWN), 5):
            kinds = UNKNOWN[g:g + 5]
            pages = [_unknown_page(rng, where, kind, g + i) for i, kind in enumerate(kinds)]
            out.append(Case("unknown", f"{where}_" + "+".join(k[0] for k in kinds), pages))
    for g in range(0, len(UNKNOWN), 5):       # a chunk has one dictionary page: five unknown fields in its header
        kinds = UNKNOWN[g:g + 5]
        p = dict_page(_body(rng, 30), 10 + g)
        for i, (_, t, payload) in enumerate(kinds):
            insert(p.sub(7), (g + 2 * i) % (4 + i), F(4 + 9 * i, t, payload))
        out.append(Case("unknown", "dict_" + "+".join(k[0] for k in kinds), [p, v1_page(_body(rng, 8), 3)]))
    return out


def _fit(make, total, length_of):
    """make(n) with n chosen so that length_of(make(n), n) == total (the varints that state n may grow with it)."""
    n = max(1, total - 64)
    for _ in range(6):
        p = make(n)
        if length_of(p, n) == total:
            return p
        n += total - length_of(p, n)
    raise AssertionError(total)


def _stats_after(rng, target, which, null_first):
    """A chunk whose first page is a v1 page with Statistics in which the byte after the long min / max binary
    (which: 1 max, 2 min) is byte `target` of the chunk, and so of the first staging window. null_count comes
    first, or right after that binary."""
    def build(n):
        nc = I(3, 1000 + target, t=6)
        stats = ([nc] if null_first else []) + [B(3 - which, b"s"), B(which, bytes([FILL]) * n)] + ([] if null_first else [nc])
        return v1_page(_body(rng, 25), 12, enc=8, stats=stats, nulls=1000 + target)
    p = _fit(build, target, lambda p, n: p.header().index(bytes([FILL]) * n) + n)
    return [p, v2_page(_body(rng, 40), 8, nulls=2, defb=3)]


def _valid_stats(rng):
    out = []
    mk = lambda stats, nulls: [v1_page(_body(rng, 30), 20, stats=stats, nulls=nulls), v2_page(_body(rng, 12), 5)]
    mm = [B(1, b"maximum"), B(2, b"min")]
    out.append(Case("stats", "null_count_first", mk([I(3, 6, t=6)] + mm, 6)))
    out.append(Case("stats", "null_count_last", mk(mm + [I(3, 6, t=6)], 6)))
    out.append(Case("stats", "null_count_absent", mk(mm + [I(4, 6, t=6)], -1)))
    out.append(Case("stats", "null_count_int32_max", mk(mm + [I(3, 2**31 - 1, t=6)], 2**31 - 1)))
    out.append(Case("stats", "null_count_2p31", mk(mm + [I(3, 2**31, t=6)], -1)))
    out.append(Case("stats", "null_count_2p40", mk([I(3, 2**40, t=6)] + mm, -1)))
    out.append(Case("stats", "null_count_negative", mk(mm + [I(3, -5, t=6)], -1)))
    out.append(Case("stats", "null_count_i8", mk(mm + [I(3, 100, t=3)], 100)))
    out.append(Case("stats", "empty", mk([], -1)))
    out.append(Case("stats", "all_six", mk([B(1, b"b"), B(2, b"a"), I(3, 2, t=6), I(4, 3, t=6), B(5, b"bb"), B(6, b"aa")], 2)))
    # DataPageHeaderV2.statistics (field 8) is skipped: num_nulls is the header's own field 2
    out.append(Case("stats", "v2_stats_skipped",
                    [v2_page(_body(rng, 50), 21, nulls=4, defb=5, stats=[B(1, b"x" * 40), I(3, 999, t=6), B(2, b"")]),
                     v1_page(_body(rng, 5), 2)]))
    # the byte after a long min / max on every offset around the end of the staging window (SCAN_STG = 512, restage
    # at SCAN_STG - SCAN_MARGIN = 496): advance() past the window, then a restage
    for target in list(range(SCAN_STG - 32, SCAN_STG + 19)) + [2000]:
        out.append(Case("stats_sweep", f"after_{target}", _stats_after(rng, target, 1 + target % 2, target % 3 == 0)))
    return out


def _valid_window(rng):
    """The second header starts at window offsets 490..515: up to 495 it is parsed from the first window and
    restaged on the way (at 496); from 496 on the page loop restages first."""
    out = []
    for start in range(SCAN_STG - SCAN_MARGIN - 6, SCAN_STG + 4):
        p0 = _fit(lambda n: v1_page(_body(rng, n), 7), start, lambda p, n: len(p.header()) + n)
        p1 = v2_page(_body(rng, 60), 9, nulls=1, rows=9, enc=8, defb=4, repb=0, comp=False, stats=[B(1, b"q" * 20), B(2, b"")], crc=True)
        out.append(Case("window", f"start_{start}", [p0, p1, v1_page(_body(rng, 10), 4, stats=[I(3, 1, t=6)], nulls=1)]))
    return out


def _valid_kinds(rng):
    out = []
    out.append(Case("kinds", "dict_v1_v2_compressed_flags",
                    [dict_page(_body(rng, 33), 6), v1_page(_body(rng, 40), 10), v2_page(_body(rng, 41), 11, comp=True),
                     v2_page(_body(rng, 42), 12, comp=False), v2_page(_body(rng, 43), 13, comp=None), v1_page(_body(rng, 4), 1)]))
    out.append(Case("kinds", "zero_values_in_the_middle",
                    [v1_page(_body(rng, 20), 5), v1_page(_body(rng, 6), 0), v2_page(_body(rng, 7), 0), v1_page(_body(rng, 9), 3)]))
    out.append(Case("kinds", "compressed_size_zero", [v1_page(b"", 5), v2_page(b"", 4, usize=0), v1_page(_body(rng, 9), 3)]))
    # INDEX_PAGE, page type 9 and no type field: skipped with their bodies, no slot, no values counted (the
    # DataPageHeader of the type-9 page says 1000 values)
    sk = lambda: [skipped_page(_body(rng, 20), INDEX, 6, []), skipped_page(_body(rng, 31), 9, 5, [I(1, 1000), I(2, 0)]),
                  skipped_page(_body(rng, 17), None, 5, [I(1, 1000)])]
    a, b, c = sk()
    out.append(Case("kinds", "skipped_between", [v1_page(_body(rng, 20), 5), a, v2_page(_body(rng, 12), 6), b, c, v1_page(_body(rng, 9), 3)]))
    a, b, c = sk()
    out.append(Case("kinds", "skipped_before_dict", [a, b, dict_page(_body(rng, 12), 3), c, v1_page(_body(rng, 9), 3)]))
    out.append(Case("kinds", "skipped_index_with_crc", [skipped_page(_body(rng, 20), INDEX, 6, [], crc=True), v1_page(_body(rng, 9), 3, crc=True)]))
    # garbage after the page that completes num_values is never read
    out.append(Case("kinds", "trailing_ff", [v1_page(_body(rng, 20), 5), v1_page(_body(rng, 9), 3)], trailing=b"\xff" * 64))
    out.append(Case("kinds", "trailing_truncated_header", [dict_page(_body(rng, 20), 5), v2_page(_body(rng, 9), 3)], trailing=b"\x15\x00\x15"))
    # libthrift keeps a field id as i16 (readI16 = (short) zigzagToInt(readVarint32())): id 65536 + 5 in long form is
    # data_page_header
    p = v1_page(_body(rng, 14), 9, enc=8)
    p.fields[-1].fid = 65536 + 5
    q = v2_page(_body(rng, 14), 9, nulls=2, defb=1)
    q.sub(8)[1].fid = 65536 + 2                         # num_nulls
    out.append(Case("kinds", "field_id_i16", [p, q, v1_page(_body(rng, 3), 1)]))
    # a count of exactly the remaining values, reached by the last page with nothing after it
    out.append(Case("kinds", "two_small", [v1_page(b"\x01", 1), v1_page(b"\x02", 1)]))
    return out


CRC_LENGTHS = (0, 1, 2, 255, 256, 257, 511, 512, 513, 1000, 65537)   # around k_page_crc's 256-thread segmentation


def _crc_pages(rng, fill):
    pages = []
    for i, n in enumerate(CRC_LENGTHS):
        body = _body(rng, n) if fill is None else bytes([fill]) * n
        pages.append(v1_page(body, 2, crc=True) if i % 2 == 0 else v2_page(body, 2, crc=True))
    return pages


def _valid_crc(rng):
    out = []
    b = _body(rng, 50)
    out.append(Case("crc", "absent_zero_i64",
                    [v1_page(_body(rng, 30), 4), v1_page(b"", 4, crc=True),          # zlib.crc32(b"") == 0
                     v2_page(b, 4, crc=True, crc_t=6),                              # an i64 crc is not PageHeader.crc: ignored
                     v1_page(b, 4, crc=True), v2_page(_body(rng, 9), 1, crc=True)]))
    out.append(Case("crc", "wrong_i64_crc_ignored", [v1_page(b, 4, crc=zlib.crc32(b) ^ 1, crc_t=6), v1_page(b, 2, crc=True)]))
    out.append(Case("crc", "dictionary_crc", [dict_page(_body(rng, 77), 5, crc=True), v1_page(_body(rng, 5), 2, crc=True)]))
    for name, fill in (("random", None), ("zeros", 0x00), ("ones", 0xFF)):
        out.append(Case("crc", f"lengths_{name}", _crc_pages(rng, fill)))
    crcs = [zlib.crc32(p.body) for p in _crc_pages(np.random.default_rng(5), None)]
    assert any(c >= 1 << 31 for c in crcs) and any(0 < c < 1 << 31 for c in crcs)
    # the same chunk with one page's crc off by one bit
    for bad, bit in ((0, 0), (3, 31), (4, 7), (7, 16), (10, 1)):
        pages = _crc_pages(np.random.default_rng(5), None)
        f = [f for f in pages[bad].fields if f.fid == 4][0]
        f.val = ((f.val & 0xFFFFFFFF) ^ (1 << bit))
        f.val -= (1 << 32) if f.val >= 1 << 31 else 0
        out.append(Case("crc_bad", f"page{bad}_bit{bit}", pages, crc_bad=bad))
    bad_dict = [dict_page(_body(rng, 77), 5, crc=True), v1_page(_body(rng, 5), 2, crc=True)]
    bad_dict[0].fields[3].val ^= 0x40
    out.append(Case("crc_bad", "dictionary", bad_dict, crc_bad=0))
    return out


@functools.lru_cache(maxsize=None)
def valid_cases():
    rng = np.random.default_rng(20)
    out = _valid_order(rng) + _valid_ints(rng) + _valid_unknown(rng) + _valid_stats(rng) + _valid_window(rng) + \
        _valid_kinds(rng) + _valid_crc(rng)
    for c in out:
        assert max(container_counts(c.data, c.num_values), default=0) <= MAX_GPU_COUNT, c
    assert len({repr(c) for c in out}) == len(out)
    return tuple(out)


def _invalid(rng):
    out = []
    good = lambda: v1_page(_body(rng, 20), 5)
    bad = lambda name, pages, err, **kw: out.append(Case("invalid", name, pages, status=CORRUPT, err_page=err, **kw))
    # a header truncated after each of its bytes (the chunk ends there): one case per byte; cut 0 is "the chunk ends
    # before num_values"
    p0, p1 = good(), v2_page(_body(rng, 10), 6, nulls=1, rows=6, enc=8, defb=2, repb=1, comp=True, crc=True)
    first = len(p0.header()) + len(p0.body)
    for k in range(len(p1.header())):
        bad(f"truncated_{k}", [p0, p1], 1, cut=first + k)
    bad("negative_compressed_size", [good(), v1_page(_body(rng, 9), 3, csize=-1)], 1)
    bad("compressed_size_int32_min", [v1_page(_body(rng, 9), 3, csize=-2**31)], 0)
    bad("body_past_chunk", [good(), good(), v1_page(_body(rng, 9), 3, csize=10)], 2)
    bad("body_far_past_chunk", [v2_page(_body(rng, 9), 3, csize=2**31 - 1, usize=2**31 - 1)], 0)
    bad("second_dictionary", [dict_page(_body(rng, 8), 2), good(), dict_page(_body(rng, 8), 2), good()], 2, num_values=10)
    bad("second_dictionary_at_once", [dict_page(_body(rng, 8), 2), dict_page(_body(rng, 8), 2), good()], 1)
    bad("dictionary_after_data", [good(), dict_page(_body(rng, 8), 2), good()], 1, num_values=10)
    bad("negative_num_values_v1", [good(), v1_page(_body(rng, 9), -3), good()], 1, num_values=10)
    bad("negative_num_values_v2", [v2_page(_body(rng, 9), -1), good()], 0, num_values=5)
    bad("v2_levels_above_compressed_size", [good(), v2_page(_body(rng, 9), 3, defb=6, repb=4, usize=100)], 1)
    bad("v2_levels_above_uncompressed_size", [good(), v2_page(_body(rng, 9), 3, defb=5, repb=4, usize=8)], 1)
    bad("v2_negative_def_bytes", [v2_page(_body(rng, 9), 3, defb=-1)], 0)
    bad("v2_negative_rep_bytes", [v2_page(_body(rng, 9), 3, repb=-1)], 0)
    p = good()
    p.fields[1] = F(2, 5, b"\x80" * 10 + b"\x00")
    bad("varint_11_bytes", [good(), p], 1, num_values=10)
    p = good()
    insert(p.fields, 2, F(9, 8, b"\xff" * 10 + b"\x00"))
    bad("binary_length_varint_11_bytes", [p], 0)
    for t in (0, 13, 14, 15):
        p = good()
        insert(p.fields, 3, F(9, t, b"\x00\x00"))
        bad(f"field_type_{t}", [good(), p], 1, num_values=10)
        p = good()
        insert(p.sub(5), 2, F(9, t, b"\x00\x00"))
        bad(f"field_type_{t}_in_data_page_header", [p], 0)
        p = good()
        insert(p.fields, 0, F(9, 9, e_list(t, [b"\x00"] * 2)))
        bad(f"list_element_type_{t}", [p], 0)
        p = good()
        insert(p.fields, 0, F(9, 11, e_map(5, t, [(e_int(1), b"\x00")])))
        bad(f"map_value_type_{t}", [p], 0)
    bad("chunk_ends_before_num_values", [good(), good()], 2, num_values=11)
    bad("skipped_page_ends_chunk", [good(), skipped_page(_body(rng, 9), INDEX, 6, [])], 1, num_values=6)
    bad("empty_chunk_wants_values", [], 0, num_values=1)
    # one container more than PF_THRIFT_MAX_NESTING inside a skipped value
    for name, t, payload in (("struct", 12, nest(MAX_NEST + 1)), ("mixed", 9, nest_mixed(MAX_NEST + 1))):
        p = good()
        insert(p.fields, 1, F(9, t, payload))
        bad(f"nesting_past_limit_{name}", [good(), p], 1, num_values=10)
        p = v1_page(_body(rng, 9), 3, stats=[F(9, t, payload)])
        bad(f"nesting_past_limit_{name}_in_statistics", [p], 0)
    # counts that run past the chunk (all within MAX_GPU_COUNT)
    for name, f in (("binary", F(9, 8, uvarint(1000) + b"abc")),
                    ("binary_2p63", F(9, 8, uvarint(2**63) + b"abc")),
                    ("binary_max", F(9, 8, uvarint(M64) + b"abc")),
                    ("list_i32", F(9, 9, e_list(5, [e_int(1)] * 3, count=60000))),
                    ("list_bool", F(9, 9, e_list(1, [e_bool(1)] * 3, count=65536))),
                    ("list_struct", F(9, 9, e_list(12, [b"\x00"] * 3, count=65536))),
                    ("map_i32_i32", F(9, 11, e_map(5, 5, [(e_int(1), e_int(2))], count=60000))),
                    ("map_bool_bool", F(9, 11, e_map(1, 1, [(e_bool(1), e_bool(0))], count=65536)))):
        p = v1_page(b"", 3)               # no body: nothing after the header for the count to run into
        p.fields.append(f)
        bad(f"count_past_chunk_{name}", [good(), p], 1)
    # too few slots: PF_ERR_CAPACITY at the first page without one (page_cap = n_pages is every valid case)
    out.append(Case("invalid", "page_cap_one_short", _trio(rng), status=CAPACITY, err_page=2, page_cap=2))
    out.append(Case("invalid", "page_cap_zero", [good()], status=CAPACITY, err_page=0, page_cap=0))
    return out


@functools.lru_cache(maxsize=None)
def invalid_cases():
    out = _invalid(np.random.default_rng(21))
    for c in out:
        assert max(container_counts(c.data, c.num_values), default=0) <= MAX_GPU_COUNT, c
    assert len({repr(c) for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def huge_count_cases():
    """Containers of 2^62 (and 2^64 - 1) zero-width or one-byte elements in a 40-byte chunk: PF_ERR_CORRUPT_PAGE
    at once, since every element costs a byte the chunk does not have. CPU only."""
    out = []
    for n in (2**62, M64):
        for name, f in (("map_bool_bool", F(9, 11, e_map(1, 1, [(e_bool(1), e_bool(0))] * 2, count=n))),
                        ("map_bool_false", F(9, 11, e_map(2, 2, [(e_bool(1), e_bool(0))] * 2, count=n))),
                        ("list_bool", F(9, 9, e_list(1, [e_bool(1)] * 4, count=n))),
                        ("list_struct", F(9, 9, e_list(12, [b"\x00"] * 4, count=n))),
                        ("list_empty_list", F(9, 9, e_list(9, [b"\x05"] * 4, count=n)))):
            p = v1_page(b"", 3)
            p.fields.append(f)
            c = Case("huge", f"{name}_{n:#x}", [p], status=CORRUPT, err_page=0, gpu=False)
            c.data = c.data + bytes(40 - len(c.data))
            assert len(c.data) == 40
            out.append(c)
    return tuple(out)


# ---------------------------------------------------------------- this module's own reader (the count bound only)
class _R:
    def __init__(self, b):
        self.b, self.p, self.counts = b, 0, []

    def byte(self):
        v = self.b[self.p]          # IndexError at the end of the chunk
        self.p += 1
        return v

    def uv(self):
        v = 0
        for i in range(10):
            c = self.byte()
            v |= (c & 0x7F) << (7 * i)
            if not c & 0x80:
                return v & M64
        raise ValueError("varint")

    def zz(self):
        u = self.uv()
        return (u >> 1) ^ -(u & 1)

    def field(self, last):
        h = self.byte()
        if h == 0:
            return 0, 0
        d = h >> 4
        fid = last + d if d else ((self.zz() + 0x8000) & 0xFFFF) - 0x8000
        return fid, h & 15

    def integer(self, t):
        if t == 3:
            return self.byte()
        if t in (4, 5, 6):
            return self.zz()
        raise ValueError("integer")

    def skip(self, t, depth=0, inside=False):
        if t in (1, 2):
            if inside:
                self.byte()
        elif t == 3:
            self.byte()
        elif t in (4, 5, 6):
            self.uv()
        elif t == 7:
            self.p += 8
        elif t == 8:
            self.p += self.uv()
        elif t in (9, 10, 11, 12):
            if depth >= MAX_NEST:
                raise ValueError("nesting")
            if t == 12:
                last = 0
                while True:
                    fid, ft = self.field(last)
                    if fid == 0 and ft == 0:
                        return
                    last = fid
                    self.skip(ft, depth + 1)
            elif t == 11:
                n = self.uv()
                self.counts.append(n)
                if n:
                    kv = self.byte()
                    for _ in range(n):
                        self.skip(kv >> 4, depth + 1, True)
                        self.skip(kv & 15, depth + 1, True)
            else:
                h = self.byte()
                n = h >> 4
                if n == 15:
                    n = self.uv()
                self.counts.append(n)
                for _ in range(n):
                    self.skip(h & 15, depth + 1, True)
        else:
            raise ValueError("type")
        if self.p > len(self.b):
            raise IndexError


def container_counts(data, num_values):
    """Every list / set / map count a page walk of the chunk meets, up to where it ends or fails."""
    r = _R(data)
    seen, off = 0, 0
    try:
        while seen < num_values:
            r.p = off
            ptype, csize, nv, last = -1, 0, 0, 0
            while True:
                fid, t = r.field(last)
                if fid == 0 and t == 0:
                    break
                last = fid
                if fid == 1:
                    ptype = r.integer(t)
                elif fid == 3:
                    csize = r.integer(t)
                elif fid in (5, 7, 8) and t == 12:
                    l2 = 0
                    while True:
                        f2, t2 = r.field(l2)
                        if f2 == 0 and t2 == 0:
                            break
                        l2 = f2
                        if f2 == 1:
                            nv = r.integer(t2)
                        else:
                            r.skip(t2)
                else:
                    r.skip(t)
            if csize < 0 or r.p + csize > len(data):
                break
            off = r.p + csize
            if ptype in (DATA, DATA_V2):
                if nv < 0:
                    break
                seen += nv
            if off >= len(data):
                break
    except (IndexError, ValueError):
        pass
    return r.counts


# ---------------------------------------------------------------- mutants
MUTATIONS = (("set00", lambda b: 0x00), ("setff", lambda b: 0xFF), ("x80", lambda b: b ^ 0x80), ("x01", lambda b: b ^ 0x01),
             ("set19", lambda b: 0x19), ("set1b", lambda b: 0x1B), ("set1c", lambda b: 0x1C))


def _opaque(data, lo, hi):
    """Positions inside a long run of FILL bytes (the payload of a long binary), four bytes from either end
    excepted: no parser interprets them, so damaging them changes nothing."""
    skip = set()
    i = lo
    while i < hi:
        j = i
        while j < hi and data[j] == FILL:
            j += 1
        if j - i >= 24:
            skip.update(range(i + 4, j - 4))
        i = max(j, i + 1)
    return skip


def mutants(case):
    """One-byte damages of every header byte of a valid case: [(name, bytes)] for the GPU, and the ones whose
    damage made a container count above MAX_GPU_COUNT, which stay on the CPU. No expectation by construction:
    they are checked differentially (host walk against GPU scan)."""
    gpu, cpu_only = [], []
    assert len(case.data) <= MUTANT_MAX_CHUNK, case
    for lo, hi in case.headers:
        skip = _opaque(case.data, lo, hi)
        for pos in range(lo, hi):
            if pos in skip:
                continue
            for name, fn in MUTATIONS:
                v = fn(case.data[pos])
                if v == case.data[pos]:
                    continue
                m = bytearray(case.data)
                m[pos] = v
                m = bytes(m)
                item = (f"{case.name}@{pos}:{name}", m)
                if max(container_counts(m, case.num_values), default=0) > MAX_GPU_COUNT:
                    cpu_only.append(item)
                else:
                    gpu.append(item)
    return gpu, cpu_only


def mutant_bases():
    """The valid cases whose headers are damaged: all of them, except that a sweep is one chunk at many lengths
    and gives its first, middle and last position, that the crc_bad chunks repeat a crc chunk, and that chunks
    above MUTANT_MAX_CHUNK (a copy per damaged byte) stay out."""
    out = []
    sweep = {}
    for c in valid_cases():
        if c.group in ("stats_sweep", "window"):
            sweep.setdefault(c.group, []).append(c)
        elif c.group != "crc_bad" and len(c.data) <= MUTANT_MAX_CHUNK:
            out.append(c)
    for g in sweep.values():
        out += [g[0], g[len(g) // 2], g[-1]]
    return out
