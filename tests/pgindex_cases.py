"""The page index of the write path (PF_ENCODE_PAGE_INDEX): the reference the tests compare with, and the cases.

ref_index states parquet-format's rules for ColumnIndex value by value, in Python, from the pages' present values alone;
test_write_pgindex_cpu.py pins it to what pyarrow writes. No product code here. Thrift is read with stats_cases.read_struct.

Pages are given whole: a case is a list of pages, a page a list of Python values with None for a null row. Every page
but the last has page_rows rows, a multiple of 8 between 8 and 48 (the encoder starts a page on a validity byte)."""
import struct

import numpy as np

import pagekit as K
import stats_cases as S

UNORDERED, ASCENDING, DESCENDING = 0, 1, 2
LIMIT = S.LIMIT          # without truncation an entry with len(min) + len(max) at or above it drops the ColumnIndex
DEFAULT_T = 64           # index_truncate = 0
_FMT = {K.INT32: "<i", K.INT64: "<q", K.FLOAT: "<f", K.DOUBLE: "<d"}


# ---------------------------------------------------------------- the reference
def _plain(ptype, v):
    if ptype == K.BYTE_ARRAY:
        return v
    if ptype == K.BOOLEAN:
        return b"\x01" if v else b"\x00"
    return struct.pack(_FMT[ptype], v)


def _decode(ptype, b):
    """A written entry back to a value that Python compares in the type's order."""
    if ptype == K.BYTE_ARRAY:
        return b                       # bytes compare unsigned, a proper prefix first
    if ptype == K.BOOLEAN:
        return b[0]
    return struct.unpack(_FMT[ptype], b)[0]   # floats by value: -0.0 == +0.0


def truncate_max(v, T):
    """The shortest upper bound of v among the strings of at most T bytes: its first T bytes less trailing 0xFF bytes,
    the last byte left incremented; None when nothing is left."""
    if T < 0 or len(v) <= T:
        return v
    cut = v[:T].rstrip(b"\xff")
    return cut[:-1] + bytes([cut[-1] + 1]) if cut else None


def ref_index(ptype, pages, T):
    """pages: [(present values, null rows)]; T: the longest BYTE_ARRAY entry, -1 for no truncation.
    -> {"valid": a ColumnIndex is written, "null_pages", "null_counts", and when valid "min_values", "max_values"
    (PLAIN bytes, b"" for a null page) and "boundary_order"}."""
    out = {"valid": True, "null_pages": [], "null_counts": [], "min_values": [], "max_values": []}
    for values, nulls in pages:
        out["null_pages"].append(len(values) == 0)
        out["null_counts"].append(nulls)
        lo = hi = None
        for v in values:
            if ptype in (K.FLOAT, K.DOUBLE) and v != v:
                continue
            lo = v if lo is None or v < lo else lo
            hi = v if hi is None or v > hi else hi
        if len(values) == 0:
            out["min_values"].append(b"")
            out["max_values"].append(b"")
            continue
        if lo is None:                                 # NaN alone: no min / max to write, no ColumnIndex
            out["valid"] = False
            continue
        if ptype in (K.FLOAT, K.DOUBLE):
            lo = -0.0 if lo == 0 else lo               # a zero min is written -0.0, a zero max +0.0
            hi = 0.0 if hi == 0 else hi
        lo, hi = _plain(ptype, lo), _plain(ptype, hi)
        if ptype == K.BYTE_ARRAY:
            if T < 0 and len(lo) + len(hi) >= LIMIT:
                out["valid"] = False
                continue
            lo = lo if T < 0 else lo[:T]
            hi = truncate_max(hi, T)
            if hi is None:
                out["valid"] = False
                continue
        out["min_values"].append(lo)
        out["max_values"].append(hi)
    if not out["valid"]:
        return {k: out[k] for k in ("valid", "null_pages", "null_counts")}
    live = [i for i, n in enumerate(out["null_pages"]) if not n]
    mins = [_decode(ptype, out["min_values"][i]) for i in live]
    maxs = [_decode(ptype, out["max_values"][i]) for i in live]
    pairs = range(len(live) - 1)
    asc = all(mins[i] <= mins[i + 1] and maxs[i] <= maxs[i + 1] for i in pairs)
    desc = all(mins[i] >= mins[i + 1] and maxs[i] >= maxs[i + 1] for i in pairs)
    out["boundary_order"] = UNORDERED if not live else ASCENDING if asc else DESCENDING if desc else UNORDERED
    return out


# ---------------------------------------------------------------- cases
class IndexCase(S.Case):
    """A stats_cases.Case built from whole pages, with its truncation length T (index_truncate; 0: the default 64)."""

    def __init__(self, name, ptype, pages, page_rows=8, T=0, optional=None):
        rows = [v for pg in pages for v in pg]
        assert page_rows % 8 == 0 and all(len(pg) == page_rows for pg in pages[:-1]) and 0 < len(pages[-1]) <= page_rows, name
        has_null = any(v is None for v in rows)
        optional = has_null if optional is None else optional
        assert optional or not has_null, name
        dense = [v for v in rows if v is not None]
        super().__init__(name, ptype, dense, present=[v is not None for v in rows] if optional else None, page_rows=page_rows)
        self.T = T
        self.pages = pages

    @property
    def trunc(self):
        return DEFAULT_T if self.T == 0 else self.T

    def ref_pages(self):
        out = []
        for pg in self.pages:
            vals = [v for v in pg if v is not None]
            if self.ptype == K.FLOAT:      # what the column holds: float32
                vals = [float(np.float32(v)) for v in vals]
            out.append((vals, len(pg) - len(vals)))
        return out

    def ref(self, T=None):
        return ref_index(self.ptype, self.ref_pages(), self.trunc if T is None else T)

    def first_rows(self):
        return [i * self.page_rows for i in range(len(self.pages))]

    def pyarrow_expressible(self):
        """pyarrow truncates nothing and drops statistics of long values by a limit of its own."""
        return self.ptype != K.BYTE_ARRAY or all(len(v) <= 1000 for v in self.dense)


TYPES = (("i32", K.INT32), ("i64", K.INT64), ("f32", K.FLOAT), ("f64", K.DOUBLE), ("b", K.BOOLEAN), ("s", K.BYTE_ARRAY))


def val(ptype, k):
    """A value of the type that grows with k (BOOLEAN: k > 0)."""
    if ptype == K.INT32:
        return 7 * k - 1000
    if ptype == K.INT64:
        return k * 10 ** 10 - 5 * 10 ** 11
    if ptype == K.FLOAT:
        return 0.5 * k - 20.0
    if ptype == K.DOUBLE:
        return 0.25 * k - 1e3 + 1e-9
    if ptype == K.BOOLEAN:
        return k > 0
    return b"key%05d" % k


def span(ptype, lo, hi, rows=8, nulls=()):
    """A page whose present values lie in [val(lo), val(hi)], both reached; rows listed in `nulls` are null."""
    live = [r for r in range(rows) if r not in nulls]
    ks = [hi if j == len(live) // 2 else lo if j == len(live) - 1 else (lo + hi + j) // 2 if hi - lo > 1 else lo
          for j in range(len(live))]
    if len(live) == 1:
        assert lo == hi
    it = iter(ks)
    return [None if r in nulls else val(ptype, next(it)) for r in range(rows)]


NULL_PAGE = [None] * 8

# (lo, hi) of every page; None: a null page. BOOLEAN has its own, over {0, 1}.
_ORDERS = {
    "ascending": ([(0, 5), (10, 15), (20, 25), (30, 35), (40, 45)], [(0, 0), (0, 1), (1, 1)]),
    "descending": ([(40, 45), (30, 35), (20, 25), (10, 15), (0, 5)], [(1, 1), (0, 1), (0, 0)]),
    "equal": ([(3, 9)] * 4, [(0, 1)] * 3),
    "max_out_of_order": ([(0, 50), (10, 60), (20, 55), (30, 70)], [(0, 1), (0, 0), (0, 1)]),
    "broken_across_null": ([(0, 5), (10, 15), None, (7, 9), (20, 30)], [(0, 0), (1, 1), None, (0, 0)]),
    "ascending_across_null": ([(0, 5), None, (10, 15), None, None, (15, 15)], [(0, 0), None, (0, 1), None, (1, 1)]),
    "descending_ties": ([(9, 9), (9, 9), (4, 9), (4, 4)], [(1, 1), (1, 1), (0, 1), (0, 0)]),
}
_ORDER_WANT = {"ascending": ASCENDING, "descending": DESCENDING, "equal": ASCENDING, "max_out_of_order": UNORDERED,
               "broken_across_null": UNORDERED, "ascending_across_null": ASCENDING, "descending_ties": DESCENDING}


def _order_cases():
    out = []
    for tname, ptype in TYPES:
        for oname, (spec, bspec) in _ORDERS.items():
            pages = [NULL_PAGE if s is None else span(ptype, s[0], s[1], nulls=(k % 3,) if k % 2 else ())
                     for k, s in enumerate(bspec if ptype == K.BOOLEAN else spec)]
            c = IndexCase(f"{tname}_{oname}", ptype, pages, optional=True)
            c.want_order = _ORDER_WANT[oname]
            out.append(c)
    return out


def _count_cases():
    """1, 64, 65, 256 and 257 pages of 8 rows: the stride and wave edges of a 256-thread workgroup; ascending runs
    broken at one pair only, which a pair loop that stops early or skips a wave edge reports as ASCENDING."""
    out = []
    for n in (1, 64, 65, 256, 257):
        out.append(IndexCase(f"i32_pages_{n}_ascending", K.INT32, [span(K.INT32, 3 * p, 3 * p + 2) for p in range(n)]))
        rng = S._rng("pgindex", n)
        pages = [[None if rng.random() < 0.2 else int(rng.integers(-50, 50)) for _ in range(8)] for _ in range(n)]
        out.append(IndexCase(f"i32_pages_{n}_random", K.INT32, pages, optional=True))
        words = [[None if rng.random() < 0.2 else bytes(rng.integers(97, 123, int(rng.integers(0, 90)), dtype=np.uint8)) for _ in range(8)]
                 for _ in range(n)]
        out.append(IndexCase(f"s_pages_{n}_random", K.BYTE_ARRAY, words, optional=True))
    for n, at in ((65, 63), (257, 63), (257, 127), (257, 255), (257, 0)):   # pair (at, at + 1) alone goes down
        ks = [3 * p if p <= at else 3 * p - 4 for p in range(n)]
        out.append(IndexCase(f"i64_pages_{n}_break_{at}", K.INT64, [span(K.INT64, k, k + 2) for k in ks]))
        ks = [3 * (n - p) if p <= at else 3 * (n - p) + 4 for p in range(n)]
        out.append(IndexCase(f"f64_pages_{n}_desc_break_{at}", K.DOUBLE, [span(K.DOUBLE, k, k + 2) for k in ks]))
    # every other page null: the compaction crosses every wave
    out.append(IndexCase("i32_pages_257_alternate_null", K.INT32,
                         [NULL_PAGE if p % 2 else span(K.INT32, p, p + 1) for p in range(257)]))
    out.append(IndexCase("page_rows_48_last_short", K.INT64, [span(K.INT64, 5 * p, 5 * p + 4, rows=48, nulls=(1, 47)) for p in range(6)] +
                         [span(K.INT64, 100, 101, rows=5)], page_rows=48))
    out.append(IndexCase("page_rows_16", K.DOUBLE, [span(K.DOUBLE, 9 - p, 9 - p, rows=16) for p in range(9)], page_rows=16))
    return out


def _null_cases():
    out = []
    for tname, ptype in (("i32", K.INT32), ("f64", K.DOUBLE), ("s", K.BYTE_ARRAY), ("b", K.BOOLEAN)):
        live = [span(ptype, 0, 1), span(ptype, 1, 1), span(ptype, 1, 1, nulls=(0, 7))]
        out.append(IndexCase(f"{tname}_null_page_first", ptype, [NULL_PAGE] + live))
        out.append(IndexCase(f"{tname}_null_page_last", ptype, live + [NULL_PAGE]))
        out.append(IndexCase(f"{tname}_null_page_middle", ptype, live[:1] + [NULL_PAGE] + live[1:]))
        out.append(IndexCase(f"{tname}_all_null", ptype, [NULL_PAGE] * 3 + [[None] * 3]))
        out.append(IndexCase(f"{tname}_optional_no_nulls", ptype, live[:2], optional=True))
        out.append(IndexCase(f"{tname}_single_value", ptype, [[val(ptype, 1)]]))
    return out


def _float_cases():
    out, nan, inf = [], float("nan"), float("inf")
    for tname, ptype in (("f32", K.FLOAT), ("f64", K.DOUBLE)):
        a, b = span(ptype, 0, 5), span(ptype, 10, 15)
        out.append(IndexCase(f"{tname}_nan_only_page", ptype, [a, [nan] * 8, b]))
        out.append(IndexCase(f"{tname}_nan_only_with_nulls", ptype, [a, [nan, None] * 4, b]))
        out.append(IndexCase(f"{tname}_nan_mixed", ptype, [[nan] + a[1:], b[:4] + [nan, -nan] + b[6:], [nan] * 7 + [99.0]]))
        out.append(IndexCase(f"{tname}_zeros", ptype, [[0.0] * 8, [-0.0] * 8, [0.0, -0.0] * 4, [-0.0, 1.0] * 4, [-1.0, 0.0] * 4]))
        out.append(IndexCase(f"{tname}_zeros_tie", ptype, [[0.0] * 8, [-0.0] * 8, [0.0] * 8]))   # -0.0 == +0.0: ASCENDING
        out.append(IndexCase(f"{tname}_inf", ptype, [[-inf] * 8, [-inf, 0.0] * 4, [1.0, inf] * 4, [inf] * 8]))
        out.append(IndexCase(f"{tname}_inf_descending", ptype, [[inf, 3.0] * 4, [2.0, -inf] * 4, [-inf, None] * 4]))
    return out


def _string_cases():
    out, T = [], 8
    base = b"abcdefghijklmnop"

    def pg(*vals):
        return [vals[i % len(vals)] for i in range(8)]

    out.append(IndexCase("s_len_T_minus_plus", K.BYTE_ARRAY, [pg(base[:T - 1]), pg(base[:T]), pg(base[:T + 1]), pg(base[:T - 1], base[:T + 1])], T=T))
    out.append(IndexCase("s_carry", K.BYTE_ARRAY, [pg(b"abcdefg\xffzz"), pg(b"abcde\xff\xff\xffzz", b"abc"), pg(b"b\xff\xff\xff\xff\xff\xff\xffq")], T=T))
    out.append(IndexCase("s_all_ff", K.BYTE_ARRAY, [pg(b"abc"), pg(b"\xff" * T + b"a", b"b")], T=T))
    out.append(IndexCase("s_all_ff_exactly_T", K.BYTE_ARRAY, [pg(b"abc"), pg(b"\xff" * T, b"b")], T=T))   # fits: written whole
    out.append(IndexCase("s_equal_after_truncation", K.BYTE_ARRAY, [pg(b"a", b"prefix__zzz"), pg(b"a", b"prefix__aaa"), pg(b"a", b"prefix__mmmm")], T=T))
    out.append(IndexCase("s_min_equal_after_truncation", K.BYTE_ARRAY, [pg(b"prefix__zzz", b"q"), pg(b"prefix__aaa", b"q")], T=T))
    out.append(IndexCase("s_empty", K.BYTE_ARRAY, [pg(b""), pg(b"", b"a"), pg(b"a", None), pg(b"", None)]))
    out.append(IndexCase("s_default_T", K.BYTE_ARRAY, [pg(b"x" * 63, b"y" * 64), pg(b"x" * 65, b"y" * 66), pg(b"y" * 63 + b"\xff" * 9)]))
    big = b"m" * 5000
    out.append(IndexCase("s_5000_T64", K.BYTE_ARRAY, [pg(b"a", b"b"), pg(b"c", big), pg(big + b"!", b"z")], T=64))
    out.append(IndexCase("s_5000_no_truncation", K.BYTE_ARRAY, [pg(b"a", b"b"), pg(b"c", big), pg(big + b"!", b"z")], T=-1))
    out.append(IndexCase("s_2047_2048_no_truncation", K.BYTE_ARRAY, [pg(b"a" * 2047, b"b" * 2048)], T=-1))    # 4095: kept
    out.append(IndexCase("s_2048_2048_no_truncation", K.BYTE_ARRAY, [pg(b"a" * 2048, b"b" * 2048)], T=-1))    # 4096: dropped
    out.append(IndexCase("s_no_truncation", K.BYTE_ARRAY, [pg(b"x" * 100, b"y" * 300), pg(b"y" * 300 + b"\xff", b"z")], T=-1))
    out.append(IndexCase("s_T1", K.BYTE_ARRAY, [pg(b"", b"a"), pg(b"ab", b"b"), pg(b"b\x00", b"cz"), pg(b"\xfe\xff")], T=1))
    out.append(IndexCase("s_T1_ff", K.BYTE_ARRAY, [pg(b"a"), pg(b"\xff\x00")], T=1))
    out.append(IndexCase("s_T2047", K.BYTE_ARRAY, [pg(b"k" * 2046, b"k" * 2047), pg(b"k" * 2048, b"l" * 3000), pg(b"l" * 2046 + b"\xff" * 9)], T=2047))
    out.append(IndexCase("s_high_bytes", K.BYTE_ARRAY, [pg(b"\x7f" * 9, b"\x80" * 9), pg(b"\x80" * 9, b"\xc3\xa9" * 5), pg(b"\xfe" * 9, b"\xff\xfe" * 5)], T=T))
    return out


_BUILDERS = (_order_cases, _count_cases, _null_cases, _float_cases, _string_cases)
_CACHE = {}


def cases():
    """{name: IndexCase}, built once and shared (callers must not modify the arrays)."""
    if not _CACHE:
        for b in _BUILDERS:
            for c in b():
                assert c.name not in _CACHE, c.name
                _CACHE[c.name] = c
    return _CACHE


def names():
    return list(cases())


# the cases run under every codec and with every other option switched on: one per type, nulls and null pages among them
OPTION_CASES = ("i32_pages_65_random", "s_pages_65_random", "f64_null_page_middle", "b_broken_across_null", "i64_ascending",
                "f32_zeros", "s_5000_T64", "s_carry")


def column_index_fields(ci):
    """A ColumnIndex struct as stats_cases.read_struct returns it -> the reference's shape."""
    return {"valid": True, "null_pages": ci[1], "min_values": ci[2], "max_values": ci[3], "boundary_order": ci[4],
            "null_counts": ci.get(5)}
