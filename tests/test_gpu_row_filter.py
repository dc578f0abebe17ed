"""Row filters on the GPU: pf_decode_row_group_filter evaluates a conjunction of predicates over the decoded (and
windowed) columns and compacts every chunk of the batch to the matching rows before anything crosses the link (k_sel_*,
csrc/pf_filter.hip). The expected arrays never come from the code under test: pagekit's expected arrays, the oracle's
decode or the arrays a file was written from, cut by window_cases.slice_chunk, masked by filter_cases.eval_predicates
and compacted by filter_cases.take_rows (plain numpy); every comparison is bit-exact, padding bits included."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import filter_cases as FC
import pagekit as K
import window_cases as WC
from conftest import GOLDEN
from pfloor._native import ChunkDesc, ColumnInfo, Predicate, RowWindow, SelectionInfo, lib
from pfloor.decoder import GpuDecoder, ParquetFile, PinnedBuffer

pytestmark = pytest.mark.gpu

RANGE, IS_NULL, NOT_NULL = FC.RANGE, FC.IS_NULL, FC.NOT_NULL
INVALID_ARG, CORRUPT_PAGE, UNSUPPORTED_TYPE, STATE = -1, -2, -7, -9
SEL_TILE = FC.SEL_TILE
I32, I64 = np.iinfo(np.int32), np.iinfo(np.int64)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dec():
    d = GpuDecoder(0)
    yield d
    d.close()


def _plain(v, ptype):
    """PLAIN bytes of a bound, by numpy (not by pfloor.predicate)."""
    if v is None:
        return None
    if ptype == K.BYTE_ARRAY:
        return bytes(v)
    return np.array([v], {K.BOOLEAN: np.uint8, K.INT32: np.int32, K.INT64: np.int64, K.FLOAT: np.float32,
                          K.DOUBLE: np.float64}[ptype]).tobytes()


@contextlib.contextmanager
def _stage(dec, path, rg, cols):
    """Every page of the chunks into the staging buffer: (file, descs, buffer, total, types). The descriptors' page
    arrays belong to the file, so it stays open over the block."""
    with ParquetFile(path) as f:
        items, total = f.plan([rg], cols)
        buf = dec.staging(total)
        descs = []
        for _rg, col, s, n, off in items:
            if n:
                f.read_into(s, n, buf.ptr.value + off)
            descs.append(f.chunk_desc(rg, col, off))
        types = [(f.columns[c].physical_type, f.columns[c].max_def, f.columns[c].max_rep) for c in cols]
        yield f, descs, buf, max(total, 1), types


@pytest.fixture
def stage(dec):
    """stage(path, rg, cols) = _stage, its files kept open until the test ends."""
    with contextlib.ExitStack() as st:
        yield lambda path, rg, cols: st.enter_context(_stage(dec, path, rg, cols))


def filtered(dec, path, cols, preds, windows=None):
    """Whole-chunk path. preds: [(position in cols, op, lo, hi)] with Python values. Returns (rc, chunks, rows_in, rows)."""
    with _stage(dec, path, 0, cols) as (_f, descs, buf, total, types):
        native = [(c, op, _plain(lo, types[c][0]), _plain(hi, types[c][0])) for c, op, lo, hi in preds]
        dec.decode(descs, buf.ptr.value, total, windows=windows, predicates=native)
        rc = dec.wait()
        got = [dec.fetch(i, *t) for i, t in enumerate(types)]
        rows_in, rows = dec.selection()
        return rc, got, rows_in, rows


def check_filtered(dec, path, exp, types, preds, windows=None, label=""):
    """One filtered decode of all chunks of `exp` against the reference; returns rows_selected."""
    n = len(exp)
    rc, got, rows_in, rows = filtered(dec, path, list(range(n)), preds, windows)
    assert rc == 0, (label, preds, dec.error())
    cut = [WC.slice_chunk(e, *(windows[c] if windows else (0, -1))) for c, e in enumerate(exp)]
    mask = FC.eval_predicates(list(zip(cut, types)), preds)
    idx = np.flatnonzero(mask)
    assert rows_in == len(mask), (label, preds)
    assert rows.dtype == np.int32 and np.array_equal(rows, idx), (label, preds, rows[:8], idx[:8])
    for c in range(n):
        assert got[c]["status"] == 0
        WC.assert_window_equal(got[c], FC.take_rows(cut[c], idx), f"{label} {preds} chunk {c}")
    return len(idx)


# ---- hand-assembled flat chunks --------------------------------------------------------------------------------------

ROWS, PAGE = 1000, 96
NULL_PAGE = 3   # data page 3 (rows 288 .. 383) of every OPTIONAL chunk is all null
FIRST, MIDDLE, LAST = 0, 500, 999
SPECIAL = {10: NAN, 11: 0.0, 12: -0.0, 13: INF, 14: -INF}   # rows of the FLOAT / DOUBLE chunks
LONG37, LONG300, LONG5000 = b"m" * 37, b"q" * 299 + b"!", bytes(range(256)) * 19 + b"z" * 136
POOL = [b"", b"a", b"a\x00", b"\xff\xff", b"ab", b"abc", b"row", b"filter", b"w" * 32, b"w" * 33, LONG37, LONG300, LONG5000]
RARE = range(20, ROWS, 97)   # rows of the BYTE_ARRAY chunks that hold b"rare": about 1 %
TYPES = (K.INT32, K.INT64, K.FLOAT, K.DOUBLE, K.BOOLEAN, K.BYTE_ARRAY)


def _full_values(ptype, rows, rng):
    if ptype == K.BYTE_ARRAY:
        v = [POOL[int(i)] for i in rng.integers(0, len(POOL), rows)]
        for r in RARE:
            v[r] = b"rare"
        v[FIRST], v[MIDDLE], v[LAST] = b"0first", b"middle!", b"zlast"
        return v
    if ptype == K.BOOLEAN:
        return rng.integers(0, 2, rows).astype(np.uint8)
    if ptype in (K.INT32, K.INT64):
        dt, lim = (np.int32, I32) if ptype == K.INT32 else (np.int64, I64)
        v = rng.integers(-500, 500, rows).astype(dt)
        v[FIRST], v[MIDDLE], v[LAST] = lim.min, 7777, lim.max
        return v
    v = (rng.normal(0, 100, rows)).astype(np.float32 if ptype == K.FLOAT else np.float64)
    for r, x in SPECIAL.items():
        v[r] = x
    v[FIRST], v[MIDDLE], v[LAST] = -1e30, 12345.5, 1e30
    return v


def _flat_chunks(oracle, rows=ROWS, page=PAGE, types=TYPES, layouts="ace", index_column=True):
    rng = np.random.default_rng(2024)
    chunks = []
    for ptype in types:
        for optional in (False, True):
            layout = K.LAYOUTS[layouts[(ptype + optional) % len(layouts)]]   # v1 uncompressed, v2 Snappy, v2 uncompressed in turn
            ch = K.Chunk(f"t{ptype}{'o' if optional else 'r'}", ptype, optional=optional, layout=layout, compress=oracle.snappy_compress)
            full = _full_values(ptype, rows, rng)
            for pg, a in enumerate(range(0, rows, page)):
                n = min(page, rows - a)
                present = None
                if optional:
                    present = rng.random(n) >= 0.3
                    if pg == NULL_PAGE:
                        present[:] = False
                    else:
                        for r in (FIRST, MIDDLE, LAST, *SPECIAL):
                            if a <= r < a + n:
                                present[r - a] = True
                part = full[a:a + n]
                if ptype == K.BYTE_ARRAY:
                    vals = [x for x, ok in zip(part, present if optional else [True] * n) if ok]
                else:
                    vals = (part[present] if optional else part).view(np.uint8).reshape(-1, K.width_of(ptype))
                ch.add_page(K.PLAIN, K.plain(ptype, vals), present=present, vals=vals)
            chunks.append(ch)
    if index_column:   # the row number, REQUIRED INT32: Range(idx, a, b) selects exactly rows a .. b
        ch = K.Chunk("idx", K.INT32, layout=K.LAYOUTS["e"])
        for a in range(0, rows, page):
            vals = np.arange(a, min(a + page, rows), dtype=np.int32).view(np.uint8).reshape(-1, 4)
            ch.add_page(K.PLAIN, K.plain(K.INT32, vals), vals=vals)
        chunks.append(ch)
    return chunks


def _expected(ch):
    e = ch.expected()
    e["width"] = 0 if ch.ptype == K.BYTE_ARRAY else ch.width
    return e


def _write(chunks, rows, path):
    data, _info = K.build_file(chunks, rows)
    with open(path, "wb") as f:
        f.write(data)
    return path


@pytest.fixture(scope="module")
def flat_file(oracle, tmp_path_factory):
    chunks = _flat_chunks(oracle)
    path = _write(chunks, ROWS, str(tmp_path_factory.mktemp("rowfilter") / "flat.parquet"))
    return path, [_expected(ch) for ch in chunks], [ch.ptype for ch in chunks], chunks


def _col(chunks, ptype, optional):
    return next(i for i, ch in enumerate(chunks) if ch.ptype == ptype and ch.optional == optional and ch.name != "idx")


IDX = 2 * len(TYPES)   # the row-number chunk


def test_one_predicate_per_type_at_every_selectivity(dec, flat_file):
    path, exp, types, chunks = flat_file
    for optional in (False, True):
        for ptype in TYPES:
            c = _col(chunks, ptype, optional)
            v = FC.values_of(exp[c], ptype)
            if ptype == K.BYTE_ARRAY:
                probes = [(b"nothing", b"nothing"), (v[FIRST], v[FIRST]), (v[MIDDLE], v[MIDDLE]), (v[LAST], v[LAST]),
                          (LONG300, LONG300), (b"rare", b"rare"), (b"a", b"row"), (None, None), (b"", b""), (b"", None), (LONG5000[:4000], LONG5000[:3999] + b"\xa0")]
                want_counts = {0: 1, 1: 3}
            elif ptype == K.BOOLEAN:
                probes = [(1, 0), (1, 1), (0, 0), (0, 1), (None, None), (None, 0)]
                want_counts = {0: 1}
            else:
                one = 5 if ptype in (K.INT32, K.INT64) else float(np.sort(v)[len(v) // 2])   # about 1 % / one value
                probes = [(600, 700), (v[FIRST], v[FIRST]), (v[MIDDLE], v[MIDDLE]), (v[LAST], v[LAST]), (one, one + 9 if ptype in (K.INT32, K.INT64) else one + 2.5),
                          (0, None), (None, None), (v[FIRST], v[LAST])]
                probes = [(None if a is None else a.item() if hasattr(a, "item") else a, None if b is None else b.item() if hasattr(b, "item") else b)
                          for a, b in probes]
                want_counts = {0: 1, 1: 3}
            counts = [check_filtered(dec, path, exp, types, [(c, RANGE, lo, hi)], label=f"type {ptype} optional {optional}") for lo, hi in probes]
            present = int(FC.present_of(exp[c]).sum())
            assert counts.count(0) >= want_counts.get(0, 0) and counts.count(1) >= want_counts.get(1, 0), (ptype, optional, counts)
            assert present in counts, (ptype, optional, counts)                       # every present row
            assert any(0.25 * present < k < 0.75 * present for k in counts), counts   # about half
            if ptype not in (K.BOOLEAN,):
                assert any(1 < k <= 0.05 * ROWS for k in counts), counts              # about 1 %


def test_null_predicates(dec, flat_file):
    path, exp, types, chunks = flat_file
    for ptype in TYPES:
        req, opt = _col(chunks, ptype, False), _col(chunks, ptype, True)
        nulls = ROWS - int(FC.present_of(exp[opt]).sum())
        assert check_filtered(dec, path, exp, types, [(opt, IS_NULL, None, None)], label="is null") == nulls >= PAGE
        assert check_filtered(dec, path, exp, types, [(opt, NOT_NULL, None, None)], label="not null") == ROWS - nulls
        assert check_filtered(dec, path, exp, types, [(req, IS_NULL, None, None)], label="required is null") == 0
        assert check_filtered(dec, path, exp, types, [(req, NOT_NULL, None, None)], label="required not null") == ROWS
        # over the null page alone, and around its edges
        a, b = NULL_PAGE * PAGE, (NULL_PAGE + 1) * PAGE
        assert check_filtered(dec, path, exp, types, [(opt, IS_NULL, None, None), (IDX, RANGE, a, b - 1)], label="null page") == PAGE
        assert check_filtered(dec, path, exp, types, [(opt, NOT_NULL, None, None), (IDX, RANGE, a, b - 1)], label="null page") == 0
        check_filtered(dec, path, exp, types, [(opt, IS_NULL, None, None), (IDX, RANGE, a - 5, b + 4)], label="null page edges")
        check_filtered(dec, path, exp, types, [(opt, RANGE, None, None), (IDX, RANGE, a - 5, b + 4)], label="null page edges, range")


def test_float_bounds_at_nan_zero_and_infinity(dec, flat_file):
    path, exp, types, chunks = flat_file
    for ptype in (K.FLOAT, K.DOUBLE):
        for optional in (False, True):
            c = _col(chunks, ptype, optional)
            count = {}
            for lo, hi in ((NAN, NAN), (NAN, None), (None, NAN), (0.0, 0.0), (-0.0, -0.0), (-0.0, 0.0), (INF, INF), (-INF, -INF),
                           (-INF, INF), (INF, None), (None, -INF), (-INF, None), (None, INF), (1e30, INF), (0.0, None), (None, -0.0)):
                count[(str(lo), str(hi))] = check_filtered(dec, path, exp, types, [(c, RANGE, lo, hi)], label=f"float type {ptype}")
            present = int(FC.present_of(exp[c]).sum())
            assert count[("nan", "nan")] == count[("nan", "None")] == count[("None", "nan")] == 0
            assert count[("0.0", "0.0")] == count[("-0.0", "-0.0")] == count[("-0.0", "0.0")] == 2   # +0.0 and -0.0 are equal
            assert count[("inf", "inf")] == count[("-inf", "-inf")] == 1 and count[("1e+30", "inf")] == 2
            assert count[("-inf", "inf")] == present - 1                                                # all but the NaN
            assert check_filtered(dec, path, exp, types, [(c, RANGE, None, None)], label="float, no bounds") == present   # NaN included


def test_integer_bounds_at_the_types_limits(dec, flat_file):
    path, exp, types, chunks = flat_file
    for ptype, lim in ((K.INT32, I32), (K.INT64, I64)):
        for optional in (False, True):
            c = _col(chunks, ptype, optional)
            present = int(FC.present_of(exp[c]).sum())
            got = [check_filtered(dec, path, exp, types, [(c, RANGE, lo, hi)], label=f"int type {ptype}")
                   for lo, hi in ((lim.min, lim.min), (lim.max, lim.max), (lim.min, lim.max), (lim.min + 1, lim.max - 1), (lim.max, lim.min),
                                  (None, lim.min), (lim.max, None), (-1, 0))]
            assert got[:5] == [1, 1, present, present - 2, 0] and got[5:7] == [1, 1] and got[7] > 0


def test_byte_array_bounds_prefixes_and_long_values(dec, flat_file):
    path, exp, types, chunks = flat_file
    for optional in (False, True):
        c = _col(chunks, K.BYTE_ARRAY, optional)
        v = [x for x, ok in zip(FC.values_of(exp[c], K.BYTE_ARRAY), FC.present_of(exp[c])) if ok]
        n = {}
        for lo, hi in ((b"a", b"a"), (b"a", b"a\x00"), (b"a\x00", b"a\x00"), (b"a", b"ab"), (b"ab", b"abc"), (b"a\x00\x00", b"ab"), (b"\xff", None),
                       (b"\xff\xff", b"\xff\xff"), (None, b"\x00"), (b"w" * 32, b"w" * 32), (b"w" * 32, b"w" * 33), (LONG37[:36], LONG37),
                       (LONG5000[:4096], None), (LONG5000[:4095], LONG5000[:4096]), (LONG300[:150], LONG300), (b"", b"")):
            n[(lo, hi)] = check_filtered(dec, path, exp, types, [(c, RANGE, lo, hi)], label="strings")
        assert n[(b"a", b"a")] == v.count(b"a") > 0 and n[(b"a", b"a\x00")] == v.count(b"a") + v.count(b"a\x00")
        assert n[(b"a", b"ab")] == v.count(b"a") + v.count(b"a\x00") + v.count(b"ab")      # a proper prefix sorts first
        assert n[(b"a\x00\x00", b"ab")] == v.count(b"ab") and n[(b"\xff", None)] == v.count(b"\xff\xff") > 0
        assert n[(None, b"\x00")] == n[(b"", b"")] == v.count(b"") > 0
        assert n[(LONG37[:36], LONG37)] == v.count(LONG37) > 0 and n[(LONG300[:150], LONG300)] == v.count(LONG300) > 0
        assert n[(LONG5000[:4096], None)] >= v.count(LONG5000) > 0 and n[(LONG5000[:4095], LONG5000[:4096])] == 0


def test_every_padding_of_the_last_validity_word(dec, flat_file):
    """rows_selected at every value mod 8 and around 64 and 128, from contiguous and from scattered rows."""
    path, exp, types, chunks = flat_file
    for n in list(range(0, 18)) + [63, 64, 65, 127, 128, 129]:
        assert check_filtered(dec, path, exp, types, [(IDX, RANGE, 283, 283 + n - 1)], label="contiguous") == n
    b = _col(chunks, K.BOOLEAN, False)
    seen = set()
    for hi in list(range(40, 56)) + list(range(100, 160)) + list(range(220, 300)):   # (a count grows by 0 or 1 with hi)
        seen.add(check_filtered(dec, path, exp, types, [(IDX, RANGE, 37, hi + 37), (b, RANGE, 1, 1)], label="scattered"))
    assert {k % 8 for k in seen} == set(range(8)) and {63, 64, 65, 127, 128, 129} <= seen, sorted(seen)


def test_conjunctions_over_columns_of_different_types(dec, flat_file):
    path, exp, types, chunks = flat_file
    i32, i64o = _col(chunks, K.INT32, False), _col(chunks, K.INT64, True)
    dbl, flo = _col(chunks, K.DOUBLE, False), _col(chunks, K.FLOAT, True)
    boo, s, so = _col(chunks, K.BOOLEAN, True), _col(chunks, K.BYTE_ARRAY, False), _col(chunks, K.BYTE_ARRAY, True)
    two = [(i32, RANGE, -250, 250), (s, RANGE, b"a", b"row")]
    three = two + [(dbl, RANGE, -50.0, None)]
    eight = [(i32, RANGE, -400, 400), (i64o, NOT_NULL, None, None), (dbl, RANGE, -150.0, 150.0), (flo, RANGE, None, 120.0),
             (boo, RANGE, 0, 1), (s, RANGE, b"", b"x"), (so, IS_NULL, None, None), (IDX, RANGE, 5, 990)]
    counts = [check_filtered(dec, path, exp, types, p, label="conjunction") for p in (two, three, eight, eight[::-1])]
    assert counts[0] > counts[1] > 0 and counts[2] == counts[3] > 0, counts
    assert check_filtered(dec, path, exp, types, [(i32, RANGE, 0, None), (i32, RANGE, None, -1)], label="empty conjunction") == 0


def test_payloads_of_other_widths(dec, tmp_path):
    """INT96 (12 bytes: one lane per output dword) and FIXED_LEN_BYTE_ARRAY of 5 and 3 bytes (one lane per output byte)
    as payloads, enough rows for several rounds of a workgroup."""
    rows = 3 * SEL_TILE + 77
    rng = np.random.default_rng(96)
    chunks = []
    for name, ptype, tl, optional in (("i96", K.INT96, 0, False), ("f5", K.FLBA, 5, True), ("f3", K.FLBA, 3, False)):
        ch = K.Chunk(name, ptype, type_length=tl, optional=optional, layout=K.LAYOUTS["e"])
        w = K.width_of(ptype, tl)
        for a in range(0, rows, 700):
            n = min(700, rows - a)
            present = rng.random(n) >= 0.4 if optional else None
            vals = rng.integers(0, 256, (n if present is None else int(present.sum()), w)).astype(np.uint8)
            ch.add_page(K.PLAIN, K.plain(ptype, vals), present=present, vals=vals)
        chunks.append(ch)
    idx = K.Chunk("idx", K.INT32, layout=K.LAYOUTS["e"])
    vals = np.arange(rows, dtype=np.int32).view(np.uint8).reshape(-1, 4)
    idx.add_page(K.PLAIN, K.plain(K.INT32, vals), vals=vals)
    chunks.append(idx)
    path = _write(chunks, rows, str(tmp_path / "widths.parquet"))
    exp, types = [_expected(ch) for ch in chunks], [ch.ptype for ch in chunks]
    assert check_filtered(dec, path, exp, types, [(3, RANGE, 5, rows - 9)], label="widths") == rows - 13
    assert check_filtered(dec, path, exp, types, [(3, RANGE, 1000, 1002), (1, NOT_NULL, None, None)], label="widths") <= 3
    check_filtered(dec, path, exp, types, [(1, IS_NULL, None, None), (0, NOT_NULL, None, None)], label="widths, null FLBA")


# ---- tiles -----------------------------------------------------------------------------------------------------------

def _tile_file(rows, tmp_path):
    rng = np.random.default_rng(rows)
    words = [b"", b"k", b"tile", b"gfx950", b"w" * 33]
    num = K.Chunk("n", K.INT32, layout=K.LAYOUTS["e"])
    txt = K.Chunk("s", K.BYTE_ARRAY, layout=K.LAYOUTS["e"])
    page = 50000
    for a in range(0, rows, page):
        n = min(page, rows - a)
        v = rng.integers(-1000, 1000, n).astype(np.int32).view(np.uint8).reshape(-1, 4)
        num.add_page(K.PLAIN, K.plain(K.INT32, v), vals=v)
        w = [words[int(i)] for i in rng.integers(0, len(words), n)]
        txt.add_page(K.PLAIN, K.plain(K.BYTE_ARRAY, w), vals=w)
    return _write([num, txt], rows, str(tmp_path / f"tile{rows}.parquet")), [_expected(num), _expected(txt)], [K.INT32, K.BYTE_ARRAY]


@pytest.mark.parametrize("rows", [SEL_TILE - 1, SEL_TILE, SEL_TILE + 1, 2 * SEL_TILE + 1, 256 * SEL_TILE + 1])
def test_tile_edges_and_the_scan_round(dec, tmp_path, rows):
    """Rows at the tile's edges, and 256 tiles + 1: the tile-count scan takes a second round with a carry. Selecting
    every row makes the output tiles cross the same edges."""
    path, exp, types = _tile_file(rows, tmp_path)
    assert check_filtered(dec, path, exp, types, [(0, RANGE, None, None)], label="all rows") == rows
    k = check_filtered(dec, path, exp, types, [(0, RANGE, 0, None)], label="half")
    assert 0.4 * rows < k < 0.6 * rows
    if rows > 4 * SEL_TILE:
        return
    v = FC.values_of(exp[0], K.INT32)
    last = int(v[-1])
    got = check_filtered(dec, path, exp, types, [(0, RANGE, last, last), (1, RANGE, b"", b"zz")], label="few")
    assert got == int((v == last).sum())
    assert check_filtered(dec, path, exp, types, [(1, RANGE, b"w" * 33, None)], label="long strings") > 0


# ---- with windows ----------------------------------------------------------------------------------------------------

def test_windows_then_filter_whole_chunk_path(dec, flat_file):
    path, exp, types, chunks = flat_file
    n = len(exp)
    i32, so = _col(chunks, K.INT32, False), _col(chunks, K.BYTE_ARRAY, True)
    for skip, take in ((3, 77), (101, 333), (285, 100), (0, 999), (1, -1), (997, 3), (500, 0), (0, ROWS)):
        wins = [(skip, take)] * n
        check_filtered(dec, path, exp, types, [(i32, RANGE, -100, None)], wins, label=f"window ({skip}, {take})")
        check_filtered(dec, path, exp, types, [(so, NOT_NULL, None, None), (IDX, RANGE, skip + 2, None)], wins, label=f"window ({skip}, {take})")
    # row numbers count from the window's first row
    rc, got, rows_in, rows = filtered(dec, path, list(range(n)), [(IDX, RANGE, 110, 112)], [(101, 333)] * n)
    assert rc == 0 and rows_in == 333 and list(rows) == [9, 10, 11]
    assert list(np.frombuffer(got[IDX]["values"].tobytes(), np.int32)) == [110, 111, 112]
    # chunks without a window ({0, -1}) beside chunks whose window turns out to keep every row, and beside moved ones
    wins = [(0, -1) if c % 2 else (0, ROWS) for c in range(n)]
    check_filtered(dec, path, exp, types, [(i32, RANGE, None, 100), (so, RANGE, b"a", None)], wins, label="identity windows")
    # windows that differ per chunk but keep equal row counts
    wins = [(c % 7, 990) for c in range(n)]
    check_filtered(dec, path, exp, types, [(i32, RANGE, None, 0), (so, RANGE, b"a", None)], wins, label="shifted windows")


@pytest.mark.parametrize("name", WC.FIXTURES)
def test_windows_then_filter_indexed_path(dec, oracle, name):
    """plan_rows over the fixtures of the row-window tests (pyarrow's irregular pages). A range that starts and ends on
    page edges of one column and not of the other leaves one chunk in the decode arenas (its window keeps every row of
    its pages) while the other was moved to the twins: both copy directions of the filter in one batch."""
    path = WC.fixture_path(name)
    cols = [0, 1]   # key INT64, s optional string
    with oracle.open(path) as of:
        exp = [of.decode(0, c) for c in cols]
    types = [K.INT64, K.BYTE_ARRAY]
    keys = FC.values_of(exp[0], K.INT64)
    with ParquetFile(path) as f:
        edges = [[r for _o, _s, r in f.page_index(0, c)["offset_index"]] for c in cols]
        rows = f.row_group_rows(0)
        own = [e for e in edges[1][1:] if e not in edges[0]] or [e for e in edges[0][1:] if e not in edges[1]]
        which = 1 if [e for e in edges[1][1:] if e not in edges[0]] else 0
        ranges = [(own[0], own[1]), (edges[which][1], edges[which][3]), (own[0] + 3, own[1] - 5), (0, rows), (7, 8), (rows - 1, rows), (40, 40)]
        mixed = 0
        for lo, hi in ranges:
            items, total, windows = f.plan_rows(0, cols, lo, hi)
            buf = dec.staging(total)
            f.read_rows(items, buf.ptr.value)
            in_place = [r.skip_rows == 0 and r.take_rows == d.num_rows for _c, d, r, _o in items]
            mixed += in_place[0] != in_place[1]
            cut = [WC.slice_chunk(e, lo, hi - lo) for e in exp]
            mid = int(np.sort(keys[lo:hi])[(hi - lo) // 2]) if hi > lo else 0
            for preds in ([(0, RANGE, mid, None)], [(1, NOT_NULL, None, None), (0, RANGE, None, mid)], [(1, IS_NULL, None, None)]):
                native = [(c, op, _plain(a, types[c]), _plain(b, types[c])) for c, op, a, b in preds]
                dec.decode([d for _c, d, _r, _o in items], buf.ptr.value, max(total, 1), windows=windows, predicates=native)
                assert dec.wait() == 0, dec.error()
                idx = np.flatnonzero(FC.eval_predicates(list(zip(cut, types)), preds))
                rows_in, got_rows = dec.selection()
                assert rows_in == hi - lo and np.array_equal(got_rows, idx)
                for i, c in enumerate(cols):
                    col = f.columns[c]
                    WC.assert_window_equal(dec.fetch(i, col.physical_type, col.max_def, col.max_rep), FC.take_rows(cut[i], idx),
                                           f"{name} rows [{lo}, {hi}) {preds} col {c}")
        assert mixed >= 2


def test_chars_rerun_keeps_the_filter(dec, tmp_path):
    """Dictionary strings whose decoded chars exceed the first-pass arena: pf_wait grows it and runs the batch again,
    window and filter stages included, with the predicate on the string column itself."""
    rows, page = 4000, 1000
    entries = [bytes([65 + i]) * 8000 for i in range(4)]
    ch = K.Chunk("big", K.BYTE_ARRAY, optional=True, layout=K.LAYOUTS["e"])
    ch.set_dictionary(entries)
    rng = np.random.default_rng(5)
    for _ in range(rows // page):
        present = rng.random(page) >= 0.3
        ids = rng.integers(0, 4, int(present.sum()))
        ch.add_page(K.RLE_DICTIONARY, K.dict_indices(ids, 2), present=present, vals=[entries[int(i)] for i in ids])
    path = _write([ch], rows, str(tmp_path / "big.parquet"))
    exp = _expected(ch)
    assert len(exp["chars"]) > (16 << 20) + 2 * os.path.getsize(path)
    for windows, preds in (([(1003, 500)], [(0, RANGE, b"B", b"D")]), (None, [(0, RANGE, b"D", None)])):
        fresh = GpuDecoder(0)   # (a context whose arena has not grown yet)
        try:
            check_filtered(fresh, path, [exp], [K.BYTE_ARRAY], preds, windows, label="chars rerun")
            assert fresh.chars_reruns() == 1
            check_filtered(fresh, path, [exp], [K.BYTE_ARRAY], [(0, IS_NULL, None, None)], windows, label="after the rerun")
            assert fresh.chars_reruns() == 0
        finally:
            fresh.close()


# ---- no predicates, state ---------------------------------------------------------------------------------------------

def test_no_predicates_is_the_windowed_decode(dec, flat_file, stage):
    path, exp, types, chunks = flat_file
    n = len(exp)
    _f, descs, buf, total, ty = stage(path, 0, list(range(n)))
    for windows in (None, [(0, -1)] * n, [(13, 200)] * n):
        dec.decode(descs, buf.ptr.value, total, windows=windows)
        assert dec.wait() == 0
        a = [dec.fetch(i, *t) for i, t in enumerate(ty)]
        stages_a = dec.timing()
        dec.decode(descs, buf.ptr.value, total, windows=windows, predicates=[])
        assert dec.wait() == 0
        b = [dec.fetch(i, *t) for i, t in enumerate(ty)]
        assert list(stages_a) == list(dec.timing()) and dec.filter_ms() == 0
        for c in range(n):
            assert a[c].keys() == b[c].keys()
            for k in a[c]:
                assert np.array_equal(np.asarray(a[c][k]), np.asarray(b[c][k])), (windows, c, k)
        assert lib().pf_selection_info_get(dec.h, C.byref(SelectionInfo())) == STATE
        if windows is None or windows[0] == (0, -1):   # batch copies still allowed
            for g, e in zip(dec.fetch_batch(ty), exp):
                WC.assert_window_equal(g, e, "fetch_batch after predicates=[]")


def test_batch_copy_is_refused_after_a_filter_and_the_context_recovers(dec, flat_file, stage):
    path, exp, types, chunks = flat_file
    n = len(exp)
    check_filtered(dec, path, exp, types, [(IDX, RANGE, 10, 20)], label="before the gates")
    size = C.c_size_t()
    pinned = PinnedBuffer(dec.h, 1 << 20)
    try:
        assert lib().pf_batch_bytes(dec.h, C.byref(size)) == STATE
        assert lib().pf_copy_batch_async(dec.h, pinned.ptr, pinned.nbytes) == STATE
        assert lib().pf_column_info_host(dec.h, 0, pinned.ptr, C.byref(ColumnInfo())) == STATE
    finally:
        pinned.free()
    small = np.zeros(5, np.int32)
    assert lib().pf_copy_selection(dec.h, small.ctypes.data, small.nbytes) == -6   # PF_ERR_CAPACITY: 11 rows need 44 bytes
    _f, descs, buf, total, ty = stage(path, 0, list(range(n)))
    dec.decode(descs, buf.ptr.value, total)
    assert dec.wait() == 0 and lib().pf_batch_bytes(dec.h, C.byref(size)) == 0
    for g, e in zip(dec.fetch_batch(ty), exp):
        WC.assert_window_equal(g, e, "plain decode after a filter")


# ---- errors ----------------------------------------------------------------------------------------------------------

def _raw_pred(chunk, op, lo=None, hi=None, lo_len=None, hi_len=None):
    p = Predicate()
    p.chunk, p.op = chunk, op
    keep = []
    for side, b, n in (("lo", lo, lo_len), ("hi", hi, hi_len)):
        if b is not None:
            raw = C.create_string_buffer(bytes(b), max(1, len(b)))
            keep.append(raw)
            setattr(p, side, C.addressof(raw))
            setattr(p, side + "_len", len(b) if n is None else n)
    return p, keep


def test_call_errors_enqueue_nothing(dec, flat_file, oracle, stage):
    path, exp, types, chunks = flat_file
    n = len(exp)
    L = lib()
    _f, descs, buf, total, ty = stage(path, 0, list(range(n)))
    arr = (ChunkDesc * n)(*descs)
    i32, i64, dbl, flo = (_col(chunks, t, False) for t in (K.INT32, K.INT64, K.DOUBLE, K.FLOAT))
    boo, s = _col(chunks, K.BOOLEAN, False), _col(chunks, K.BYTE_ARRAY, False)
    four, eight = b"\x01\x00\x00\x00", b"\x01" + b"\x00" * 7
    bad = [(_raw_pred(n, NOT_NULL), INVALID_ARG), (_raw_pred(-1, NOT_NULL), INVALID_ARG), (_raw_pred(i32, 3), INVALID_ARG),
           (_raw_pred(i32, -1), INVALID_ARG), (_raw_pred(i32, IS_NULL, lo=four), INVALID_ARG), (_raw_pred(i32, NOT_NULL, hi=four), INVALID_ARG),
           (_raw_pred(i32, RANGE, lo=eight), INVALID_ARG), (_raw_pred(i64, RANGE, hi=four), INVALID_ARG), (_raw_pred(dbl, RANGE, lo=four), INVALID_ARG),
           (_raw_pred(flo, RANGE, lo=eight), INVALID_ARG), (_raw_pred(boo, RANGE, lo=four), INVALID_ARG), (_raw_pred(boo, RANGE, lo=b"\x02"), INVALID_ARG),
           (_raw_pred(i32, RANGE, lo=b""), INVALID_ARG), (_raw_pred(s, RANGE, lo=b"x" * 4097), INVALID_ARG),
           (_raw_pred(s, RANGE, hi=b"x", hi_len=-1), INVALID_ARG)]
    for (p, _keep), want in bad:
        one = (Predicate * 1)(p)
        assert L.pf_decode_row_group_filter(dec.h, arr, n, None, one, 1, buf.ptr, total, 0) == want
        assert L.pf_wait(dec.h) == STATE   # nothing was enqueued
    ok = (Predicate * 9)(*[_raw_pred(i32, NOT_NULL)[0]] * 9)
    for count in (-1, 9):
        assert L.pf_decode_row_group_filter(dec.h, arr, n, None, ok, count, buf.ptr, total, 0) == INVALID_ARG
        assert L.pf_wait(dec.h) == STATE
    assert L.pf_decode_row_group_filter(dec.h, arr, n, None, None, 1, buf.ptr, total, 0) == INVALID_ARG
    win = (RowWindow * n)(*[RowWindow(-1, 5)] * n)
    assert L.pf_decode_row_group_filter(dec.h, arr, n, win, ok, 1, buf.ptr, total, 0) == INVALID_ARG
    assert L.pf_wait(dec.h) == STATE
    # bounds of 4095 and 4096 bytes are fine
    for k in (0, 1, 4095, 4096):
        check_filtered(dec, path, exp, types, [(s, RANGE, b"a" * k, None)], label=f"bound of {k} bytes")
    # unsupported types: a predicate on a repeated column; a range over INT96 and FIXED_LEN_BYTE_ARRAY (IS_NULL is fine)
    nested = os.path.join(GOLDEN, "list_prim.parquet")
    _f, d2, b2, t2, ty2 = stage(nested, 0, [0])
    one = (Predicate * 1)(_raw_pred(0, NOT_NULL)[0])
    assert L.pf_decode_row_group_filter(dec.h, (ChunkDesc * 1)(*d2), 1, None, one, 1, b2.ptr, t2, 0) == UNSUPPORTED_TYPE
    assert L.pf_wait(dec.h) == STATE
    edge = os.path.join(GOLDEN, "edge_types_v2.parquet")
    with ParquetFile(edge) as f:
        kinds = {c.physical_type: c.index for c in f.columns if c.max_rep == 0}
    assert 3 in kinds and 7 in kinds
    with oracle.open(edge) as of:
        for pt in (3, 7):
            _f, d3, b3, t3, ty3 = stage(edge, 0, [kinds[pt]])
            one = (Predicate * 1)(_raw_pred(0, RANGE, lo=b"\x00" * 12)[0])
            assert L.pf_decode_row_group_filter(dec.h, (ChunkDesc * 1)(*d3), 1, None, one, 1, b3.ptr, t3, 0) == UNSUPPORTED_TYPE
            assert L.pf_wait(dec.h) == STATE
            e = of.decode(0, kinds[pt])
            dec.decode(d3, b3.ptr.value, t3, predicates=[(0, NOT_NULL, None, None)])
            assert dec.wait() == 0, dec.error()
            idx = np.flatnonzero(FC.present_of(e))
            WC.assert_window_equal(dec.fetch(0, *ty3[0]), FC.take_rows(e, idx), f"NOT_NULL over physical type {pt}")
            assert np.array_equal(dec.selection()[1], idx)
    # and the context still decodes
    check_filtered(dec, path, exp, types, [(i32, RANGE, 0, 10)], label="after the call errors")


def test_per_chunk_statuses(dec, flat_file, oracle, stage):
    path, exp, types, chunks = flat_file
    n = len(exp)
    cols = list(range(n))
    i32, s = _col(chunks, K.INT32, False), _col(chunks, K.BYTE_ARRAY, False)
    # a payload chunk whose row count differs: its own INVALID_ARG, the others are filtered
    wins = [(10, 20)] * n
    wins[3] = (10, 21)
    preds = [(i32, RANGE, None, 0)]
    rc, got, rows_in, rows = filtered(dec, path, cols, preds, wins)
    assert rc == INVALID_ARG and rows_in == 20
    cut = [WC.slice_chunk(e, 10, 20) for e in exp]
    idx = np.flatnonzero(FC.eval_predicates(list(zip(cut, types)), preds))
    assert np.array_equal(rows, idx)
    for c in cols:
        if c == 3:
            assert got[c]["status"] == INVALID_ARG
        else:
            WC.assert_window_equal(got[c], FC.take_rows(cut[c], idx), f"neighbour {c} of a row-count mismatch")
    # a payload chunk whose window fails: its own status stays
    wins[3] = (990, 20)
    rc, got, _ri, _r = filtered(dec, path, cols, preds, wins)
    assert rc == INVALID_ARG and [g["status"] for g in got] == [INVALID_ARG if c == 3 else 0 for c in cols]
    # a predicate chunk that fails to window, or whose row count differs from the first predicate's: every chunk takes it
    for bad in ((990, 20), (10, 21)):
        wins = [(10, 20)] * n
        wins[s] = bad
        rc, got, rows_in, rows = filtered(dec, path, cols, [(i32, RANGE, None, 0), (s, RANGE, b"a", None)], wins)
        assert rc == INVALID_ARG and all(g["status"] == INVALID_ARG for g in got) and len(rows) == 0
        assert dec.selection_info().status == INVALID_ARG
    # a corrupt predicate chunk hands its decode status to all chunks; as a payload its failure stays its own
    _f, descs, buf, total, ty = stage(path, 0, cols)
    victim = next(c for c, ch in enumerate(chunks) if ch.layout.codec == K.SNAPPY and c not in (i32, s))
    d = descs[victim]
    pg = d.pages[1]
    raw = buf.array()
    raw[d.chunk_offset + pg.offset:d.chunk_offset + pg.offset + pg.compressed_size] = 0xFF
    dec.decode(descs, buf.ptr.value, total)
    assert dec.wait() != 0
    status = dec.info(victim).status
    assert status != 0 and all(dec.info(c).status == 0 for c in cols if c != victim)
    dec.decode(descs, buf.ptr.value, total, predicates=[(victim, NOT_NULL, None, None)])
    assert dec.wait() == status and all(dec.info(c).status == status for c in cols)
    assert dec.selection_info().status == status and dec.selection_info().rows_selected == 0
    dec.decode(descs, buf.ptr.value, total, predicates=[(i32, RANGE, _plain(0, K.INT32), None)])
    assert dec.wait() == status
    idx = np.flatnonzero(FC.eval_predicates(list(zip(exp, types)), [(i32, RANGE, 0, None)]))
    for c in cols:
        if c == victim:
            assert dec.info(c).status == status
        else:
            WC.assert_window_equal(dec.fetch(c, *ty[c]), FC.take_rows(exp[c], idx), f"neighbour {c} of a corrupt payload chunk")
    # a nested payload chunk (list_prim: xs list<int32>, a flat INT64 beside it): UNSUPPORTED_TYPE, its flat sibling is filtered
    nested = os.path.join(GOLDEN, "list_prim.parquet")
    with oracle.open(nested) as of:
        e = of.decode(0, 1)
    assert "rep_levels" not in e
    _f, d2, b2, t2, ty2 = stage(nested, 0, [0, 1])
    assert ty2[0][2] == 1 and ty2[1][2] == 0
    keys = FC.values_of(e, K.INT64)
    mid = int(np.sort(keys)[len(keys) // 2])
    dec.decode(d2, b2.ptr.value, t2, predicates=[(1, RANGE, _plain(mid, K.INT64), None)])
    assert dec.wait() == UNSUPPORTED_TYPE and dec.info(0).status == UNSUPPORTED_TYPE and dec.info(1).status == 0
    idx = np.flatnonzero(FC.eval_predicates([(e, K.INT64)], [(0, RANGE, mid, None)]))
    assert 0 < len(idx) < len(keys) and np.array_equal(dec.selection()[1], idx)
    WC.assert_window_equal(dec.fetch(1, *ty2[1]), FC.take_rows(e, idx), "flat sibling of a nested payload")
    # the context still decodes
    check_filtered(dec, path, exp, types, [(i32, RANGE, 0, 10)], label="after the failures")


# ---- end to end: the reader -------------------------------------------------------------------------------------------

from pfloor import writer as W   # noqa: E402
from pfloor.predicate import Eq, IsNull, NotNull, Range   # noqa: E402
from pfloor.reader import Hydrator, HydratorSupplier, IllegalArgumentException, ParquetReader   # noqa: E402

E2E_RG, E2E_ROWS = 3, 4000


class _Rows(Hydrator):
    def start(self):
        return []

    def add(self, target, heading, value):
        target.append((heading, value))
        return target

    def finish(self, target):
        return tuple(target)


@pytest.fixture(scope="module")
def e2e_file(dec, tmp_path_factory):
    """3 row groups of 4,000 rows, pages of 500: k sorted with gaps (page index + Bloom filter), d an unsorted nullable
    double, s a nullable string. Returns the path and the written values per row."""
    schema = W.MessageType("rowfilter", W.required(W.INT64).named("k"), W.optional(W.DOUBLE).named("d"),
                           W.optional(W.BINARY).as_string().named("s"))
    path = str(tmp_path_factory.mktemp("rowfilter_e2e") / "e2e.parquet")
    w = W.ParquetWriter(schema, path, None, decoder=dec, page_index=True, page_rows=500, bloom_filters={"k": True})
    rng = np.random.default_rng(77)
    ks, ds, ss = [], [], []
    for g in range(E2E_RG):
        k = 1_000_000 * g + 3 * np.arange(E2E_ROWS, dtype=np.int64) + 7
        d = rng.random(E2E_ROWS)
        dv = rng.random(E2E_ROWS) >= 0.2
        sv = rng.random(E2E_ROWS) >= 0.25
        words = [b"s%d" % (i % 23) for i in range(E2E_ROWS)]
        offs = np.zeros(E2E_ROWS + 1, np.int32)
        np.cumsum([len(x) if ok else 0 for x, ok in zip(words, sv)], out=offs[1:])
        chars = np.frombuffer(b"".join(x for x, ok in zip(words, sv) if ok), np.uint8)
        w.write_columns({"k": k, "d": (d, np.packbits(dv, bitorder="little")), "s": (offs, chars, np.packbits(sv, bitorder="little"))},
                        E2E_ROWS)
        ks += [int(x) for x in k]
        ds += [float(x) if ok else None for x, ok in zip(d, dv)]
        ss += [x.decode() if ok else None for x, ok in zip(words, sv)]
    w.close()
    return path, ks, ds, ss


def _page_of(f, rg, row, col=0):
    """(row_lo, row_hi) of the data page of column col that holds the row, from the file's own OffsetIndex."""
    first = [r for _o, _s, r in f.page_index(rg, col)["offset_index"]]
    return next(p for p in WC.page_rows(first, f.row_group_rows(rg)) if p[0] <= row < p[1])


def _collect(path, **kw):
    with ParquetReader.streamContent(path, HydratorSupplier.constantly(_Rows()), **kw) as s:
        got = s.collect()
        return got, dict(s.reader.filter_stats)


def test_reader_where(dec, e2e_file):
    path, ks, ds, ss = e2e_file
    whole, stats = _collect(path)
    assert len(whole) == E2E_RG * E2E_ROWS and [dict(r)["k"] for r in whole] == ks
    assert [dict(r)["s"] for r in whole] == ss and stats["rows_decoded"] == 0
    size = os.path.getsize(path)
    # a present key: one page of one row group is decoded, the other two row groups are skipped by the index
    at = E2E_ROWS + 1234
    got, stats = _collect(path, where=[Eq("k", ks[at])])
    assert got == [whole[at]]
    assert stats["row_groups_skipped_index"] == 2 and stats["row_groups_skipped_bloom"] == 0
    with ParquetFile(path) as f:
        page = _page_of(f, 1, 1234)
    assert 490 <= page[1] - page[0] <= 510   # (page_rows = 500, as the writer rounds it)
    assert stats["rows_selected"] == 1 and stats["rows_decoded"] == page[1] - page[0] and 0 < stats["bytes_read"] < size
    # an absent key inside a page's [min, max]: the index keeps its row group, the Bloom filter drops it
    got, stats = _collect(path, where=[Eq("k", ks[at] + 1)])
    assert got == [] and stats["row_groups_skipped_index"] == 2 and stats["row_groups_skipped_bloom"] == 1
    assert stats["rows_decoded"] == 0 and stats["rows_selected"] == 0
    # a predicate column outside the projection, an unsorted column the index cannot narrow
    want = [i for i in range(len(ks)) if ds[i] is not None and 0.25 <= ds[i] <= 0.5 and ss[i] is not None]
    got, stats = _collect(path, columns=["k", "s"], where=[Range("d", 0.25, 0.5), NotNull("s")])
    assert got == [tuple(x for x in whole[i] if x[0] in ("k", "s")) for i in want] and len(want) > 100
    assert all(h in ("k", "s") for r in got for h, _v in r)   # the Hydrator never saw d
    assert stats["row_groups_skipped_index"] == 0 and stats["rows_decoded"] == len(ks) and stats["rows_selected"] == len(want)
    # rows= first, then where=
    lo, hi = E2E_ROWS - 700, 2 * E2E_ROWS + 300
    want = [i for i in range(lo, hi) if ds[i] is None and ks[lo + 5] <= ks[i] <= ks[hi - 40]]
    got, stats = _collect(path, rows=(lo, hi), where=[IsNull("d"), Range("k", ks[lo + 5], ks[hi - 40])])
    assert got == [whole[i] for i in want] and len(want) > 100
    assert stats["rows_decoded"] < hi - lo + 1000 and stats["rows_selected"] == len(want)
    got, stats = _collect(path, rows=(10, 20), where=[Eq("k", ks[15])])
    assert got == [whole[15]]
    got, stats = _collect(path, rows=(10, 20), where=[Eq("k", ks[25])])   # the key exists, outside the rows
    assert got == [] and stats["rows_selected"] == 0
    # a row group that selects nothing is passed over
    got, stats = _collect(path, where=[Range("d", 2.0, None)])
    assert got == [] and stats["rows_decoded"] == len(ks)
    with pytest.raises(IllegalArgumentException):
        ParquetReader.streamContent(path, HydratorSupplier.constantly(_Rows()), where=[Eq("nope", 1)])
    with pytest.raises(IllegalArgumentException):
        ParquetReader.streamContent(os.path.join(GOLDEN, "list_prim.parquet"), HydratorSupplier.constantly(_Rows()), where=[NotNull(1)])


def test_prune_bloom_probe_and_decode_file_where(dec, e2e_file):
    from pfloor.decoder import decode_file
    path, ks, ds, ss = e2e_file
    with ParquetFile(path) as f:
        for g in range(E2E_RG):
            k = ks[g * E2E_ROWS + 2100]
            assert f.bloom_probe(g, 0, int(k).to_bytes(8, "little", signed=True)) is True
            assert f.bloom_probe(g, 0, int(k + 1).to_bytes(8, "little", signed=True)) is False
            assert f.bloom_probe(g, 1, b"\x00" * 8) is None
            page = _page_of(f, g, 2100)
            a, b = page
            assert f.prune_row_group(g, [Eq("k", k)]) == page
            assert f.prune_row_group(g, [Eq("k", k + 1)]) is None and f._prune(g, [Eq("k", k + 1)])[1] == "bloom"
            assert f.prune_row_group(g, [Eq("k", k)], 0, a) is None and f.prune_row_group(g, [Eq("k", k)], a + 50, b - 50) == (a + 50, b - 50)
            assert f.prune_row_group(g, [Range("k", None, ks[g * E2E_ROWS] - 1)]) is None
            assert f.prune_row_group(g, [Range("k", ks[g * E2E_ROWS + 600], ks[g * E2E_ROWS + 1700]), NotNull("s"), Range("d", 0.1, 0.2)]) == \
                (_page_of(f, g, 600)[0], _page_of(f, g, 1700)[1])
            assert f.prune_row_group(g, [IsNull("d")]) == (0, E2E_ROWS)
    g = 2
    base = g * E2E_ROWS
    out = decode_file(path, row_groups=[g], columns=[0, 2], decoder=dec, where=[Range("k", ks[base + 990], ks[base + 1010]), Range("d", 0.5, None)])
    with ParquetFile(path) as f:
        span = (_page_of(f, g, 990)[0], _page_of(f, g, 1010)[1])
    assert out["_status"] == 0 and out["_range"] == span and span[0] < 990 and span[1] > 1011
    want = [i for i in range(990, 1011) if ds[base + i] is not None and ds[base + i] >= 0.5]
    rows_in, sel = out["_selection"]
    assert rows_in == span[1] - span[0] and list(sel) == want and len(want) > 3 and set(out) >= {(g, 0), (g, 2)} and (g, 1) not in out
    WC.assert_window_equal(out[(g, 0)], WC.canonical_fixed([ks[base + i] for i in want], np.int64, False), "decode_file where, k")
    WC.assert_window_equal(out[(g, 2)], WC.canonical_strings([ss[base + i] for i in want], True), "decode_file where, s")
    out = decode_file(path, row_groups=[g], decoder=dec, where=[Eq("k", ks[base] - 1)])
    assert out["_range"] is None and out["_selection"][0] == 0 and (g, 0) not in out


def test_async_column_copies_describe_the_selection(dec, flat_file, stage):
    """pf_copy_columns_async after a filtered decode: capacities are those of the selection, one byte less is refused."""
    from pfloor._native import ColumnOut
    path, exp, types, chunks = flat_file
    n = len(exp)
    _f, descs, buf, total, ty = stage(path, 0, list(range(n)))
    i64o, so = _col(chunks, K.INT64, True), _col(chunks, K.BYTE_ARRAY, True)
    preds = [(IDX, RANGE, 100, 612)]
    dec.decode(descs, buf.ptr.value, total, predicates=[(IDX, RANGE, _plain(100, K.INT32), _plain(612, K.INT32))])
    assert dec.wait() == 0, dec.error()
    idx = np.flatnonzero(FC.eval_predicates(list(zip(exp, types)), preds))
    want = [FC.take_rows(exp[c], idx) for c in (i64o, so)]
    outs = (ColumnOut * 2)()
    arrs = []
    for k, (c, w) in enumerate(zip((i64o, so), want)):
        ci = dec.info(c)
        assert (ci.num_rows, ci.num_slots, ci.num_entries, ci.num_values, ci.num_chars) == (513, 513, 513, w["num_values"], w["num_chars"])
        got = {name: np.full(len(np.asarray(w[name]).view(np.uint8).ravel()), 0xEE, np.uint8) for name in ("values", "validity", "offsets", "chars") if name in w}
        for name, a in got.items():
            setattr(outs[k], name, a.ctypes.data if a.size else None)
            setattr(outs[k], name + "_cap", a.nbytes)
        arrs.append(got)
    which = (C.c_int * 2)(i64o, so)
    assert lib().pf_copy_columns_async(dec.h, 2, which, outs) == 0 and lib().pf_sync(dec.h) == 0
    for got, w in zip(arrs, want):
        for name, a in got.items():
            assert np.array_equal(a, np.asarray(w[name]).view(np.uint8).ravel()), name
    outs[1].chars_cap -= 1
    assert lib().pf_copy_columns_async(dec.h, 2, which, outs) == -6   # PF_ERR_CAPACITY, nothing enqueued
    assert lib().pf_sync(dec.h) == 0
