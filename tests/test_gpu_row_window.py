"""Row windows on the GPU: pf_decode_row_group_rows cuts decoded chunks to rows [skip, skip + take) before they cross
the link (k_win_bounds / k_win_copy, csrc/pf_window.hip). The expected arrays never come from the code under test:
the oracle's decode of the whole chunk, pagekit's expected arrays, or the arrays a file was written from, cut by
window_cases.slice_chunk (plain numpy); every comparison is bit-exact, padding bits included."""
import ctypes as C
import os

import numpy as np
import pytest

import pagekit as K
import window_cases as WC
from conftest import GOLDEN
from pfloor import writer as W
from pfloor._native import ChunkDesc, ColumnInfo, RowWindow, lib
from pfloor.decoder import GpuDecoder, ParquetFile, PinnedBuffer
from pfloor.reader import Hydrator, HydratorSupplier, IllegalArgumentException, ParquetReader, RowGroupPipeline

pytestmark = pytest.mark.gpu

WIN_TILE = WC.WIN_TILE   # k_win_copy: output bytes of one array per workgroup round (csrc/pf_internal.h)
INVALID_ARG, CORRUPT_PAGE, STATE = -1, -2, -9


@pytest.fixture(scope="module")
def dec():
    d = GpuDecoder(0)
    yield d
    d.close()


def decode_whole_chunks(dec, path, rg, cols, windows, call="rows"):
    """The whole-chunk path: every page of the chunks goes up, the windows trim (indexed = 0)."""
    with ParquetFile(path) as f:
        items, total = f.plan([rg], cols)
        buf = dec.staging(total)
        descs = []
        for _rg, col, s, n, off in items:
            if n:
                f.read_into(s, n, buf.ptr.value + off)
            descs.append(f.chunk_desc(rg, col, off))
        if call == "plain":
            dec.decode(descs, buf.ptr.value, max(total, 1))
        else:
            dec.decode(descs, buf.ptr.value, max(total, 1), windows=windows)
        rc = dec.wait()
        return rc, [dec.fetch(i, f.columns[c].physical_type, f.columns[c].max_def, f.columns[c].max_rep)
                    for i, c in enumerate(cols)]


def decode_indexed(dec, path, rg, cols, lo, hi):
    """The indexed path: ParquetFile.plan_rows, so only the dictionary page and the selected pages reach the GPU."""
    with ParquetFile(path) as f:
        items, total, windows = f.plan_rows(rg, cols, lo, hi)
        buf = dec.staging(total)
        buf.array()[:max(total, 1)] = 0xEE   # nothing of an earlier batch left between the ranges
        nread = f.read_rows(items, buf.ptr.value)
        dec.decode([d for _c, d, _r, _o in items], buf.ptr.value, max(total, 1), windows=windows)
        rc = dec.wait()
        out = [dec.fetch(i, f.columns[c].physical_type, f.columns[c].max_def, f.columns[c].max_rep) for i, c in enumerate(cols)]
        return rc, out, [r for _c, _d, r, _o in items], nread


# ---- flat chunks, whole-chunk path: hand-assembled pages -------------------------------------------------------------

ROWS, PAGE = 1000, 96
NULL_PAGE = 3   # data page 3 (rows 288 .. 383) of every OPTIONAL chunk is all null


def _flat_chunks(oracle, rows=ROWS, page=PAGE, types=None):
    rng = np.random.default_rng(42)
    words = [b"", b"a", b"", b"row", b"window", b"MI355X-gfx950", b"x" * 37]
    chunks = []
    types = types or (K.INT32, K.INT64, K.DOUBLE, K.BOOLEAN, K.BYTE_ARRAY)
    for ptype in types:
        for optional in (False, True):
            # v1 uncompressed, v2 Snappy, v2 uncompressed in turn
            layout = K.LAYOUTS["ace"[(ptype + optional) % 3]]
            ch = K.Chunk(f"t{ptype}{'o' if optional else 'r'}", ptype, optional=optional, layout=layout,
                         compress=oracle.snappy_compress)
            for pg, a in enumerate(range(0, rows, page)):
                n = min(page, rows - a)
                present = None
                if optional:
                    present = rng.random(n) >= 0.3
                    if pg == NULL_PAGE:
                        present[:] = False
                nv = n if present is None else int(present.sum())
                if ptype == K.BYTE_ARRAY:
                    vals = [words[int(i)] for i in rng.integers(0, len(words), nv)]
                elif ptype == K.BOOLEAN:
                    vals = rng.integers(0, 2, (nv, 1)).astype(np.uint8)
                else:
                    vals = rng.integers(0, 256, (nv, K.width_of(ptype))).astype(np.uint8)
                ch.add_page(K.PLAIN, K.plain(ptype, vals), present=present, vals=vals)
            chunks.append(ch)
    return chunks


def _expected(ch):
    e = ch.expected()
    e["width"] = 0 if ch.ptype == K.BYTE_ARRAY else ch.width
    return e


@pytest.fixture(scope="module")
def flat_file(oracle, tmp_path_factory):
    chunks = _flat_chunks(oracle)
    data, _info = K.build_file(chunks, ROWS)
    path = str(tmp_path_factory.mktemp("rowwin") / "flat.parquet")
    with open(path, "wb") as f:
        f.write(data)
    return path, [_expected(ch) for ch in chunks], chunks


def _run_windows(dec, path, exp, windows_per_chunk, label):
    """windows_per_chunk: one (skip, take) per chunk, all in one batch."""
    rc, got = decode_whole_chunks(dec, path, 0, list(range(len(exp))), windows_per_chunk)
    assert rc == 0, dec.error()
    for c, (g, e, (skip, take)) in enumerate(zip(got, exp, windows_per_chunk)):
        assert g["status"] == 0
        WC.assert_window_equal(g, WC.slice_chunk(e, skip, take), f"{label} chunk {c} window ({skip}, {take})")


def test_flat_every_bit_alignment(dec, flat_file):
    """skip % 8 x take % 8, takes around 64 so the funnel shift crosses a 64-bit word, skips around a word edge."""
    path, exp, _chunks = flat_file
    for s in range(8):
        for t in range(8):
            _run_windows(dec, path, exp, [(184 + s + 8 * (c % 3), 60 + t) for c in range(len(exp))], "bits")


def test_flat_edges_identity_and_tiles(dec, flat_file):
    path, exp, chunks = flat_file
    n = len(exp)
    for skip, take in ((0, 0), (0, 1), (999, 1), (0, ROWS), (0, -1), (1000, 0), (1000, -1), (7, -1), (500, 0)):
        _run_windows(dec, path, exp, [(skip, take)] * n, "edges")
    # the copy kernel's tile: WIN_TILE output bytes, so WIN_TILE / width rows of values (offsets: 4 bytes a row)
    for d in (-1, 0, 1):
        wins = []
        for ch in chunks:
            rows = WIN_TILE // (4 if ch.ptype == K.BYTE_ARRAY else ch.width) + d
            wins.append((3, rows) if 3 + rows <= ROWS else (3, WIN_TILE // 8 + d))
        _run_windows(dec, path, exp, wins, "tile")
    # a different window for every chunk of one batch, identity among them
    _run_windows(dec, path, exp, [(0, -1) if c % 4 == 0 else (c * 13, 100 + c) for c in range(n)], "mixed")


def test_flat_tile_of_narrow_types(dec, oracle, tmp_path):
    """INT32, BOOLEAN and BYTE_ARRAY need more than 1,000 rows to fill a tile of values, and a tile of validity bits
    is 8 * WIN_TILE rows: 33,000 rows in pages of 3,000."""
    rows = 33000
    chunks = _flat_chunks(oracle, rows, 3000, (K.INT32, K.BOOLEAN, K.BYTE_ARRAY))
    data, _ = K.build_file(chunks, rows)
    path = str(tmp_path / "narrow.parquet")
    with open(path, "wb") as f:
        f.write(data)
    exp = [_expected(ch) for ch in chunks]
    for d in (-1, 0, 1):
        wins = [(5, WIN_TILE // (4 if ch.ptype == K.BYTE_ARRAY else ch.width) + d) for ch in chunks]
        _run_windows(dec, path, exp, wins, "narrow tile")
        _run_windows(dec, path, exp, [(5, 8 * WIN_TILE + d)] * len(exp), "validity tile")


def test_flat_nulls_at_the_window_edges(dec, flat_file):
    path, exp, chunks = flat_file
    n = len(exp)
    opt = next(i for i, ch in enumerate(chunks) if ch.optional)
    valid = WC._bits(exp[opt]["validity"], ROWS).astype(bool)
    null = int(np.flatnonzero(~valid[400:])[0]) + 400
    a, b = NULL_PAGE * PAGE, (NULL_PAGE + 1) * PAGE
    for skip, take in ((null, 9), (null - 8, 9), (null, 1), (a - 3, 10), (b - 5, 10), (a, PAGE), (a - 1, PAGE + 2), (a + 10, 20)):
        _run_windows(dec, path, exp, [(skip, take)] * n, "nulls")


@pytest.mark.parametrize("name", ["edge_types_v1", "edge_types_v2"])
def test_flat_flba_int96_goldens(dec, oracle, name):
    path = os.path.join(GOLDEN, name + ".parquet")
    with oracle.open(path) as of:
        cols = list(range(of.num_columns))
        exp = [of.decode(0, c) for c in cols]
    rows = exp[0]["num_rows"]
    for skip, take in ((0, 1), (13, 71), (rows - 67, 67), (341, 342), (5, -1), (0, 0)):
        rc, got = decode_whole_chunks(dec, path, 0, cols, [(skip, take)] * len(cols))
        assert rc == 0, dec.error()
        for c in cols:
            WC.assert_window_equal(got[c], WC.slice_chunk(exp[c], skip, take), f"{name} col {c} ({skip}, {take})")


# ---- flat chunks, indexed path: files of the GPU writer ------------------------------------------------------------

def _written_columns(rows):
    rng = np.random.default_rng(11)
    ids = np.arange(rows, dtype=np.int64) * 3 + 7                      # unique: a big dictionary, or DELTA_BINARY_PACKED
    small = rng.integers(0, 50, rows).astype(np.int32)                 # dictionary-encoded either way
    x = rng.random(rows)
    valid = rng.random(rows) >= 0.3
    valid[192:288] = False                                             # a null page (page_rows = 96)
    words = [b"w%d" % (i % 17) if i % 5 else b"" for i in range(rows)]
    lens = np.array([len(w) if v else 0 for w, v in zip(words, valid)])
    offs = np.zeros(rows + 1, np.int32)
    np.cumsum(lens, out=offs[1:])
    chars = np.frombuffer(b"".join(w for w, v in zip(words, valid) if v), np.uint8)
    uniq = [b"u%07d-%s" % (i, b"z" * (i % 11)) for i in range(rows)]   # sorted, unique: DELTA_BYTE_ARRAY when it falls back
    uoffs = np.zeros(rows + 1, np.int32)
    np.cumsum([len(u) for u in uniq], out=uoffs[1:])
    vbits = np.packbits(valid, bitorder="little")
    cols = {"id": ids, "small": small, "x": (x, vbits), "s": (offs, chars, vbits), "u": (uoffs, np.frombuffer(b"".join(uniq), np.uint8))}
    exp = [WC.canonical_fixed(list(map(int, ids)), np.int64, False), WC.canonical_fixed(list(map(int, small)), np.int32, False),
           WC.canonical_fixed([float(v) if ok else None for v, ok in zip(x, valid)], np.float64, True),
           WC.canonical_strings([w if ok else None for w, ok in zip(words, valid)], True), WC.canonical_strings(uniq, False)]
    return cols, exp


SCHEMA = W.MessageType("rowwin", W.required(W.INT64).named("id"), W.required(W.INT32).named("small"),
                       W.optional(W.DOUBLE).named("x"), W.optional(W.BINARY).as_string().named("s"),
                       W.required(W.BINARY).as_string().named("u"))


@pytest.mark.parametrize("codec", [W.UNCOMPRESSED, W.SNAPPY, W.ZSTD], ids=["none", "snappy", "zstd"])
@pytest.mark.parametrize("route", ["dictionary", "plain_fallback", "delta_fallback"])
def test_indexed_files_of_the_gpu_writer(dec, tmp_path, codec, route):
    rows = 1000
    cols, exp = _written_columns(rows)
    path = str(tmp_path / "w.parquet")
    delta = route == "delta_fallback"
    w = W.ParquetWriter(SCHEMA, path, None, decoder=dec, codec=codec, delta_fallback=delta, page_index=True, page_rows=96)
    if route != "dictionary":   # a 4 KiB dictionary limit: the unique columns fall back, `small` and `s` stay dictionary
        encode = w.enc.encode
        w.enc.encode = lambda *a, **kw: encode(*a, dict_page_limit=4096, **kw)
    w.write_columns(cols, rows)
    routes = [tuple(r) for r in w.last_chunks]   # (dict_entries, data_encoding, fallback)
    w.close()
    if route == "dictionary":
        assert all(r[0] > 0 for r in routes), routes
    else:
        assert routes[1][0] > 0 and routes[0][0] == 0 and routes[4][0] == 0, routes
        assert (routes[0][1], routes[4][1]) == ((K.DELTA_BINARY_PACKED, K.DELTA_BYTE_ARRAY) if delta else (K.PLAIN, K.PLAIN)), routes
    whole = os.path.getsize(path)
    for lo, hi in ((0, 0), (0, 1), (0, rows), (999, 1000), (1000, 1000), (100, 130), (97, 192), (96, 97), (190, 290), (95, 481), (288, 300)):
        rc, got, infos, nread = decode_indexed(dec, path, 0, list(range(5)), lo, hi)
        assert rc == 0, dec.error()
        for c in range(5):
            assert infos[c].indexed == 1
            WC.assert_window_equal(got[c], WC.slice_chunk(exp[c], lo, hi - lo), f"codec {codec} {route} col {c} rows [{lo}, {hi})")
        assert nread == sum(r.dict_size + r.data_size for r in infos)
        if 0 < hi - lo <= 30:   # at most two of a chunk's eleven pages, and its dictionary page
            assert all(1 <= r.n_data_pages <= 2 for r in infos) and nread < whole


# ---- nested chunks -------------------------------------------------------------------------------------------------

def _nested_windows(a):
    """Windows that begin / end on an empty list, a null list and an ordinary one, one row, and spans."""
    rows = a["num_rows"]
    lo = np.asarray(a["list_offsets"])
    lv = WC._bits(a["list_validity"], rows).astype(bool)
    empty = np.flatnonzero((np.diff(lo) == 0) & lv)
    null = np.flatnonzero(~lv)
    full = np.flatnonzero(np.diff(lo) > 1)
    wins = [(0, 0), (0, 1), (rows - 1, 1), (rows, 0), (0, rows), (3, -1), (rows // 2, 1)]
    for idx in (empty, null, full):
        assert len(idx) > 2
        r = int(idx[len(idx) // 2])
        wins += [(r, 1), (r, min(9, rows - r)), (max(r - 8, 0), r - max(r - 8, 0) + 1), (r, 0)]
    return wins


@pytest.mark.parametrize("name", ["c5_nested", "list_prim"])
def test_nested_goldens_whole_chunk(dec, oracle, name):
    path = os.path.join(GOLDEN, name + ".parquet")
    with oracle.open(path) as of:
        cols = list(range(of.num_columns))
        exp = [of.decode(0, c) for c in cols]
    assert any("rep_levels" in e for e in exp)
    for skip, take in _nested_windows(next(e for e in exp if "rep_levels" in e)) + [(1, 1023), (2, 1024), (0, 1025)]:
        if skip + max(take, 0) > exp[0]["num_rows"]:
            continue
        rc, got = decode_whole_chunks(dec, path, 0, cols, [(skip, take)] * len(cols))
        assert rc == 0, dec.error()
        for c in cols:
            WC.assert_window_equal(got[c], WC.slice_chunk(exp[c], skip, take), f"{name} col {c} ({skip}, {take})")


@pytest.mark.parametrize("name", WC.FIXTURES)
def test_nested_fixtures_indexed(dec, oracle, name):
    """pyarrow's pages: row-aligned at irregular edges (145, 294, 409, ...), which the GPU writer never produces."""
    path = WC.fixture_path(name)
    with oracle.open(path) as of:
        exp = [of.decode(0, c) for c in range(3)]
    with ParquetFile(path) as f:
        first = [r for _o, _s, r in f.page_index(0, 2)["offset_index"]]
    rows = exp[0]["num_rows"]
    e = first[1:]
    assert any(x % 8 for x in e)
    ranges = [(0, 0), (0, 1), (0, rows), (rows - 1, rows), (rows, rows),
              (e[0] + 3, e[1] - 3), (e[0] + 5, e[1]), (e[1], e[1] + 7), (e[1] - 2, e[1] + 2), (e[0] - 1, e[2] + 1),   # 1, 1, 1, 2, 4 pages
              (e[3], e[4]), (e[3] + 1, e[3] + 2)]
    ranges += [(s, s + t) for s, t in _nested_windows(exp[2]) if t > 0 and s + t <= rows]
    seen_pages = set()
    for lo, hi in ranges:
        rc, got, infos, _n = decode_indexed(dec, path, 0, [0, 1, 2], lo, hi)
        assert rc == 0, (lo, hi, dec.error())
        seen_pages.add(infos[2].n_data_pages)
        for c in range(3):
            assert infos[c].indexed == 1
            WC.assert_window_equal(got[c], WC.slice_chunk(exp[c], lo, hi - lo), f"{name} col {c} rows [{lo}, {hi})")
    assert {0, 1, 2, len(first)} <= seen_pages


# ---- errors and state ------------------------------------------------------------------------------------------------

def test_window_past_the_end_fails_its_chunk_only(dec, flat_file):
    path, exp, _chunks = flat_file
    n = len(exp)
    for bad in ((990, 11), (1001, 0), (1001, -1), (0, 1001)):
        wins = [(10, 20)] * n
        wins[3] = bad
        rc, got = decode_whole_chunks(dec, path, 0, list(range(n)), wins)
        assert rc == INVALID_ARG
        for c in range(n):
            if c == 3:
                assert got[c]["status"] == INVALID_ARG
            else:
                WC.assert_window_equal(got[c], WC.slice_chunk(exp[c], 10, 20), f"neighbour {c} of a window past the end")


def test_bad_window_arguments_enqueue_nothing(dec, flat_file):
    path, exp, _chunks = flat_file
    with ParquetFile(path) as f:
        items, total = f.plan([0], [0, 1])
        buf = dec.staging(total)
        descs = (ChunkDesc * 2)(*[f.chunk_desc(0, c, off) for _rg, c, _s, _n, off in items])
        for _rg, _c, s, n, off in items:
            f.read_into(s, n, buf.ptr.value + off)
        for skip, take in ((-1, 5), (0, -2), (-3, -1)):
            win = (RowWindow * 2)(RowWindow(0, 5), RowWindow(skip, take))
            assert lib().pf_decode_row_group_rows(dec.h, descs, 2, win, buf.ptr, total, 0) == INVALID_ARG
            assert lib().pf_wait(dec.h) == STATE   # nothing was enqueued
    _run_windows(dec, path, exp, [(1, 2)] * len(exp), "after bad arguments")


def test_first_nested_page_that_starts_mid_row_is_corrupt(dec, oracle, tmp_path):
    """The levels and values of the v1 golden list_prim, less the first entry of its first row, in a hand-assembled
    page: the page starts with repetition level 1."""
    with oracle.open(os.path.join(GOLDEN, "list_prim.parquet")) as of:
        a = of.decode(0, 0)
    reps, defs = a["rep_levels"][:600], a["def_levels"][:600]
    assert reps[0] == 0 and reps[1] == 1 and defs[0] == 3
    vals_all = np.frombuffer(a["values"].tobytes(), np.uint8).reshape(-1, 4)
    valid = WC._bits(a["validity"], a["num_slots"]).astype(bool)

    def chunk(drop):
        ch = K.Chunk("xs", K.INT32, nested=True, layout=K.LAYOUTS["a"])
        r, d = reps[drop:], defs[drop:]
        nslots = int((defs >= 2).sum())
        v = vals_all[:nslots][valid[:nslots]][drop:]
        ch.add_page(K.PLAIN, K.plain(K.INT32, v), defs=d, reps=r, vals=v)
        return ch
    for drop, want in ((0, 0), (1, CORRUPT_PAGE)):
        ch = chunk(drop)
        rows = int((reps[drop:] == 0).sum())
        data, _ = K.build_file([ch], rows)
        path = str(tmp_path / f"mid{drop}.parquet")
        with open(path, "wb") as f:
            f.write(data)
        rc, got = decode_whole_chunks(dec, path, 0, [0], [(2, 5)])
        assert rc == want and got[0]["status"] == want
        if want == 0:
            WC.assert_window_equal(got[0], WC.slice_chunk(ch.expected() | {"width": 4}, 2, 5), "hand-assembled page, whole rows")


def test_batch_copy_is_refused_after_windows_and_the_context_recovers(dec, oracle):
    path = os.path.join(GOLDEN, "c2_lineitem.parquet")
    with oracle.open(path) as of:
        cols = list(range(of.num_columns))
        exp = [of.decode(0, c) for c in cols]
    rc, got = decode_whole_chunks(dec, path, 0, cols, [(100, 50)] * len(cols))
    assert rc == 0
    for c in cols:
        WC.assert_window_equal(got[c], WC.slice_chunk(exp[c], 100, 50), f"lineitem col {c}")
    n = C.c_size_t()
    pinned = PinnedBuffer(dec.h, 1 << 20)
    try:
        assert lib().pf_batch_bytes(dec.h, C.byref(n)) == STATE
        assert lib().pf_copy_batch_async(dec.h, pinned.ptr, pinned.nbytes) == STATE
        assert lib().pf_column_info_host(dec.h, 0, pinned.ptr, C.byref(ColumnInfo())) == STATE
    finally:
        pinned.free()
    # identity windows everywhere: no stage, batch copies allowed
    rc, _ = decode_whole_chunks(dec, path, 0, cols, [(0, -1)] * len(cols))
    assert rc == 0 and lib().pf_batch_bytes(dec.h, C.byref(n)) == 0
    # a plain decode on the same context equals one on a fresh context
    rc, again = decode_whole_chunks(dec, path, 0, cols, None, call="plain")
    fresh = GpuDecoder(0)
    try:
        rc2, ref = decode_whole_chunks(fresh, path, 0, cols, None, call="plain")
    finally:
        fresh.close()
    assert rc == 0 and rc2 == 0
    for c in cols:
        WC.assert_window_equal(again[c], ref[c], f"after windows, col {c}")
        WC.assert_window_equal(again[c], exp[c], f"after windows vs oracle, col {c}")


def test_chars_rerun_keeps_the_window(dec, tmp_path):
    """Dictionary strings whose decoded chars (about 2,800 x 8,000 bytes) exceed the first-pass arena (twice the page bytes
    + 16 MiB): pf_wait grows it and runs the batch again, window stage included."""
    rows, page = 4000, 1000
    entries = [bytes([65 + i]) * 8000 for i in range(4)]
    ch = K.Chunk("big", K.BYTE_ARRAY, optional=True, layout=K.LAYOUTS["e"])
    ch.set_dictionary(entries)
    rng = np.random.default_rng(5)
    for _ in range(rows // page):
        present = rng.random(page) >= 0.3
        ids = rng.integers(0, 4, int(present.sum()))
        ch.add_page(K.RLE_DICTIONARY, K.dict_indices(ids, 2), present=present, vals=[entries[int(i)] for i in ids])
    data, _ = K.build_file([ch], rows)
    path = str(tmp_path / "big.parquet")
    with open(path, "wb") as f:
        f.write(data)
    exp = _expected(ch)
    assert len(exp["chars"]) > (16 << 20) + 2 * len(data)
    fresh = GpuDecoder(0)   # (a context whose arena has not grown yet)
    try:
        for i, (skip, take) in enumerate(((1003, 77), (0, 1), (3990, 10))):
            rc, got = decode_whole_chunks(fresh, path, 0, [0], [(skip, take)])
            assert rc == 0, fresh.error()
            # the first decode overflows and pf_wait runs the batch, window stage included, once more; the context
            # remembers the size, so the later ones fit at once
            assert fresh.chars_reruns() == (1 if i == 0 else 0)
            WC.assert_window_equal(got[0], WC.slice_chunk(exp, skip, take), f"chars rerun ({skip}, {take})")
    finally:
        fresh.close()
    fresh = GpuDecoder(0)   # the rerun itself with a window at the chunk's end
    try:
        rc, got = decode_whole_chunks(fresh, path, 0, [0], [(3990, 10)])
        assert rc == 0 and fresh.chars_reruns() == 1, fresh.error()
        WC.assert_window_equal(got[0], WC.slice_chunk(exp, 3990, 10), "chars rerun (3990, 10), fresh context")
    finally:
        fresh.close()


@pytest.mark.parametrize("name", ["c2_lineitem", "c5_nested", "edge_types_v2"])
def test_null_windows_are_the_plain_decode(dec, name):
    path = os.path.join(GOLDEN, name + ".parquet")
    with ParquetFile(path) as f:
        cols = list(range(f.num_columns))
    rc_a, a = decode_whole_chunks(dec, path, 0, cols, None, call="plain")
    stages_a = dec.timing()
    rc_b, b = decode_whole_chunks(dec, path, 0, cols, None, call="rows")
    stages_b = dec.timing()
    assert rc_a == 0 and rc_b == 0 and list(stages_a) == list(stages_b) and len(stages_a) == 10
    assert dec.window_ms() == 0
    for c in cols:
        assert a[c].keys() == b[c].keys()
        for k in a[c]:
            assert np.array_equal(np.asarray(a[c][k]), np.asarray(b[c][k])), (name, c, k)


# ---- the reader ------------------------------------------------------------------------------------------------------

class _Rows(Hydrator):
    def start(self):
        return []

    def add(self, target, heading, value):
        target.append((heading, value))
        return target

    def finish(self, target):
        return tuple(target)


def test_reader_row_range(dec, tmp_path, monkeypatch):
    rows_rg, n_rg = 700, 3
    path = str(tmp_path / "three.parquet")
    w = W.ParquetWriter(SCHEMA, path, None, decoder=dec, page_index=True, page_rows=96)
    for g in range(n_rg):
        cols, _exp = _written_columns(rows_rg)
        cols["id"] = cols["id"] + 100000 * g
        w.write_columns(cols, rows_rg)
    w.close()
    total = rows_rg * n_rg
    sup = HydratorSupplier.constantly(_Rows())
    with ParquetReader.streamContent(path, sup) as s:
        whole = s.collect()
    assert len(whole) == total
    decoded = []
    real = GpuDecoder.decode

    def counting(self, descs, buf, nbytes, on_device=False, windows=None):
        decoded.append(None if windows is None else [tuple(x) for x in windows])
        return real(self, descs, buf, nbytes, on_device, windows)
    monkeypatch.setattr(GpuDecoder, "decode", counting)
    for lo, hi, n_decodes in ((750, 790, 1), (650, 760, 2), (5, total - 5, 3), (300, 300, 0), (0, total, 3), (700, 1400, 1),
                              (699, 701, 2), (0, 0, 0), (total, total, 0), (total - 1, total, 1)):
        decoded.clear()
        with ParquetReader.streamContent(path, sup, rows=(lo, hi)) as s:
            got = s.collect()
        assert got == whole[lo:hi], (lo, hi)
        assert len(decoded) == n_decodes, (lo, hi, decoded)   # row groups outside the range were never enqueued
        if (lo, hi) in ((0, total), (700, 1400)):
            assert all(wn is None for wn in decoded)        # whole row groups take the path they always took
    decoded.clear()
    with ParquetReader.streamContent(path, sup, ["id", "s"], rows=(690, 712)) as s:
        assert s.collect() == [tuple(x for x in r if x[0] in ("id", "s")) for r in whole[690:712]]
    closed = []
    real_close = ParquetFile.close
    monkeypatch.setattr(ParquetFile, "close", lambda self: (closed.append(bool(self.h)), real_close(self))[1])
    with pytest.raises(IllegalArgumentException):
        ParquetReader.streamContent(path, sup, rows=(5, total + 1))
    assert closed and closed[0]   # the constructor closed the file it had opened before it raised
    monkeypatch.setattr(ParquetFile, "close", real_close)
    # the pipeline on its own: a window per row group
    with ParquetFile(path) as f:
        colsel = [f.columns[0]]
        pipe = RowGroupPipeline(f, colsel, [0, 2], windows=[(10, 20), None])
        try:
            a = pipe.take(0)
            b = pipe.take(1)
        finally:
            pipe.close()
        assert a[0]["num_rows"] == 10 and b[0]["num_rows"] == rows_rg
        assert np.frombuffer(a[0]["values"].tobytes(), np.int64)[0] == 10 * 3 + 7
