"""The page index of the write path without a GPU (PF_ENCODE_PAGE_INDEX): the reference against pyarrow's
writer, the file writer (pf_writer_*) on hand-built chunks, the host parser (pf_file_column_index, pf_file_offset_index)
on our files and on pyarrow's, and the parser under AddressSanitizer + UBSan (tests/native/pf_pgindex_check.cpp)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pagekit as K
import pgindex_cases as P
import stats_cases as S
from conftest import ROOT

CSRC = os.path.join(ROOT, "parquet-floor_amd", "csrc")


@pytest.fixture(scope="module")
def W():
    from pfloor import writer
    writer.lib()
    return writer


def test_constants_are_the_headers(W):
    hdr = open(os.path.join(ROOT, "include", "pfloor.h")).read()
    assert int(re.search(r"#define PF_ENCODE_PAGE_INDEX\s+(\d+)", hdr).group(1)) == W.ENCODE_PAGE_INDEX == 32
    src = open(os.path.join(CSRC, "pf_enc_tables.h")).read()
    assert int(re.search(r"ST_LIMIT = (\d+);", src).group(1)) == P.LIMIT
    assert (W.UNORDERED, W.ASCENDING, W.DESCENDING) == (P.UNORDERED, P.ASCENDING, P.DESCENDING) == (0, 1, 2)


# ---------------------------------------------------------------- 1. the reference
def _file_index(path, col=0, rg=0):
    """(ColumnIndex fields or None, OffsetIndex fields, the ColumnChunk's fields) by stats_cases' Thrift reader."""
    raw = open(path, "rb").read()
    cc = S.footer(path)[4][rg][1][col]
    ci = S.read_struct(raw, cc[6]) if 6 in cc else None
    oi = S.read_struct(raw, cc[4])
    if ci is not None:
        assert ci[1] == cc[6] + cc[7], "column_index_length"
    assert oi[1] == cc[4] + cc[5], "offset_index_length"
    return (ci[0] if ci else None), oi[0], cc


def _pyarrow_file(case, path, **kw):
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    # one page per write_batch_size rows: a page is closed once its values reach data_page_size, null pages included
    pq.write_table(pa.table({"c": case.arrow()}), path, data_page_version="2.0", compression="NONE", use_dictionary=False,
                   write_page_index=True, write_batch_size=case.page_rows, data_page_size=0, row_group_size=1 << 20, **kw)


@pytest.mark.parametrize("name", [n for n in P.names() if P.cases()[n].pyarrow_expressible()])
def test_reference_is_what_pyarrow_writes(tmp_path, name):
    """Untruncated (T = -1), the reference's lists, order and validity are pyarrow's for every case it can express:
    fields 1-5 of ColumnIndex, first_row_index of OffsetIndex; a NaN-only page drops the ColumnIndex and keeps the
    OffsetIndex; an all-null chunk is UNORDERED; a single page ASCENDING."""
    case = P.cases()[name]
    path = str(tmp_path / "p.parquet")
    _pyarrow_file(case, path)
    ci, oi, _cc = _file_index(path)
    ref = case.ref(T=-1)
    assert [loc[3] for loc in oi[1]] == case.first_rows()
    assert (ci is not None) == ref["valid"]
    if ci is not None:
        got = P.column_index_fields(ci)
        assert {k: got[k] for k in ref} == ref
    if hasattr(case, "want_order"):
        assert ref["boundary_order"] == case.want_order


def test_pyarrow_layout_is_column_indexes_then_offset_indexes(tmp_path):
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    path = str(tmp_path / "two.parquet")
    pq.write_table(pa.table({"a": list(range(64)), "b": [float(i) for i in range(64)]}), path, write_page_index=True,
                   row_group_size=32, write_batch_size=8, data_page_size=0, use_dictionary=False)
    fm = S.footer(path)
    ccs = [cc for rg in fm[4] for cc in rg[1]]
    assert len(ccs) == 4
    ci, oi = [cc[6] for cc in ccs], [cc[4] for cc in ccs]
    assert ci == sorted(ci) and oi == sorted(oi) and ci[-1] + ccs[-1][7] == oi[0]


def test_reference_rules():
    """What pyarrow cannot pin: truncation, and the size limit without it."""
    T = P.truncate_max
    assert T(b"abcdef", 6) == b"abcdef" and T(b"abcdefg", 6) == b"abcdeg" and T(b"abcde\xffg", 6) == b"abcdf"
    assert T(b"a\xff\xff\xffz", 4) == b"b" and T(b"\xff\xff\xff\xffz", 4) is None and T(b"\xff\xff\xff\xff", 4) == b"\xff" * 4
    assert T(b"\xfe\xff\xff", 1) == b"\xff" and T(b"", 1) == b"" and T(b"x" * 9000, -1) == b"x" * 9000
    cs = P.cases()
    for name, valid in (("s_all_ff", False), ("s_all_ff_exactly_T", True), ("s_5000_T64", True), ("s_5000_no_truncation", False),
                        ("s_2047_2048_no_truncation", True), ("s_2048_2048_no_truncation", False), ("s_T1_ff", False),
                        ("f32_nan_only_page", False), ("f64_nan_only_with_nulls", False), ("f64_nan_mixed", True), ("i32_all_null", True)):
        assert cs[name].ref()["valid"] == valid, name
    r = cs["s_equal_after_truncation"].ref()
    assert r["max_values"] == [b"prefix_`"] * 3 and r["boundary_order"] == P.ASCENDING
    assert cs["s_equal_after_truncation"].ref(T=-1)["boundary_order"] == P.UNORDERED
    r = cs["s_carry"].ref()
    assert r["max_values"] == [b"abcdefh", b"abcdf", b"c"] and r["min_values"][2] == b"b" + b"\xff" * 7
    r = cs["s_5000_T64"].ref()
    assert r["max_values"][1] == b"m" * 63 + b"n" and r["min_values"][2] == b"m" * 64
    z = cs["f64_zeros"].ref()
    assert z["min_values"][0] == struct.pack("<d", -0.0) and z["max_values"][1] == struct.pack("<d", 0.0)
    assert cs["f32_zeros_tie"].ref()["boundary_order"] == P.ASCENDING
    assert cs["b_all_null"].ref()["boundary_order"] == P.UNORDERED and cs["i32_pages_1_ascending"].ref()["boundary_order"] == P.ASCENDING
    for name in P.names():
        if "_break_" in name:
            assert cs[name].ref()["boundary_order"] == P.UNORDERED, name


# ---------------------------------------------------------------- 2. the file writer on hand-built chunks
def _plain_page(ptype, page):
    """One uncompressed v2 PLAIN page of `page` (values, None = null): header + levels + values. OPTIONAL iff it can be."""
    vals = [v for v in page if v is not None]
    if ptype == K.BYTE_ARRAY:
        body = b"".join(struct.pack("<I", len(v)) + v for v in vals)
    else:
        body = np.asarray(vals, S._DT[ptype]).tobytes()
    return vals, body


def _chunk_bytes(ptype, pages, optional):
    """-> (chunk bytes, [(offset, size, first row)])."""
    out, locs, row = b"", [], 0
    for page in pages:
        vals, body = _plain_page(ptype, page)
        lv = b""
        if optional:
            groups = (len(page) + 7) // 8
            lv = S.w_uvarint((groups << 1) | 1) + np.packbits([v is not None for v in page], bitorder="little").tobytes()
        pg = S.w_page_header_v2(len(page), len(page) - len(vals), 0, len(lv), len(body)) + lv + body
        locs.append((len(out), len(pg), row))
        out += pg
        row += len(page)
    return out, locs


def _index_chunk(W, ptype, pages, optional, T=-1, with_index=True, bloom=None):
    body, locs = _chunk_bytes(ptype, pages, optional)
    n = sum(len(p) for p in pages)
    c = W.EncodedChunk()
    keep = [C.create_string_buffer(body, len(body))]
    c.bytes = C.cast(keep[0], C.c_void_p)
    c.size = c.total_uncompressed_size = len(body)
    c.num_values = n
    c.dictionary_page_offset, c.data_page_offset, c.n_data_pages = -1, 0, len(pages)
    ref = P.ref_index(ptype, [([v for v in p if v is not None], sum(v is None for v in p)) for p in pages], T)
    if bloom:
        keep.append(C.create_string_buffer(bloom, len(bloom)))
        c.bloom, c.bloom_len = C.cast(keep[-1], C.c_void_p), len(bloom)
    if with_index:
        np_ = len(pages)

        def arr(ct, vals):
            a = (ct * max(1, len(vals)))(*vals)
            keep.append(a)
            return C.cast(a, C.POINTER(ct))

        c.index_pages = np_
        c.page_offset = arr(C.c_int64, [l[0] for l in locs])
        c.page_size = arr(C.c_int32, [l[1] for l in locs])
        c.page_first_row = arr(C.c_int64, [l[2] for l in locs])
        c.index_null_pages = arr(C.c_uint8, [int(b) for b in ref["null_pages"]])
        c.index_null_counts = arr(C.c_int64, ref["null_counts"])
        c.column_index = int(ref["valid"])
        if ref["valid"]:
            c.boundary_order = ref["boundary_order"]
            flat = [v for pair in zip(ref["min_values"], ref["max_values"]) for v in pair]
            c.index_value_off = arr(C.c_uint32, list(np.cumsum([0] + [len(v) for v in flat])))
            c.index_values = arr(C.c_uint8, list(b"".join(flat)))
    return c, keep, ref, locs


_FIELDS = ((b"id", K.INT64, 0, 0), (b"price", K.DOUBLE, 1, 0), (b"word", K.BYTE_ARRAY, 0, 1))


def _hand_pages(nan_page=False):
    ids = [list(range(8 * p, 8 * p + 8)) for p in range(3)]
    prices = [[1.5, None, 2.5, 0.0, None, -1.0, 9.0, 3.0], [None] * 8, [float("nan") if nan_page else 7.0] * 8]
    words = [[b"pear", b"apple", b"fig", b"", b"kiwi", b"plum", b"date", b"lime"], [b"zebra" * 30, b"yak"] * 4, [b"w\xc3\xb6rd"] * 8]
    return [ids, prices, words]


def _write(W, path, groups, fields=_FIELDS):
    """groups: [[(chunk, keep, ...)] per field] per row group."""
    fl = (W.WriteField * len(fields))(*[W.WriteField(*f) for f in fields])
    w = C.c_void_p()
    L = W.lib()
    assert L.pf_writer_open(path.encode(), fl, len(fields), C.byref(w)) == 0
    for chunks in groups:
        for i, item in enumerate(chunks):
            assert L.pf_writer_add_chunk(w, i, C.byref(item[0])) == 0, L.pf_writer_last_error()
        assert L.pf_writer_end_row_group(w, chunks[0][0].num_values) == 0
    assert L.pf_writer_close(w) == 0, L.pf_writer_last_error()


def _parsed(path, rg, col):
    from pfloor.decoder import ParquetFile
    with ParquetFile(path) as f:
        return f.page_index(rg, col), f.index_ranges(rg, col)


def _expected_ci(ref):
    return {k: ref[k] for k in ("null_pages", "min_values", "max_values", "boundary_order", "null_counts")}


def test_writer_layout_footer_and_parser(W, tmp_path):
    """Two row groups of three chunks with index fields set, a Bloom filter on two of them: ColumnIndexes, OffsetIndexes,
    Bloom filters, footer, in that order and each in row-group then column order; ColumnChunk fields 4-7 point at them;
    pyarrow opens the file, reads the data and sees the index; pf_file_* return the lists that went in."""
    pq = pytest.importorskip("pyarrow.parquet")
    path = str(tmp_path / "idx.parquet")
    pages = _hand_pages()
    groups = []
    for g in range(2):
        groups.append([_index_chunk(W, f[1], pages[i], bool(f[2]), T=-1 if i < 2 else 8, bloom=bytes(32) if i != 1 else None)
                       for i, f in enumerate(_FIELDS)])
    _write(W, path, groups)
    raw = open(path, "rb").read()
    fm = S.footer(path)
    assert fm[7] == [{1: {}}] * 3                      # column_orders: the index holds min / max
    ccs = [cc for rg in fm[4] for cc in rg[1]]
    end_of_groups = max(cc[3][9] + cc[3][7] for cc in ccs)   # (no dictionary pages)
    ci_off, oi_off = [cc[6] for cc in ccs], [cc[4] for cc in ccs]
    bl = [(cc[3][14], cc[3][15]) for cc in ccs if 14 in cc[3]]
    assert len(bl) == 4
    pos = end_of_groups
    for cc in ccs:                                      # every ColumnIndex, back to back
        assert cc[6] == pos
        pos += cc[7]
    for cc in ccs:                                      # every OffsetIndex
        assert cc[4] == pos
        pos += cc[5]
    for off, ln in bl:                                  # the Bloom filters
        assert off == pos
        pos += ln
    assert pos == len(raw) - 8 - struct.unpack("<I", raw[-8:-4])[0]   # then the footer
    assert ci_off == sorted(ci_off) and oi_off == sorted(oi_off)
    for g in range(2):
        for col in range(3):
            _c, _keep, ref, locs = groups[g][col]
            cc = fm[4][g][1][col]
            ci, oi, _ = _file_index(path, col, g)
            assert {k: P.column_index_fields(ci)[k] for k in ref} == ref
            start = cc[3][9]
            assert [(l[1], l[2], l[3]) for l in oi[1]] == [(start + o, s, r) for o, s, r in locs]
            got, ranges = _parsed(path, g, col)
            assert ranges == ((cc[6], cc[7]), (cc[4], cc[5]))
            assert got["column_index"] == _expected_ci(ref)
            assert got["offset_index"] == [(start + o, s, r) for o, s, r in locs]
    assert groups[0][2][2]["max_values"][1] == b"zebrazec"   # truncated to 8 bytes
    t = pq.read_table(path)
    assert t.column("id").to_pylist() == [v for p in pages[0] for v in p] * 2
    assert t.column("price").to_pylist() == [v for p in pages[1] for v in p] * 2
    assert t.column("word").to_pylist() == [v.decode() for p in pages[2] for v in p] * 2
    md = pq.ParquetFile(path).metadata.row_group(1).column(0)
    assert md.has_offset_index and md.has_column_index
    # a filtered read goes through pyarrow's own use of the statistics; the data survive it
    assert pq.read_table(path, filters=[("id", ">=", 16)]).column("id").to_pylist() == list(range(16, 24)) * 2


def test_writer_offset_index_without_column_index(W, tmp_path):
    """A NaN-only page: no ColumnIndex, fields 6 / 7 absent, the OffsetIndex is there; no column_orders by the index."""
    path = str(tmp_path / "nan.parquet")
    pages = _hand_pages(nan_page=True)
    item = _index_chunk(W, K.DOUBLE, pages[1], True)
    assert item[2]["valid"] is False
    _write(W, path, [[item]], fields=_FIELDS[1:2])
    fm = S.footer(path)
    cc = fm[4][0][1][0]
    assert 6 not in cc and 7 not in cc and 4 in cc and 5 in cc and 7 not in fm
    got, ranges = _parsed(path, 0, 0)
    assert got["column_index"] is None and ranges[0] is None and len(got["offset_index"]) == 3
    from pfloor.decoder import ParquetFile
    from pfloor._native import ColumnIndex, lib
    with ParquetFile(path) as f:
        assert lib().pf_file_column_index(f.h, 0, 0, C.byref(ColumnIndex())) == -9   # PF_ERR_STATE


def test_file_without_index_keeps_its_bytes(W, tmp_path):
    """Chunks with index_pages = 0: whatever the other index fields hold, the file is the one written with all of them
    zero, its ColumnChunks have fields 2 and 3 alone, and the Bloom filter starts where the last row group ends."""
    pages = _hand_pages()
    a, b = str(tmp_path / "a.parquet"), str(tmp_path / "b.parquet")
    plain = [_index_chunk(W, f[1], pages[i], bool(f[2]), with_index=False, bloom=bytes(range(32)) if i == 0 else None)
             for i, f in enumerate(_FIELDS)]
    _write(W, a, [plain])
    junk = [_index_chunk(W, f[1], pages[i], bool(f[2]), bloom=bytes(range(32)) if i == 0 else None) for i, f in enumerate(_FIELDS)]
    for item in junk:
        item[0].index_pages = 0
        item[0].column_index = 0
    _write(W, b, [junk])
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    fm = S.footer(a)
    assert set(fm) == {1, 2, 3, 4, 6}
    ccs = fm[4][0][1]
    assert all(set(cc) == {2, 3} for cc in ccs)
    assert ccs[0][3][14] == ccs[2][3][9] + ccs[2][3][7]
    # the bytes in front of the footer are the three chunks and the filter, nothing else
    body = b"".join(_chunk_bytes(f[1], pages[i], bool(f[2]))[0] for i, f in enumerate(_FIELDS))
    assert raw[4:4 + len(body)] == body and raw[4 + len(body) + ccs[0][3][15]:-8] == raw[-8 - struct.unpack("<I", raw[-8:-4])[0]:-8]
    got, ranges = _parsed(a, 0, 0)
    assert got == {"offset_index": None, "column_index": None} and ranges == (None, None)


def test_writer_rejects_inconsistent_index_fields(W, tmp_path):
    pages = _hand_pages()
    fl = (W.WriteField * 1)(W.WriteField(*_FIELDS[0]))
    L = W.lib()
    w = C.c_void_p()
    assert L.pf_writer_open(str(tmp_path / "r.parquet").encode(), fl, 1, C.byref(w)) == 0
    for spoil in ("page_offset", "page_size", "page_first_row", "index_null_pages", "index_null_counts", "index_values",
                  "index_value_off"):
        c, _keep, _ref, _locs = _index_chunk(W, K.INT64, pages[0], False)
        setattr(c, spoil, None)
        assert L.pf_writer_add_chunk(w, 0, C.byref(c)) == -1, spoil
    for field, v in (("index_pages", -1), ("column_index", 2), ("boundary_order", 3), ("boundary_order", -1)):
        c, _keep, _ref, _locs = _index_chunk(W, K.INT64, pages[0], False)
        setattr(c, field, v)
        assert L.pf_writer_add_chunk(w, 0, C.byref(c)) == -1, (field, v)
    c, _keep, _ref, _locs = _index_chunk(W, K.INT64, pages[0], False)
    c.index_pages = 0                                    # column_index = 1 without pages
    assert L.pf_writer_add_chunk(w, 0, C.byref(c)) == -1
    c, _keep, _ref, _locs = _index_chunk(W, K.INT64, pages[0], False)
    c.page_size[2] = c.size                              # a page that leaves the chunk
    assert L.pf_writer_add_chunk(w, 0, C.byref(c)) == -1
    c, _keep, _ref, _locs = _index_chunk(W, K.INT64, pages[0], False)
    c.index_value_off[3] = 1000                          # offsets out of order
    assert L.pf_writer_add_chunk(w, 0, C.byref(c)) == -1
    c, _keep, _ref, _locs = _index_chunk(W, K.INT64, pages[0], False)
    c.column_index = 0                                   # the OffsetIndex alone needs no values
    c.index_values = c.index_value_off = None
    assert L.pf_writer_add_chunk(w, 0, C.byref(c)) == 0, L.pf_writer_last_error()
    assert L.pf_writer_end_row_group(w, 24) == 0 and L.pf_writer_close(w) == 0


# ---------------------------------------------------------------- 3. the reader on pyarrow's files
_READER_CASES = ("i32_pages_65_random", "s_pages_65_random", "f64_null_page_middle", "b_broken_across_null", "i32_all_null", "f32_nan_only_page", "s_empty", "f64_zeros", "s_no_truncation", "i32_pages_257_alternate_null")


@pytest.mark.parametrize("name", _READER_CASES)
def test_reader_on_pyarrow_files(tmp_path, name):
    """pyarrow's structs carry fields of their own (ColumnIndex 6 / 7, the level histograms; OffsetIndex 2,
    unencoded_byte_array_data_bytes): the parser skips them and returns what read_struct reads, and the page locations
    are where the header walk of pf_file_chunk_desc finds the pages."""
    from pfloor.decoder import ParquetFile
    case = P.cases()[name]
    path = str(tmp_path / "p.parquet")
    _pyarrow_file(case, path)
    ci, oi, cc = _file_index(path)
    if case.optional and ci is not None:
        assert 6 in ci or 7 in ci, "pyarrow no longer writes the histograms: the skip is untested"
    if case.ptype == K.BYTE_ARRAY:
        assert 2 in oi
    with ParquetFile(path) as f:
        got = f.page_index(0, 0)
        d = f.chunk_desc(0, 0, 0)
        start, _size = f.chunk_range(0, 0)
        walk = [(d.pages[i].offset, d.pages[i].compressed_size) for i in range(d.n_pages)]
    if ci is None:
        assert got["column_index"] is None
    else:
        want = P.column_index_fields(ci)
        want.pop("valid")
        assert got["column_index"] == want
    assert got["offset_index"] == [(l[1], l[2], l[3]) for l in oi[1]]
    assert len(walk) == len(got["offset_index"])
    for (body, size), (off, total, _row) in zip(walk, got["offset_index"]):
        assert off + total == start + body + size       # the page ends where the walk's body ends
    assert [o for o, _s, _r in got["offset_index"]][1:] == [o + s for o, s, _r in got["offset_index"]][:-1]
    assert got["offset_index"][0][0] == start


def test_reader_refuses_ranges_outside_the_file(W, tmp_path):
    """An index range that leaves the file is PF_ERR_IO (like pf_file_chunk_bloom); a damaged struct PF_ERR_CORRUPT_PAGE."""
    from pfloor.decoder import ParquetFile
    from pfloor._native import ColumnIndex, PageLocation, lib
    path = str(tmp_path / "ok.parquet")
    pages = _hand_pages()
    _write(W, path, [[_index_chunk(W, K.INT64, pages[0], False)]], fields=_FIELDS[:1])
    raw = bytearray(open(path, "rb").read())
    cc = S.footer(path)[4][0][1][0]
    bad = str(tmp_path / "cut.parquet")
    cut = bytearray(raw)
    cut[cc[6] + 1] = 0x7f                                 # the null_pages list header: 7 elements of type 15
    open(bad, "wb").write(cut)
    with ParquetFile(bad) as f:
        assert lib().pf_file_column_index(f.h, 0, 0, C.byref(ColumnIndex())) == -2
        n = C.c_int()
        assert lib().pf_file_offset_index(f.h, 0, 0, None, 0, C.byref(n)) == -6 and n.value == 3   # PF_ERR_CAPACITY, the count
        locs = (PageLocation * 3)()
        assert lib().pf_file_offset_index(f.h, 0, 0, locs, 3, C.byref(n)) == 0
    # the same file with the footer's offset_index_offset pushed past the end: rewrite the i64 in place
    n_foot = struct.unpack("<I", raw[-8:-4])[0]
    foot = bytes(raw[-8 - n_foot:-8])
    old = bytes([0x16]) + S.w_zz(cc[4])                   # field 4 behind field 3: delta 1, i64
    assert foot.count(old) == 1
    new = bytes([0x16]) + S.w_zz(len(raw) * 2)
    foot2 = foot.replace(old, new)
    far = str(tmp_path / "far.parquet")
    open(far, "wb").write(bytes(raw[:-8 - n_foot]) + foot2 + struct.pack("<I", len(foot2)) + b"PAR1")
    with ParquetFile(far) as f:
        co, oo, cl, ol = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        assert lib().pf_file_chunk_index_ranges(f.h, 0, 0, C.byref(co), C.byref(cl), C.byref(oo), C.byref(ol)) == -8


# ---------------------------------------------------------------- 4. the parser under the sanitizers
def test_parser_under_asan(W, tmp_path):
    """Valid structs of ours and of pyarrow, every prefix of them and every single-byte change, through
    parse_column_index / parse_offset_index built with -fsanitize=address,undefined, as a program of its own."""
    structs = []
    path = str(tmp_path / "ours.parquet")
    pages = _hand_pages()
    _write(W, path, [[_index_chunk(W, f[1], pages[i], bool(f[2]), T=-1 if i < 2 else 8) for i, f in enumerate(_FIELDS)]])
    raw = open(path, "rb").read()
    for cc in S.footer(path)[4][0][1]:
        structs += [(0, raw[cc[6]:cc[6] + cc[7]]), (1, raw[cc[4]:cc[4] + cc[5]])]
    try:
        import pyarrow  # noqa: F401
        for name in ("s_empty", "f64_null_page_middle"):
            p2 = str(tmp_path / (name + ".parquet"))
            _pyarrow_file(P.cases()[name], p2)
            r2 = open(p2, "rb").read()
            cc = S.footer(p2)[4][0][1][0]
            structs += [(0, r2[cc[6]:cc[6] + cc[7]]), (1, r2[cc[4]:cc[4] + cc[5]])]
    except ImportError:
        pass
    structs.append((0, b"\x19\x01\x19\x08\x19\x08\x15\x00\x00"))   # no pages at all
    structs.append((1, b"\x19\x0c\x00"))
    cases = str(tmp_path / "structs.bin")
    with open(cases, "wb") as f:
        for kind, s in structs:
            assert len(s) < 700, len(s)
            f.write(struct.pack("<II", kind, len(s)) + s)
    exe = str(tmp_path / "pf_pgindex_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "pf_pgindex_check.cpp"), os.path.join(CSRC, "pf_meta.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([exe, cases], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    m = re.search(r"valid (\d+) accepted (\d+) refused (\d+) failures 0", r.stdout)
    assert m and int(m.group(1)) == len(structs) and int(m.group(3)) > int(m.group(1)), r.stdout
