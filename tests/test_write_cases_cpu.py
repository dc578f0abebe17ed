"""The default write route's reference (tests/write_cases.py), host side (no GPU).

The expected bytes of test_gpu_write_bytes.py are stated in write_cases.Case.plan from a case's inputs alone. Here
every case's reference pages are wrapped in a file by pagekit (its own page headers and footer) and read back to
the inputs by the CPU oracle and by pyarrow: two readers that share no code with the reference. The page-header
reader the GPU test walks chunks with is checked against pagekit's header writer, and the packing against bytes
worked out by hand."""
import numpy as np
import pytest

import pagekit as K
import write_cases as WC
from golden_util import assert_chunk_equal


@pytest.mark.parametrize("fid", WC.FILE_IDS)
def test_reference_pages_read_by_oracle_and_pyarrow(oracle, tmp_path, fid):
    pq = pytest.importorskip("pyarrow.parquet")
    rows, cases = WC.file_cases(fid)
    chunks = [WC.reference_chunk(case) for case in cases]
    data, _info = K.build_file(chunks, rows)
    path = str(tmp_path / f"{fid}.parquet")
    with open(path, "wb") as f:
        f.write(data)
    with oracle.open(path) as of:
        assert of.num_columns == len(cases)
        for c, case in enumerate(cases):
            o = of.decode(0, c)
            assert o["status"] == 0, (fid, case.name, o["error"])
            assert_chunk_equal(o, case.expected(), f"{fid} {case.name} [oracle]")
    if rows == 0:
        return
    t = pq.ParquetFile(path).read_row_group(0)
    assert t.num_rows == rows
    for case in cases:
        case.check_arrow(t.column(case.name), f"{fid} {case.name} [pyarrow]")


def test_page_reader_against_pagekit_headers():
    """read_pages finds in a pagekit chunk the fields pagekit's header writer was given."""
    _rows, cases = WC.file_cases("r3003")
    for case in cases[:12]:
        ch, p = WC.reference_chunk(case), case.plan()
        pages = WC.read_pages(ch.dict + b"".join(ch.pages))
        if p["dict"] is not None:
            d = pages.pop(0)
            assert (d["type"], d["num_values"], d["encoding"], d["body"]) == (WC.PAGE_DICTIONARY, len(p["dict"]), K.PLAIN, p["dict_bytes"])
        assert len(pages) == len(p["pages"]) == 4
        for got, pg in zip(pages, p["pages"]):
            assert (got["type"], got["num_values"], got["num_nulls"], got["num_rows"], got["encoding"], got["def_bytes"], got["rep_bytes"]) == \
                (WC.PAGE_DATA_V2, pg["rows"], pg["nulls"], pg["rows"], p["encoding"], len(pg["levels"]), 0)
            assert got["usize"] == got["csize"] == len(got["body"]) and got["body"] == pg["levels"] + pg["values"]
    hdr = K._T().i32(1, 3).i32(2, 70000).i32(3, -1 & 0x7fffffff).i32(4, -5).begin(8).i32(1, 9).i32(2, 1).i32(3, 9).i32(4, 8) \
        .i32(5, 300).i32(6, 0).boolean(7, False).begin(8).string(5, b"\x00\x01").i64(3, 1 << 40).end().end().done()
    h, end = WC._struct(hdr, 0)
    assert end == len(hdr) and (h[1], h[2], h[3], h[4]) == (3, 70000, 0x7fffffff, -5)
    assert h[8][7] is False and h[8][5] == 300 and h[8][8] == {5: b"\x00\x01", 3: 1 << 40}


def test_reference_by_hand():
    assert [WC.id_width(d) for d in (1, 2, 3, 4, 5, 8, 9, 256, 257, 65536, 65537, (1 << 19) + 1)] == [1, 1, 2, 2, 3, 3, 4, 8, 9, 16, 17, 20]
    # three ids at width 2: one group, 1 | 2 << 2 | 3 << 4 = 0x39, zero padding
    assert WC.packed_ids([1, 2, 3], 2) == bytes([0x03, 0x39, 0x00])
    # nine ids at width 9 straddle bytes and a 64-bit word: bits of id k at [9 k, 9 k + 9)
    ids = [0x1ff, 0, 0x155, 1, 0x100, 0xff, 2, 0x1fe, 0x1ff]
    acc = sum(v << (9 * k) for k, v in enumerate(ids))
    assert WC.packed_ids(ids, 9) == bytes([0x05]) + acc.to_bytes(18, "little")
    # 7, 3, 7 (null) 9: dictionary 7 3 9 in first-occurrence order, ids 0 1 2, the null's garbage nowhere
    c = WC.Case("h", K.INT32, [7, 3, 9], present=[True, True, False, True])
    p = c.plan()
    assert p["dict_bytes"] == np.array([7, 3, 9], "<i4").tobytes() and p["bw"] == 2 and p["fallback"] == 0
    assert p["pages"] == [{"rows": 4, "nulls": 1, "levels": bytes([0x03, 0x0b]), "values": bytes([2, 0x03, 0x24, 0x00]), "d0": 0, "cnt": 3}]
    data, validity = c.row_arrays()
    assert data[2] not in (7, 3, 9) and validity.tolist() == [0x0b]
    # raw-bit identity: +0.0 / -0.0 and two NaN payloads are four entries
    f = np.array([0, 0x80000000, 0x7fc00001, 0x7fc00002, 0, 0x7fc00001], np.uint32).view(np.float32)
    p = WC.Case("f", K.FLOAT, f).plan()
    assert p["dict_bytes"] == f[:4].tobytes() and p["pages"][0]["values"] == bytes([2, 0x03]) + (0 | 1 << 2 | 2 << 4 | 3 << 6 | 0 << 8 | 2 << 10).to_bytes(2, "little")
    # BOOLEAN: never a dictionary; PLAIN bits LSB-first; an all-null page is no value bytes
    p = WC.Case("b", K.BOOLEAN, [1, 0, 1], present=[True, True, True] + [False] * 8, page_rows=8).plan()
    assert (p["fallback"], p["encoding"]) == (3, K.PLAIN)
    assert [(g["levels"], g["values"]) for g in p["pages"]] == [(bytes([0x03, 0x07]), bytes([0x05])), (bytes([0x03, 0x00]), b"")]
    # a dictionary page with no present value in a page: the width byte alone
    p = WC.Case("n", K.INT64, [5, 6], present=[True, True] + [False] * 14, page_rows=8).plan()
    assert [g["values"] for g in p["pages"]] == [bytes([1, 0x03, 0x02]), bytes([1])]
    # page_rows rounds up to a multiple of 8
    assert [g["rows"] for g in WC.Case("r", K.INT32, np.arange(2500), page_rows=1001).plan()["pages"]] == [1008, 1008, 484]
    # limits count D * w and the sum of 4 + len
    assert WC.Case("l", K.INT64, [1, 2, 1], dict_page_limit=16).plan()["fallback"] == 0
    assert WC.Case("l", K.INT64, [1, 2, 1], dict_page_limit=15).plan()["fallback"] == 1
    assert WC.Case("l", K.BYTE_ARRAY, [b"ab", b"", b"ab"], dict_page_limit=10).plan()["fallback"] == 0
    assert WC.Case("l", K.BYTE_ARRAY, [b"ab", b"", b"ab"], dict_page_limit=9).plan()["fallback"] == 1


@pytest.mark.parametrize("fid", WC.FILE_IDS)
def test_rows_under_nulls_hold_garbage(fid):
    """The encoder's inputs: present rows hold the case's values, null rows values that differ from row to row and
    occur nowhere among the present ones (BOOLEAN apart), and the validity bits are the mask."""
    rows, cases = WC.file_cases(fid)
    for case in cases:
        data, validity = case.row_arrays()
        mask = case.mask()
        assert (validity is None) == (not case.optional or not case.send_validity), case.name
        if validity is not None:
            assert np.array_equal(np.unpackbits(validity, bitorder="little")[:rows].astype(bool), mask), case.name
        if case.ptype == K.BYTE_ARRAY:
            offsets, chars = data
            vals = [chars[offsets[r]:offsets[r + 1]].tobytes() for r in range(rows)]
            assert [v for v, p in zip(vals, mask) if p] == case.dense, case.name
            under = [v for v, p in zip(vals, mask) if not p]
            assert all(under) and len(set(under)) == len(under) and not set(under) & set(case.dense), case.name
            continue
        assert data.dtype == WC._DTYPE[case.ptype] and len(data) == rows, case.name
        bits = data.view(WC._BITS[case.ptype])
        assert np.array_equal(bits[mask], case.keys()), case.name
        if case.ptype != K.BOOLEAN:
            under = bits[~mask]
            assert len(np.unique(under)) == len(under) and not np.isin(under, case.keys()).any(), case.name


def test_cases_cover_what_they_claim():
    """The width sweep reaches every width 1..20 with pages that end inside a group, and garbage sits under every null."""
    widths, partial = set(), 0
    for d in WC.SWEEP_D:
        case = WC._sweep_case(d) if d <= 1025 else None
        widths.add(WC.id_width(d))
        if case is not None:
            p = case.plan()
            assert len(p["dict"]) == d and p["bw"] == WC.id_width(d)
            partial += sum(1 for g in p["pages"] if g["cnt"] % 8)
    assert widths == set(range(1, 21)) and partial > 50
