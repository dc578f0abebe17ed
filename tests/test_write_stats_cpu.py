"""Statistics and page CRCs of the write path, host side (no GPU): the reference of the GPU tests pinned to
pyarrow's writer, the header and footer writers on hand-built chunks, and the host fold of CRC pieces."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import pagekit as K
import stats_cases as S
from conftest import ROOT

CSRC = os.path.join(ROOT, "parquet-floor_amd", "csrc")
_FMT = {K.INT32: "<i", K.INT64: "<q", K.FLOAT: "<f", K.DOUBLE: "<d"}


@pytest.fixture(scope="module")
def W():
    from pfloor import writer
    writer.lib()
    return writer


def test_tile_size_is_the_kernels():
    """The page sizes of the GPU cases sit around ST_TILE and the size limit is ST_LIMIT."""
    src = open(os.path.join(CSRC, "pf_enc_tables.h")).read()
    assert int(re.search(r"ST_TILE = (\d+);", src).group(1)) == S.TILE
    assert int(re.search(r"ST_LIMIT = (\d+);", src).group(1)) == S.LIMIT
    hdr = open(os.path.join(ROOT, "include", "pfloor.h")).read()
    from pfloor import writer as Wr
    for name, v in (("PF_ENCODE_STATISTICS", Wr.ENCODE_STATISTICS), ("PF_ENCODE_PAGE_CRC", Wr.ENCODE_PAGE_CRC),
                    ("PF_STATS_NULL_COUNT", Wr.STATS_NULL_COUNT), ("PF_STATS_MIN_MAX", Wr.STATS_MIN_MAX)):
        assert int(re.search(rf"#define {name}\s+(\d+)", hdr).group(1)) == v, name
    assert (Wr.ENCODE_STATISTICS, Wr.ENCODE_PAGE_CRC) == (8, 16)


# ---------------------------------------------------------------- 1. the reference against pyarrow's writer
def _plain(ptype, v):
    if v is None:
        return None
    if ptype == K.BYTE_ARRAY:
        return v
    if ptype == K.BOOLEAN:
        return b"\x01" if v else b"\x00"
    return struct.pack(_FMT[ptype], v)


@pytest.mark.parametrize("fid", S.STAT_FILE_IDS)
def test_reference_is_what_pyarrow_writes(tmp_path, fid):
    """pyarrow writes every numeric, boolean and short-string case (v2 data pages); its chunk statistics are the
    reference's: has_min_max, min and max as PLAIN bytes (so the sign of a zero counts), null_count. The long
    values are left out: pyarrow's size limit is per value."""
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    for rows, cases in S.file_groups(fid):
        cases = [c for c in cases if not c.name.startswith("long_")]
        path = str(tmp_path / f"{fid}_{rows}.parquet")
        pq.write_table(pa.table({c.name: c.arrow() for c in cases}), path, data_page_version="2.0", compression="NONE",
                       row_group_size=rows, use_dictionary=False)
        md = pq.ParquetFile(path).metadata
        assert md.num_row_groups == 1
        for col, case in enumerate(cases):
            st = md.row_group(0).column(col).statistics
            _pages, ref = case.page_refs()
            assert st is not None and st.has_null_count and st.null_count == ref["null_count"], case.name
            assert st.has_min_max == (ref["min"] is not None), case.name
            if st.has_min_max:
                assert (_plain(case.ptype, st.min), _plain(case.ptype, st.max)) == (ref["min"], ref["max"]), case.name


def test_reference_rules():
    """The rules that pyarrow cannot pin: the size limit, the legacy fields, the ordering chain."""
    chain = [b"", b"a", b"a\x00", b"b", b"\xc3\xa9", b"\xff"]
    for i in range(len(chain) - 1):
        r = S.ref_stats(K.BYTE_ARRAY, [chain[i + 1], chain[i]], 0)
        assert (r["min"], r["max"], r["legacy"]) == (chain[i], chain[i + 1], False)
    assert S.ref_stats(K.BYTE_ARRAY, [b"a" * 2047, b"z" * 2047], 3)["null_count"] == 3
    assert S.ref_stats(K.BYTE_ARRAY, [b"a" * 2048, b"z" * 2048], 3) is None
    assert S.expected_fields(S.ref_stats(K.BYTE_ARRAY, [b"q", b"q"], 1)) == {1: b"q", 2: b"q", 3: 1, 5: b"q", 6: b"q"}
    assert S.expected_fields(S.ref_stats(K.BYTE_ARRAY, [b"p", b"q"], 1)) == {3: 1, 5: b"q", 6: b"p"}
    assert S.expected_fields(S.ref_stats(K.DOUBLE, [float("nan")], 2)) == {3: 2}
    z = S.ref_stats(K.FLOAT, [0.0, float("nan")], 0)
    assert (z["min"], z["max"]) == (struct.pack("<f", -0.0), struct.pack("<f", 0.0))
    assert S.expected_fields(S.ref_stats(K.INT32, [-1, 0], 0)) == {1: b"\0\0\0\0", 2: b"\xff\xff\xff\xff", 3: 0,
                                                                    5: b"\0\0\0\0", 6: b"\xff\xff\xff\xff"}


# ---------------------------------------------------------------- 2. header and footer writers alone
def _chunk(W, body, n, stats=None, nulls=0):
    c = W.EncodedChunk()
    keep = [C.create_string_buffer(body, len(body))]
    c.bytes = C.cast(keep[0], C.c_void_p)
    c.size = c.total_uncompressed_size = len(body)
    c.num_values = n
    c.dictionary_page_offset = -1
    c.data_page_offset = 0
    c.n_data_pages = 1
    if stats is not None:
        lo, hi = stats
        keep += [C.create_string_buffer(lo, max(1, len(lo))), C.create_string_buffer(hi, max(1, len(hi)))]
        c.stats_flags = W.STATS_NULL_COUNT | W.STATS_MIN_MAX
        c.stat_min_len, c.stat_max_len, c.null_count = len(lo), len(hi), nulls
        c.stat_min, c.stat_max = C.cast(keep[1], C.c_void_p), C.cast(keep[2], C.c_void_p)
    return c, keep


def _hand_built(with_stats, with_crc):
    """Three chunks of 1,000 rows, one uncompressed v2 PLAIN page each: INT64, OPTIONAL DOUBLE, UTF8 BYTE_ARRAY."""
    n = 1000
    ids = np.arange(n, dtype=np.int64) * 3 - 700
    present = (np.arange(n) % 4) != 0
    prices = (np.arange(n) * 0.25 - 10.0)[present]
    groups = (n + 7) // 8
    defl = S.w_uvarint((groups << 1) | 1) + np.packbits(present, bitorder="little").tobytes()
    words = [f"wörd{k % 37:02d}".encode() for k in range(n)]
    pages = [(b"", ids.tobytes(), 0, (struct.pack("<q", int(ids.min())), struct.pack("<q", int(ids.max())))),
             (defl, prices.tobytes(), int((~present).sum()), (struct.pack("<d", prices.min()), struct.pack("<d", prices.max()))),
             (b"", b"".join(struct.pack("<I", len(w)) + w for w in words), 0, (min(words), max(words)))]
    out = []
    for k, (lv, vals, nulls, (lo, hi)) in enumerate(pages):
        st = {3: nulls, 5: hi, 6: lo}
        if k < 2:
            st[1], st[2] = hi, lo
        hdr = S.w_page_header_v2(n, nulls, 0, len(lv), len(vals), crc=zlib.crc32(lv + vals) if with_crc else None,
                                 stats=st if with_stats else None)
        out.append((hdr + lv + vals, nulls, (lo, hi)))
    return n, ids, present, prices, words, out


def _write(W, path, n, chunks):
    fields = (W.WriteField * 3)(W.WriteField(b"id", W.INT64, 0, 0), W.WriteField(b"price", W.DOUBLE, 1, 0),
                                W.WriteField(b"word", W.BINARY, 0, 1))
    w = C.c_void_p()
    L = W.lib()
    assert L.pf_writer_open(path.encode(), fields, 3, C.byref(w)) == 0
    for i, (c, _keep) in enumerate(chunks):
        assert L.pf_writer_add_chunk(w, i, C.byref(c)) == 0, L.pf_writer_last_error()
    assert L.pf_writer_end_row_group(w, n) == 0
    assert L.pf_writer_close(w) == 0


def test_writer_statistics_and_crc_read_by_pyarrow_and_oracle(W, oracle, tmp_path):
    pq = pytest.importorskip("pyarrow.parquet")
    n, ids, present, prices, words, built = _hand_built(True, True)
    path = str(tmp_path / "s.parquet")
    _write(W, path, n, [_chunk(W, body, n, stats, nulls) for body, nulls, stats in built])
    md = pq.ParquetFile(path).metadata.row_group(0)
    st = [md.column(c).statistics for c in range(3)]
    assert all(s is not None and s.has_min_max for s in st)
    assert (st[0].min, st[0].max, st[0].null_count) == (int(ids.min()), int(ids.max()), 0)
    assert (st[1].min, st[1].max, st[1].null_count) == (prices.min(), prices.max(), int((~present).sum()))
    assert (st[2].min, st[2].max, st[2].null_count) == (min(words).decode(), max(words).decode(), 0)
    fm = S.footer(path)
    assert fm[7] == [{1: {}}] * 3
    assert set(fm[4][0][1][0][3][12]) == {1, 2, 3, 5, 6} and set(fm[4][0][1][2][3][12]) == {3, 5, 6}   # legacy: not for BYTE_ARRAY
    for col in range(3):
        (p,) = S.page_headers(path, col)
        assert p["stats"] == ({1: built[col][2][1], 2: built[col][2][0]} if col < 2 else {}) | \
            {3: built[col][1], 5: built[col][2][1], 6: built[col][2][0]}
    t = pq.read_table(path, page_checksum_verification=True)
    assert np.array_equal(t.column("id").to_numpy(), ids)
    assert t.column("word").to_pylist() == [w.decode() for w in words]
    assert [v for v in t.column("price").to_pylist() if v is not None] == prices.tolist()
    with oracle.open(path) as of:
        for col in range(3):
            cnt, err, pages = of.chunk_pages(0, col, verify_crc=True)
            assert (cnt, err) == (1, -1) and pages[0]["has_crc"] and pages[0]["crc_ok"]
    raw = bytearray(open(path, "rb").read())
    (p,) = S.page_headers(path, 1)
    raw[p["body"] + p["compressed"] // 2] ^= 1
    bad = str(tmp_path / "bad.parquet")
    open(bad, "wb").write(raw)
    with pytest.raises(OSError, match="(?i)crc|checksum"):
        pq.read_table(bad, page_checksum_verification=True)
    with oracle.open(bad) as of:
        cnt, err, _pages = of.chunk_pages(0, 1, verify_crc=True)
        assert cnt < 0 and err == 0
        assert of.chunk_pages(0, 0, verify_crc=True)[0] == 1


def test_writer_without_statistics_keeps_its_footer(W, tmp_path):
    """Chunks that carry no statistics: no FileMetaData field 7, no ColumnMetaData field 12, and whatever the other
    new fields hold, the file is the one written with all of them zero."""
    n, _ids, _present, _prices, _words, built = _hand_built(False, False)
    a, b = str(tmp_path / "a.parquet"), str(tmp_path / "b.parquet")
    _write(W, a, n, [_chunk(W, body, n) for body, _nulls, _stats in built])
    junk = []
    for body, _nulls, (lo, hi) in built:
        c, keep = _chunk(W, body, n, (lo, hi), 77)
        c.stats_flags = 0
        junk.append((c, keep))
    _write(W, b, n, junk)
    assert open(a, "rb").read() == open(b, "rb").read()
    fm = S.footer(a)
    assert 7 not in fm and set(fm) == {1, 2, 3, 4, 6}
    assert all(12 not in cc[3] for cc in fm[4][0][1])
    for col in range(3):
        (p,) = S.page_headers(a, col)
        assert p["crc"] is None and p["stats"] is None


def test_writer_rejects_flagged_min_max_without_bytes(W, tmp_path):
    n, _ids, _present, _prices, _words, built = _hand_built(False, False)
    body, _nulls, (lo, hi) = built[0]
    fields = (W.WriteField * 1)(W.WriteField(b"id", W.INT64, 0, 0))
    L = W.lib()
    w = C.c_void_p()
    assert L.pf_writer_open(str(tmp_path / "r.parquet").encode(), fields, 1, C.byref(w)) == 0
    for spoil in ("min", "max", "min_len", "max_len"):
        c, _keep = _chunk(W, body, n, (lo, hi))
        if spoil in ("min", "max"):
            setattr(c, "stat_" + spoil, None)
        else:
            setattr(c, "stat_" + spoil, -1)
        assert L.pf_writer_add_chunk(w, 0, C.byref(c)) == -1, spoil
    c, _keep = _chunk(W, body, n)
    c.stats_flags = W.STATS_NULL_COUNT        # null_count alone needs no bytes
    assert L.pf_writer_add_chunk(w, 0, C.byref(c)) == 0
    assert L.pf_writer_end_row_group(w, n) == 0 and L.pf_writer_close(w) == 0
    assert S.footer(str(tmp_path / "r.parquet"))[4][0][1][0][3][12] == {3: 0}


# ---------------------------------------------------------------- 3. the host fold of CRC pieces
def test_crc_combine_under_asan(tmp_path):
    exe = str(tmp_path / "pf_crc_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "pf_crc_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "failures 0" in r.stdout
