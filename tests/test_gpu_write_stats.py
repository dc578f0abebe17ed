"""Page / chunk statistics and page CRCs written on the GPU (PF_ENCODE_STATISTICS, PF_ENCODE_PAGE_CRC).

Every page's Statistics struct and every chunk's are compared field by field with stats_cases.ref_stats, which
states the rules from the present values alone (test_write_stats_cpu.py pins it to pyarrow's writer); every
PageHeader.crc with zlib.crc32 of the stored page bytes, and with three verifiers: pf_scan_pages, the CPU oracle
and pyarrow. The files of a test id (one per row count of its cases, tests/stats_cases.py) are written once per
route and codec and shared."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import pagekit as K
import stats_cases as S
from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

PAGE_DICTIONARY, PAGE_DATA_V2 = 2, 3
CODECS = pytest.mark.parametrize("codec", [K.SNAPPY, K.UNCOMPRESSED], ids=["snappy", "uncompressed"])


@pytest.fixture(scope="module")
def dec():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _encode(dec, case, codec, **kw):
    """pf_encode_chunk of one case -> (chunk bytes, EncodedChunk copy, its statistics())."""
    from pfloor import writer as W
    data, validity = case.row_arrays()
    out = W.GpuColumnEncoder(dec).encode(W.Field(case.name, case.ptype, case.optional), data, validity, case.rows,
                                         page_rows=case.page_rows, codec=codec, **kw)
    return C.string_at(out.bytes, out.size), W.EncodedChunk.from_buffer_copy(out), out.statistics()


def _write(dec, path, rows, cases, codec, **kw):
    """The cases as one row group -> [(data_encoding, fallback, statistics())] per chunk."""
    from pfloor import writer as W
    L = W.lib()
    names = [c.name.encode() for c in cases]
    fields = (W.WriteField * len(cases))(*[W.WriteField(names[i], c.ptype, int(c.optional), 0) for i, c in enumerate(cases)])
    w = C.c_void_p()
    assert L.pf_writer_open(path.encode(), fields, len(cases), C.byref(w)) == 0
    chunks = []
    enc = W.GpuColumnEncoder(dec)
    for i, case in enumerate(cases):
        data, validity = case.row_arrays()
        out = enc.encode(W.Field(case.name, case.ptype, case.optional), data, validity, rows,
                         page_rows=case.page_rows, codec=codec, **kw)
        chunks.append((out.data_encoding, out.fallback, out.statistics()))
        assert L.pf_writer_add_chunk(w, i, C.byref(out)) == 0, L.pf_writer_last_error()
    assert L.pf_writer_end_row_group(w, rows) == 0
    assert L.pf_writer_close(w) == 0
    return chunks


@pytest.fixture(scope="module")
def written(dec, tmp_path_factory):
    """written(fid, route, codec, statistics=True, page_checksums=True) -> [(path, cases, chunks)], each once."""
    root = tmp_path_factory.mktemp("stats")
    cache = {}

    def get(fid, route, codec, statistics=True, page_checksums=True):
        key = (fid, route, codec, statistics, page_checksums)
        if key not in cache:
            files = []
            for rows, cases in S.file_groups(fid):
                path = str(root / f"{fid}_{rows}_{route}_{codec}_{int(statistics)}{int(page_checksums)}.parquet")
                chunks = _write(dec, path, rows, cases, codec, statistics=statistics, page_checksums=page_checksums,
                                **S.ROUTES[route])
                files.append((path, cases, chunks))
            cache[key] = files
        return cache[key]
    return get


def _stored(path, page):
    with open(path, "rb") as f:
        f.seek(page["body"])
        return f.read(page["compressed"])


def _check_zlib(path, n_cols, label):
    """PageHeader.crc of every page = zlib.crc32 of the compressed_page_size bytes after the header."""
    n = 0
    for col in range(n_cols):
        for p in S.page_headers(path, col):
            assert p["crc"] is not None, f"{label} col {col} page {p['page']}: no crc"
            assert p["crc"] == zlib.crc32(_stored(path, p)), f"{label} col {col} page {p['page']} ({p['compressed']} bytes)"
            n += 1
    return n


def _check_statistics(path, cases, chunks, label):
    fm = S.footer(path)
    assert len(fm[7]) == len(cases) and all(o == {1: {}} for o in fm[7]), f"{label}: column_orders"
    for col, case in enumerate(cases):
        page_refs, chunk_ref = case.page_refs()
        pages = [p for p in S.page_headers(path, col) if p["type"] == PAGE_DATA_V2]
        assert len(pages) == len(page_refs), f"{label} {case.name}"
        for k, (p, ref) in enumerate(zip(pages, page_refs)):
            assert p["stats"] == S.expected_fields(ref), f"{label} {case.name} page {k}: {p['stats']} for {S.expected_fields(ref)}"
            if ref is not None:
                assert p["stats"][3] == p["v2"][2], f"{label} {case.name} page {k}: null_count is not num_nulls"
        md = fm[4][0][1][col][3]
        assert md.get(12) == S.expected_fields(chunk_ref), f"{label} {case.name} chunk: {md.get(12)}"
        nulls, lo, hi = chunks[col][2]
        if chunk_ref is None:
            assert (nulls, lo, hi) == (None, None, None), f"{label} {case.name}"
        else:
            assert (nulls, lo, hi) == (chunk_ref["null_count"], chunk_ref["min"], chunk_ref["max"]), f"{label} {case.name}"


# ---------------------------------------------------------------- 1. statistics
@pytest.mark.parametrize("route", list(S.ROUTES))
@pytest.mark.parametrize("fid", S.STAT_FILE_IDS)
def test_statistics(written, fid, route):
    """Every page's and every chunk's Statistics are the reference's, field for field, whatever the encoding."""
    seen = set()
    for path, cases, chunks in written(fid, route, K.SNAPPY):
        _check_statistics(path, cases, chunks, f"{fid} {route}")
        _check_zlib(path, len(cases), f"{fid} {route}")
        seen |= {c[0] for c in chunks}
    want = {"dictionary": {K.RLE_DICTIONARY}, "plain_fallback": {K.PLAIN}, "hybrid_runs": {K.RLE_DICTIONARY, K.RLE},
            "delta_fallback": {K.DELTA_BINARY_PACKED, K.DELTA_BYTE_ARRAY, K.PLAIN}, "all_bits": {K.RLE_DICTIONARY, K.RLE}}[route]
    if fid == "bools":                        # BOOLEAN has no dictionary and no DELTA_* encoding
        want = {K.RLE} if route in ("hybrid_runs", "all_bits") else {K.PLAIN}
    assert seen & want, (fid, route, seen)    # the route was taken
    if route == "plain_fallback":
        assert seen == {K.PLAIN}


def test_size_limit_drops_the_struct(written):
    """min and max of 2,047 bytes each: statistics; of 2,048 each: none on that page and on the chunk, while the
    other pages and the neighbouring chunks keep theirs."""
    for path, cases, _chunks in written("strings", "plain_fallback", K.SNAPPY):
        fm = S.footer(path)
        for col, case in enumerate(cases):
            pages = [p for p in S.page_headers(path, col) if p["type"] == PAGE_DATA_V2]
            md = fm[4][0][1][col][3]
            if case.name.startswith("long_2048"):
                assert pages[0]["stats"] is None and 12 not in md
                assert all(p["stats"] is not None and 5 in p["stats"] for p in pages[1:])
            else:
                assert all(p["stats"] is not None for p in pages) and 12 in md
            if case.name.startswith("long_2047"):
                assert len(pages[0]["stats"][5]) == len(pages[0]["stats"][6]) == 2047 and len(md[12][5]) == 2047
                assert 1 not in pages[0]["stats"]


# ---------------------------------------------------------------- 2. CRC
def _verify_three(dec, oracle, path, n_cols, label):
    """pf_scan_pages(verify_crc=1), the oracle and pyarrow accept every page; -> pages verified."""
    pq = pytest.importorskip("pyarrow.parquet")
    from pfloor.decoder import ParquetFile
    with open(path, "rb") as f:
        data = f.read()
    with ParquetFile(path) as pf:
        rows = pf.row_group_rows(0)
        ranges = [pf.chunk_range(0, col) for col in range(n_cols)]
    n_pages = [len(S.page_headers(path, col)) for col in range(n_cols)]
    rc, res = dec.scan_pages(data, [(s, n, rows) for s, n in ranges], verify_crc=True)
    assert rc == 0, label
    for col, (status, err_page, crc_pages, pages) in enumerate(res):
        assert (status, err_page) == (0, -1), f"{label} col {col}"
        assert crc_pages == len(pages) == n_pages[col], f"{label} col {col}: {crc_pages} of {n_pages[col]} pages verified"
    with oracle.open(path) as of:
        for col in range(n_cols):
            n, err, pages = of.chunk_pages(0, col, verify_crc=True)
            assert (n, err) == (n_pages[col], -1), f"{label} col {col} [oracle]"
            assert all(p["has_crc"] and p["crc_ok"] for p in pages), f"{label} col {col} [oracle]"
    assert pq.read_table(path, page_checksum_verification=True).num_rows == rows, label
    return sum(n_pages)


@CODECS
@pytest.mark.parametrize("route", ["dictionary", "all_bits"])
@pytest.mark.parametrize("fid", S.STAT_FILE_IDS)
def test_crc(dec, oracle, written, fid, route, codec):
    """Every page header's crc is zlib's CRC-32 of the stored page, and three verifiers accept the file."""
    for path, cases, _chunks in written(fid, route, codec):
        label = f"{fid} {route} codec {codec}"
        assert _check_zlib(path, len(cases), label) == _verify_three(dec, oracle, path, len(cases), label)


@CODECS
@pytest.mark.parametrize("route", ["plain", "plain_hybrid", "dictionary", "delta"])
def test_crc_at_job_boundaries(dec, oracle, tmp_path, route, codec):
    """Values sections of exactly 0, 1, 8,191, 8,192, 8,193 and 16,385 bytes (the compressor's job boundaries):
    OPTIONAL columns with levels from the host and (hybrid runs) from the device, dictionary pages of those
    sizes, DELTA_BYTE_ARRAY pages."""
    kw = {"plain": dict(dictionary=False), "plain_hybrid": dict(dictionary=False, hybrid_runs=True),
          "dictionary": dict(dictionary=True, dict_page_limit=1 << 20), "delta": dict(dictionary=False, delta_fallback=True)}[route]
    (rows, cases), = S.file_groups("sizes")
    path = str(tmp_path / "sizes.parquet")
    chunks = _write(dec, path, rows, cases, codec, statistics=True, page_checksums=True, **kw)
    label = f"sizes {route} codec {codec}"
    assert _check_zlib(path, len(cases), label) == _verify_three(dec, oracle, path, len(cases), label)
    _check_statistics(path, cases, chunks, label)
    sizes = {p["uncompressed"] - (p["v2"][5] if p["v2"] else 0) for col in range(len(cases)) for p in S.page_headers(path, col)}
    if route == "plain":
        assert {0, 1, 8191, 8192, 8193, 16385} <= sizes, sizes
        assert chunks[0][0] == K.PLAIN
    if route == "dictionary":
        dict_sizes = {p["uncompressed"] for col in range(len(cases)) for p in S.page_headers(path, col) if p["type"] == PAGE_DICTIONARY}
        assert {8191, 8192, 8193, 16385} <= dict_sizes and 1 in sizes, (dict_sizes, sizes)
    if route == "delta":
        assert chunks[0][0] == K.DELTA_BYTE_ARRAY
    from pfloor.decoder import decode_file
    got = decode_file(path, decoder=dec)
    assert got["_status"] == 0, got["_error"]
    for col, case in enumerate(cases):
        assert_chunk_equal(got[(0, col)], case.expected(), f"{label} {case.name} [GPU reader]")


@CODECS
def test_flipped_byte_is_found_at_its_page(dec, oracle, written, tmp_path, codec):
    """One flipped body byte: pf_scan_pages and the oracle name the page, pyarrow refuses the file."""
    pq = pytest.importorskip("pyarrow.parquet")
    from pfloor.decoder import ParquetFile
    path, cases, _chunks = written("r20001", "all_bits", codec)[0]
    with open(path, "rb") as f:
        good = f.read()
    with ParquetFile(path) as pf:
        rows = pf.row_group_rows(0)
        ranges = [pf.chunk_range(0, col) for col in range(len(cases))]
    for col, k in ((0, 1), (4, 0), (len(cases) - 1, 2)):   # a data page behind a dictionary, a dictionary page, a last page
        pages = S.page_headers(path, col)
        p = pages[k]
        assert p["compressed"] > 0
        bad = bytearray(good)
        bad[p["body"] + p["compressed"] // 2] ^= 0x10
        rc, res = dec.scan_pages(bytes(bad), [ranges[col]  + (rows,)], verify_crc=True)
        assert rc == -2 and (res[0][0], res[0][1]) == (-2, k), (col, k, rc, res[0][:3])
        with oracle.open(data=bytes(bad)) as of:
            n, err, _pages = of.chunk_pages(0, col, verify_crc=True)
            assert n < 0 and err == k, (col, k, n, err)
        broken = str(tmp_path / f"bad_{col}.parquet")
        with open(broken, "wb") as f:
            f.write(bad)
        with pytest.raises(OSError, match="(?i)crc|checksum"):
            pq.read_table(broken, page_checksum_verification=True)


# ---------------------------------------------------------------- 3. routing and read-back
def test_bits_are_independent(dec, written):
    """Bit 8 alone: statistics and no crc; bit 16 alone: crc and no statistics; neither: no field 4, no statistics,
    no column_orders; and the data-page bodies of all four are the same bytes."""
    bodies = {}
    for st, crc in ((False, False), (True, False), (False, True), (True, True)):
        for path, cases, chunks in written("ints", "all_bits", K.SNAPPY, statistics=st, page_checksums=crc):
            fm = S.footer(path)
            assert (7 in fm) == st
            for col, case in enumerate(cases):
                pages = S.page_headers(path, col)
                assert all((p["crc"] is not None) == crc for p in pages), (st, crc, case.name)
                assert all((p["stats"] is not None) == st for p in pages if p["type"] == PAGE_DATA_V2), (st, crc, case.name)
                assert (12 in fm[4][0][1][col][3]) == st
                assert (chunks[col][2] != (None, None, None)) == st
                bodies.setdefault((path.rsplit("_", 1)[0], col), []).append([_stored(path, p) for p in pages])
            if st:
                _check_statistics(path, cases, chunks, f"bits {st} {crc}")
            if crc:
                _check_zlib(path, len(cases), f"bits {st} {crc}")
    assert bodies and all(len(b) == 4 and b[0] == b[1] == b[2] == b[3] for b in bodies.values())


def test_clear_bits_leave_the_chunk_unchanged(dec):
    """statistics=False, page_checksums=False gives the bytes of an encode without the keywords, on every route."""
    case = S.file_groups("ints")[1][1][0]
    for route, kw in S.ROUTES.items():
        for codec in (K.SNAPPY, K.UNCOMPRESSED):
            b0, c0, s0 = _encode(dec, case, codec, **kw)
            b1, c1, s1 = _encode(dec, case, codec, statistics=False, page_checksums=False, **kw)
            assert b0 == b1 and s0 == s1 == (None, None, None), route
            assert (c0.stats_flags, c0.stat_min_len, c0.stat_max_len, c0.null_count, c0.stat_min, c0.stat_max) == (0, 0, 0, 0, None, None)


@CODECS
@pytest.mark.parametrize("fid", S.STAT_FILE_IDS)
def test_round_trip(dec, oracle, written, fid, codec):
    """A file with statistics and CRCs decodes bit-exact through pyarrow, the oracle and the GPU reader."""
    pq = pytest.importorskip("pyarrow.parquet")
    from pfloor.decoder import decode_file
    for path, cases, _chunks in written(fid, "all_bits", codec):
        got = decode_file(path, decoder=dec)
        assert got["_status"] == 0, got["_error"]
        t = pq.read_table(path, page_checksum_verification=True)
        with oracle.open(path) as of:
            for col, case in enumerate(cases):
                exp = case.expected()
                o = of.decode(0, col)
                assert o["status"] == 0, (fid, case.name, o["error"])
                assert_chunk_equal(o, exp, f"{fid} {case.name} [oracle]")
                assert_chunk_equal(got[(0, col)], exp, f"{fid} {case.name} [GPU reader]")
                a = t.column(case.name).combine_chunks()
                assert a.is_valid().to_numpy(zero_copy_only=False).tolist() == case.mask().tolist(), case.name
                if case.ptype == K.BYTE_ARRAY:
                    assert [v for v in a.to_pylist() if v is not None] == case.dense, f"{fid} {case.name} [pyarrow]"
                else:
                    v = a.drop_null().to_numpy(zero_copy_only=False).astype(case.dense.dtype)
                    assert v.tobytes() == case.dense.tobytes(), f"{fid} {case.name} [pyarrow]"


def test_parquet_writer_statistics_filter_row_groups(tmp_path):
    """ParquetWriter(statistics=True, page_checksums=True), columns encoded on two contexts: pyarrow reads the chunk
    statistics, verifies the checksums, and a dataset filter above the chunk max returns no row."""
    pa = pytest.importorskip("pyarrow")
    import pyarrow.dataset as ds
    import pyarrow.parquet as pq
    from pfloor import writer as W
    from pfloor.decoder import GpuDecoder
    n = 5000
    rng = np.random.default_rng(5)
    ids = rng.integers(-10**12, 10**12, n)
    price = rng.random(n) * 100
    present = rng.random(n) >= 0.3
    words = [f"w{int(k):05d}é".encode() for k in rng.integers(0, 3000, n)]
    offsets = np.zeros(n + 1, np.int32)
    np.cumsum([len(w) for w in words], out=offsets[1:])
    chars = np.frombuffer(b"".join(words), np.uint8)
    sch = W.MessageType("m", W.required(W.INT64).named("id"), W.optional(W.DOUBLE).named("price"),
                        W.required(W.BINARY).as_string().named("word"))
    path = str(tmp_path / "w.parquet")
    d1, d2 = GpuDecoder(0), GpuDecoder(0)
    try:
        w = W.ParquetWriter(sch, path, None, decoders=[d1, d2], statistics=True, page_checksums=True, delta_fallback=True,
                            hybrid_runs=True)
        w.write_columns({"id": ids, "price": (price, np.packbits(present, bitorder="little")), "word": (offsets, chars)}, n)
        w.close()
    finally:
        d1.close()
        d2.close()
    md = pq.ParquetFile(path).metadata.row_group(0)
    st = [md.column(c).statistics for c in range(3)]
    assert all(s is not None and s.has_min_max for s in st)
    assert (st[0].min, st[0].max, st[0].null_count) == (int(ids.min()), int(ids.max()), 0)
    assert (st[1].min, st[1].max, st[1].null_count) == (price[present].min(), price[present].max(), int((~present).sum()))
    assert (st[2].min, st[2].max) == (min(words).decode(), max(words).decode())
    t = pq.read_table(path, page_checksum_verification=True)
    assert np.array_equal(t.column("id").to_numpy(), ids) and t.column("word").to_pylist() == [w_.decode() for w_ in words]
    data = ds.dataset(path, format="parquet")
    assert data.to_table(filter=ds.field("id") > int(ids.max())).num_rows == 0
    assert data.to_table(filter=ds.field("word") > max(words).decode()).num_rows == 0
    assert data.to_table(filter=ds.field("id") >= int(ids.max())).num_rows == 1
    frags = list(data.get_fragments(filter=ds.field("id") > int(ids.max())))
    assert sum(len(f.split_by_row_group(ds.field("id") > int(ids.max()))) for f in frags) == 0   # skipped by its statistics


@CODECS
def test_crc_of_levels_without_a_validity_array(dec, oracle, tmp_path, codec):
    """An OPTIONAL column handed over without a validity array (all present): the host builds the level run from
    nothing but the row count, 2,502 bytes a page, and their CRC with it; 20,001 rows end in a partial byte."""
    from pfloor import writer as W
    L = W.lib()
    n = 20001
    vals = np.arange(n, dtype=np.int64) % 1000
    path = str(tmp_path / "novalidity.parquet")
    fields = (W.WriteField * 1)(W.WriteField(b"v", W.INT64, 1, 0))
    w = C.c_void_p()
    assert L.pf_writer_open(path.encode(), fields, 1, C.byref(w)) == 0
    out = W.GpuColumnEncoder(dec).encode(W.Field("v", W.INT64, True), vals, None, n, codec=codec, statistics=True,
                                         page_checksums=True)
    assert out.statistics() == (0, struct.pack("<q", 0), struct.pack("<q", 999))
    assert L.pf_writer_add_chunk(w, 0, C.byref(out)) == 0
    assert L.pf_writer_end_row_group(w, n) == 0 and L.pf_writer_close(w) == 0
    assert _check_zlib(path, 1, "no validity") == _verify_three(dec, oracle, path, 1, "no validity") == 3
    assert [p["v2"][5] for p in S.page_headers(path, 0) if p["v2"]] == [2502, 2]


@CODECS
def test_chunk_without_rows(dec, codec):
    """0 rows: one empty data page whose statistics are null_count 0 alone and whose crc is that of its body."""
    for tname, ptype in S.TYPES:
        case = S.Case(tname, ptype, [], present=np.zeros(0, bool))
        raw, c, st = _encode(dec, case, codec, dictionary=True, statistics=True, page_checksums=True)
        h, end = S.read_struct(raw, 0)
        assert c.n_data_pages == 1 and end + h[3] == len(raw), tname
        assert h[4] & 0xffffffff == zlib.crc32(raw[end:]) and h[8][8] == {3: 0}, (tname, h)
        assert st == (0, None, None)
