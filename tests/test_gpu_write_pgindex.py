"""The page index built on the GPU (PF_ENCODE_PAGE_INDEX, k_enc_pgindex).

Every case of pgindex_cases runs pf_encode_chunk with bit 32 and must give the reference's lists, boundary order and
validity flag exactly; test_write_pgindex_cpu.py pins that reference to what pyarrow writes. Page locations are compared
with a host walk of the chunk's bytes, and the bytes themselves with those of the same encode without the bit."""
import ctypes as C

import numpy as np
import pytest

import pagekit as K
import pgindex_cases as P
import stats_cases as S
from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

SNAPPY, UNCOMPRESSED, ZSTD = 1, 0, 6
CODECS = {"snappy": SNAPPY, "uncompressed": UNCOMPRESSED, "zstd": ZSTD}


@pytest.fixture(scope="module")
def dec():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _encode(dec, case, codec=SNAPPY, page_index=True, **kw):
    """pf_encode_chunk of one case -> (chunk bytes, EncodedChunk copy, ColumnIndex lists or None, page locations or None)."""
    from pfloor import writer as W
    data, validity = case.row_arrays()
    kw.setdefault("index_truncate", case.T)
    out = W.GpuColumnEncoder(dec).encode(W.Field(case.name, case.ptype, case.optional), data, validity, case.rows,
                                         page_rows=case.page_rows, codec=codec, page_index=page_index, **kw)
    return C.string_at(out.bytes, out.size), W.EncodedChunk.from_buffer_copy(out), out.page_column_index(), out.page_locations()


def _walk(body, first_rows=True):
    """The data pages of a chunk's bytes, by their headers: [(offset, header + stored body, first row)]."""
    out, pos, row = [], 0, 0
    while pos < len(body):
        h, end = S.read_struct(body, pos)
        size = end - pos + h[3]
        if h[1] == 3:
            out.append((pos, size, row))
            row += h[8][3]
        else:
            assert h[1] == 2 and pos == 0, "a dictionary page comes first"
        pos += size
    assert pos == len(body)
    return out


def _check(case, body, out, ci, locs, label=""):
    ref = case.ref()
    tag = f"{case.name} {label}"
    assert out.index_pages == out.n_data_pages == len(case.pages), tag
    assert locs == _walk(body), tag
    assert [r for _o, _s, r in locs] == case.first_rows(), tag
    assert out.column_index == int(ref["valid"]), tag
    assert [bool(out.index_null_pages[i]) for i in range(out.index_pages)] == ref["null_pages"], tag
    assert [out.index_null_counts[i] for i in range(out.index_pages)] == ref["null_counts"], tag
    if ref["valid"]:
        for k in ("null_pages", "null_counts", "min_values", "max_values", "boundary_order"):
            assert ci[k] == ref[k], f"{tag}: {k}"
    else:
        assert ci is None and out.boundary_order == 0 and not out.index_values and not out.index_value_off, tag


# ---------------------------------------------------------------- 1. every case
@pytest.mark.parametrize("name", P.names())
def test_encode_gives_the_reference(dec, name):
    """Lists, order, validity and page locations; and the chunk's bytes do not change: bit 32 alone gives the bytes of
    no bit, bits 8 | 32 those of bit 8."""
    case = P.cases()[name]
    body, out, ci, locs = _encode(dec, case)
    _check(case, body, out, ci, locs)
    assert out.stats_flags == 0
    plain, pout, pci, plocs = _encode(dec, case, page_index=False)
    assert plain == body, name
    assert pci is None and plocs is None and pout.index_pages == 0 and pout.column_index == 0 and pout.boundary_order == 0
    assert not pout.page_offset and not pout.index_values and not pout.index_null_pages
    sbody, sout, sci, slocs = _encode(dec, case, statistics=True)
    _check(case, sbody, sout, sci, slocs, "with statistics")
    assert sbody == _encode(dec, case, page_index=False, statistics=True)[0], name


# ---------------------------------------------------------------- 2. routes, codecs, the other options
_ROUTES = dict(S.ROUTES, plain=dict(dictionary=False))


@pytest.mark.parametrize("name", P.OPTION_CASES + ("s_pages_257_random", "i64_pages_257_break_255", "s_T2047"))
def test_every_route_gives_the_same_index(dec, name):
    """The index depends on the values alone: dictionary ids, PLAIN, DELTA_*, hybrid runs and ZSTD pages carry the same one."""
    case = P.cases()[name]
    encodings = set()
    for route, kw in _ROUTES.items():
        for cname, codec in CODECS.items():
            body, out, ci, locs = _encode(dec, case, codec=codec, **kw)
            _check(case, body, out, ci, locs, f"{route} {cname}")
            encodings.add(out.data_encoding)
    if case.ptype != K.BOOLEAN:
        assert K.RLE_DICTIONARY in encodings and K.PLAIN in encodings
    if case.ptype in (K.INT32, K.INT64, K.BYTE_ARRAY):
        assert encodings & {K.DELTA_BINARY_PACKED, K.DELTA_BYTE_ARRAY}


@pytest.mark.parametrize("cname", list(CODECS))
@pytest.mark.parametrize("name", P.OPTION_CASES)
def test_all_options_together(dec, name, cname):
    """Page CRCs, statistics and a Bloom filter with the index, under every codec: headers grow and bodies shrink, the
    offsets and sizes follow them."""
    case = P.cases()[name]
    kw = dict(statistics=True, page_checksums=True, bloom_bytes=64, hybrid_runs=True, delta_fallback=True)
    body, out, ci, locs = _encode(dec, case, codec=CODECS[cname], **kw)
    _check(case, body, out, ci, locs, cname)
    assert body == _encode(dec, case, codec=CODECS[cname], page_index=False, **kw)[0]
    for off, _size, _row in locs:
        h, _end = S.read_struct(body, off)
        assert 4 in h, "crc"


# ---------------------------------------------------------------- 3. inputs in device memory
@pytest.mark.parametrize("name", ["i32_pages_257_random", "s_pages_65_random", "s_5000_T64", "f64_nan_only_with_nulls"])
def test_on_device_inputs(dec, name):
    from pfloor import writer as W
    L = W.lib()
    case = P.cases()[name]
    data, validity = case.row_arrays()
    held = []

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        assert L.pf_device_alloc(dec.h, max(arr.nbytes, 1), C.byref(p)) == 0
        held.append((p, arr))
        assert L.pf_memcpy_h2d(dec.h, p, arr.ctypes.data, arr.nbytes) == 0
        return p.value

    c = W.EncodeColumn()
    c.physical_type, c.max_def, c.num_rows = case.ptype, int(case.optional), case.rows
    try:
        if validity is not None:
            c.validity = upload(validity)
        if case.ptype == K.BYTE_ARRAY:
            c.offsets, c.chars, c.chars_len = upload(data[0]), upload(data[1]), data[1].size
        else:
            c.values = upload(data)
        # the uploads are asynchronous on the context's stream; an encode ends with the stream synchronised
        _encode(dec, P.cases()["i32_pages_1_ascending"])
        c.dictionary, c.page_rows, c.codec, c.index_truncate = 1 | W.ENCODE_PAGE_INDEX, case.page_rows, SNAPPY, case.T
        out = W.EncodedChunk()
        assert L.pf_encode_chunk(dec.h, C.byref(c), 1, C.byref(out)) == 0, L.pf_last_error(dec.h)
        body = C.string_at(out.bytes, out.size)
        _check(case, body, W.EncodedChunk.from_buffer_copy(out), out.page_column_index(), out.page_locations(), "on device")
    finally:
        for p, _arr in held:
            L.pf_device_free(dec.h, p)
    assert body == _encode(dec, case)[0]


# ---------------------------------------------------------------- 4. arguments
def test_index_truncate_range(dec):
    from pfloor._native import PfError
    case = P.cases()["s_empty"]
    for bad in (-2, 2048, 1 << 20, -(1 << 31)):
        with pytest.raises(PfError) as e:
            _encode(dec, case, index_truncate=bad)
        assert e.value.code == -1
        _encode(dec, case, index_truncate=bad, page_index=False)                      # ignored with the bit clear
        _encode(dec, P.cases()["i32_ascending"], index_truncate=bad)                  # and for the other types
    for ok in (-1, 0, 1, 2047):
        _encode(dec, case, index_truncate=ok)


def test_empty_chunk(dec):
    """No rows: one empty page, a null page; the ColumnIndex is there and UNORDERED."""
    from pfloor import writer as W
    out = W.GpuColumnEncoder(dec).encode(W.Field("e", K.INT64, True), np.zeros(0, np.int64), None, 0, page_index=True)
    assert out.index_pages == 1 and out.column_index == 1 and out.boundary_order == 0
    ci = out.page_column_index()
    assert ci == {"null_pages": [True], "min_values": [b""], "max_values": [b""], "boundary_order": 0, "null_counts": [0]}
    assert out.page_locations() == _walk(C.string_at(out.bytes, out.size))


# ---------------------------------------------------------------- 5. files
def _columns(cases):
    cols = {}
    for c in cases:
        data, validity = c.row_arrays()
        if c.ptype == K.BYTE_ARRAY:
            cols[c.name] = (data[0], data[1], validity) if validity is not None else data
        else:
            cols[c.name] = (data, validity) if validity is not None else data
    return cols


def _schema(W, cases):
    return W.MessageType("m", *[W.Field(c.name, c.ptype, c.optional) for c in cases])


def _file_cases():
    """Five pages of 8 rows per column, every type: ascending, descending, tied, unordered, with null rows and a null page."""
    spec = {"i32": [(0, 5), (10, 15), (20, 25), (30, 35), (40, 45)], "i64": [(40, 45), (30, 35), (20, 25), (10, 15), (0, 5)],
            "f32": [(3, 9)] * 5, "f64": [(0, 50), (10, 60), (20, 55), None, (30, 70)], "b": [(0, 0), (0, 0), (0, 1), (1, 1), (1, 1)],
            "s": [(0, 5), None, (5, 5), (7, 9), (9, 30)]}
    out = []
    for tname, ptype in P.TYPES:
        pages = [P.NULL_PAGE if s is None else P.span(ptype, s[0], s[1], nulls=(k,) if tname in ("f64", "s", "i64") else ())
                 for k, s in enumerate(spec[tname])]
        out.append(P.IndexCase(f"{tname}_col", ptype, pages))
    return out


@pytest.mark.parametrize("parallel", [False, True], ids=["one_context", "two_contexts"])
@pytest.mark.parametrize("T", [0, -1])
def test_parquet_writer_files(dec, tmp_path, T, parallel):
    """ParquetWriter(page_index=True), two row groups: this reader and pyarrow read the data back bit-exact;
    pf_file_column_index / pf_file_offset_index return the reference's lists and the pages' places; the layout is
    ColumnIndexes, OffsetIndexes, Bloom filter, footer; with T = -1 the index is the one pyarrow writes for the data."""
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    from pfloor import writer as W
    from pfloor.decoder import GpuDecoder, ParquetFile, decode_file
    cases = _file_cases()
    assert all(c.rows == 40 for c in cases)
    path = str(tmp_path / "w.parquet")
    d2 = GpuDecoder(0) if parallel else None
    try:
        w = W.ParquetWriter(_schema(W, cases), path, None, decoder=None if parallel else dec, decoders=[dec, d2] if parallel else None,
                            page_index=True, index_truncate=T, bloom_filters={"i32_col": {"bytes": 64}}, statistics=parallel,
                            page_rows=8)
        for _ in range(2):
            w.write_columns(_columns(cases), 40)
        w.close()
    finally:
        if d2:
            d2.close()
    raw = open(path, "rb").read()
    fm = S.footer(path)
    ccs = [cc for rg in fm[4] for cc in rg[1]]
    pos = max(cc[3].get(11, cc[3][9]) + cc[3][7] for cc in ccs)   # the end of the last row group
    for cc in ccs:
        assert cc[6] == pos
        pos += cc[7]
    for cc in ccs:
        assert cc[4] == pos
        pos += cc[5]
    blooms = [cc[3][14] for cc in ccs if 14 in cc[3]]
    assert blooms == sorted(blooms) and blooms[0] == pos and len(blooms) == 2
    assert fm[7] == [{1: {}}] * len(cases)
    got = decode_file(path, decoder=dec)
    assert got["_status"] == 0, got["_error"]
    t = pq.read_table(path)
    with ParquetFile(path) as f:
        for rg in range(2):
            for col, case in enumerate(cases):
                assert_chunk_equal(got[(rg, col)], case.expected(), f"{case.name} rg{rg} [GPU reader]")
                idx = f.page_index(rg, col)
                ref = case.ref(T=64 if T == 0 else -1)
                assert ref["valid"]
                assert idx["column_index"] == {k: ref[k] for k in ("null_pages", "min_values", "max_values", "boundary_order", "null_counts")}
                start, size = f.chunk_range(rg, col)
                with open(path, "rb") as fh:
                    fh.seek(start)
                    chunk = fh.read(size)
                assert idx["offset_index"] == [(start + o, s, r) for o, s, r in _walk(chunk)]
    for case in cases:
        a = t.column(case.name).combine_chunks()
        assert a.is_valid().to_numpy(zero_copy_only=False).tolist() == case.mask().tolist() * 2, case.name
        if case.ptype == K.BYTE_ARRAY:
            assert [v for v in a.to_pylist() if v is not None] == case.dense * 2
        else:
            v = a.drop_null().to_numpy(zero_copy_only=False).astype(case.dense.dtype)
            assert v.tobytes() == case.dense.tobytes() * 2, case.name
    if T == -1:   # pyarrow's own index for the same data
        theirs = str(tmp_path / "pa.parquet")
        pq.write_table(pa.table({c.name: c.arrow() for c in cases}), theirs, data_page_version="2.0", use_dictionary=False,
                       write_page_index=True, write_batch_size=8, data_page_size=0, row_group_size=40)
        tfm, traw = S.footer(theirs), open(theirs, "rb").read()
        for col in range(len(cases)):
            mine = S.read_struct(raw, fm[4][0][1][col][6])[0]
            other = S.read_struct(traw, tfm[4][0][1][col][6])[0]
            assert {k: mine[k] for k in (1, 2, 3, 4, 5)} == {k: other[k] for k in (1, 2, 3, 4, 5)}, cases[col].name
            assert [l[3] for l in S.read_struct(raw, fm[4][0][1][col][4])[0][1]] == \
                [l[3] for l in S.read_struct(traw, tfm[4][0][1][col][4])[0][1]]


def test_parquet_writer_default_has_no_index(dec, tmp_path):
    from pfloor import writer as W
    from pfloor.decoder import ParquetFile
    case = P.cases()["i32_ascending"]
    path = str(tmp_path / "d.parquet")
    w = W.ParquetWriter(_schema(W, [case]), path, None, decoder=dec)
    w.write_columns(_columns([case]), case.rows)
    w.close()
    cc = S.footer(path)[4][0][1][0]
    assert set(cc) == {2, 3}
    with ParquetFile(path) as f:
        assert f.page_index(0, 0) == {"offset_index": None, "column_index": None}
