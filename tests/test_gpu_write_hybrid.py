"""RLE / bit-packed hybrid streams written on the GPU in parquet-mr's run shape (PF_ENCODE_HYBRID_RUNS;
DESIGN 4.4): dictionary ids, definition levels, BOOLEAN values.

The expected bytes of every page are stated from its inputs alone: hybrid_cases.encode, a value-by-value
restatement of parquet-mr's encoder (test_write_hybrid_cpu.py reads those streams back with the oracle
and pyarrow), over the page's levels and over the ids of its present values in first-occurrence order.
The encoder must produce them byte for byte, and the files it writes are read back by three independent
readers: pyarrow, the CPU oracle and the GPU read path. One file per test id holds every case of that
id (tests/hybrid_cases.py), written once per codec and shared."""
import ctypes as C

import numpy as np
import pytest

import hybrid_cases as HC
import pagekit as K
from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

PAGE_DATA_V2 = 3


@pytest.fixture(scope="module")
def dec():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _encode(dec, case, codec, **kw):
    """pf_encode_chunk of one case -> (chunk bytes, EncodedChunk copy)."""
    from pfloor import writer as W
    data, validity = case.row_arrays()
    out = W.GpuColumnEncoder(dec).encode(W.Field(case.name, case.ptype, case.optional), data, validity, case.rows,
                                         page_rows=case.page_rows, codec=codec, **kw)
    return C.string_at(out.bytes, out.size), W.EncodedChunk.from_buffer_copy(out)


def _write(dec, path, rows, cases, codec, **kw):
    """The cases as one row group -> [(data_encoding, fallback, n_data_pages, dict_entries)]."""
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
        chunks.append((out.data_encoding, out.fallback, out.n_data_pages, out.dict_entries))
        assert L.pf_writer_add_chunk(w, i, C.byref(out)) == 0
    assert L.pf_writer_end_row_group(w, rows) == 0
    assert L.pf_writer_close(w) == 0
    return chunks


@pytest.fixture(scope="module")
def written(dec, tmp_path_factory):
    """written(fid, codec) -> (path, chunks); every chunk with dictionary = 1 | 4, each file once."""
    root = tmp_path_factory.mktemp("hybrid")
    cache = {}

    def get(fid, codec):
        if (fid, codec) not in cache:
            rows, cases = HC.file_cases(fid)
            path = str(root / f"{fid}_{codec}.parquet")
            cache[(fid, codec)] = (path, _write(dec, path, rows, cases, codec, dictionary=True, hybrid_runs=True))
        return cache[(fid, codec)]
    return get


def _data_pages(path, col):
    """[(encoding, num_values, num_nulls, def_bytes, stored page body)] of the chunk's data pages."""
    from pfloor.decoder import ParquetFile
    with ParquetFile(path) as pf:
        start, size = pf.chunk_range(0, col)
        d = pf.chunk_desc(0, col, 0)
        pages = [(d.pages[i].page_type, d.pages[i].offset, d.pages[i].compressed_size, d.pages[i].encoding,
                  d.pages[i].num_values, d.pages[i].num_nulls, d.pages[i].def_bytes) for i in range(d.n_pages)]
    with open(path, "rb") as f:
        f.seek(start)
        raw = f.read(size)
    return [(enc, nv, nn, db, raw[off:off + cs]) for pt, off, cs, enc, nv, nn, db in pages if pt == PAGE_DATA_V2]


def _same(got, exp, label):
    if got != exp:
        g, e = np.frombuffer(got, np.uint8), np.frombuffer(exp, np.uint8)
        m = min(len(g), len(e))
        bad = np.flatnonzero(g[:m] != e[:m])
        raise AssertionError(f"{label}: {len(g)} bytes for {len(e)}, first difference at {bad[:1]}")


# ---------------------------------------------------------------- 1. exact bytes
@pytest.mark.parametrize("fid", HC.FILE_IDS)
def test_exact_bytes(dec, written, fid):
    """UNCOMPRESSED: every data page is the reference stream of its levels, then the width byte and the
    reference stream of its ids (or the 4-byte length and the stream of its BOOLEAN values)."""
    path, chunks = written(fid, K.UNCOMPRESSED)
    _rows, cases = HC.file_cases(fid)
    for col, case in enumerate(cases):
        exp_pages = case.pages()
        if case.rows == 0:   # no value, no dictionary: one empty PLAIN page
            raw, c = _encode(dec, case, K.UNCOMPRESSED, dictionary=True, hybrid_runs=True)
            assert (c.data_encoding, c.n_data_pages, c.dict_entries) == (K.PLAIN, 1, 0) and len(raw) < 64
            continue
        boolean = case.ptype == K.BOOLEAN
        assert chunks[col] == (case.encoding, 3 if boolean else 0, len(exp_pages), 0 if boolean else len(case.dictionary)), \
            (fid, case.name, chunks[col])
        got = _data_pages(path, col)
        assert len(got) == len(exp_pages), (fid, case.name)
        for k, ((enc, nv, nn, db, body), (present, vals, ids)) in enumerate(zip(got, exp_pages)):
            label = f"{fid} {case.name} page {k}"
            assert enc == case.encoding, label
            assert nv - nn == len(vals), label
            _same(body[:db], case.levels_stream(present), label + " levels")
            _same(body[db:], case.values_stream(ids), label + " values")


# ---------------------------------------------------------------- 2. round trip
@pytest.mark.parametrize("codec", [K.SNAPPY, K.UNCOMPRESSED], ids=["snappy", "uncompressed"])
@pytest.mark.parametrize("fid", [f for f in HC.FILE_IDS if f != "r0"])
def test_round_trip(dec, oracle, written, fid, codec):
    """pyarrow, the oracle and the GPU reader return the inputs: values and validity."""
    pq = pytest.importorskip("pyarrow.parquet")
    from pfloor.decoder import decode_file
    path, chunks = written(fid, codec)
    rows, cases = HC.file_cases(fid)
    assert all(c[0] == case.encoding for c, case in zip(chunks, cases))
    got = decode_file(path, decoder=dec)
    assert got["_status"] == 0, got["_error"]
    with oracle.open(path) as of:
        for col, case in enumerate(cases):
            exp = case.expected()
            o = of.decode(0, col)
            assert o["status"] == 0, (fid, case.name, o["error"])
            assert_chunk_equal(o, exp, f"{fid} {case.name} [oracle]")
            assert_chunk_equal(got[(0, col)], exp, f"{fid} {case.name} [GPU reader]")
    t = pq.ParquetFile(path).read_row_group(0)
    assert t.num_rows == rows
    for case in cases:
        assert t.column(case.name).to_pylist() == case.pylist(), f"{fid} {case.name} [pyarrow]"


# ---------------------------------------------------------------- 3. routing
def _routing_cases():
    rng = np.random.default_rng(11)
    present = rng.random(3000) >= 0.3
    present[1000:2100] = True                     # a page and more without nulls
    m = int(present.sum())
    return (HC.Case("i", K.INT32, np.sort(rng.integers(-2**31, 2**31 - 1, m)), present=present, page_rows=1000),   # ~2100 distinct
            HC.Case("b", K.BOOLEAN, HC._bool_family("longruns", m, "routing"), present=present, page_rows=1000))


def test_routing_bit_clear_is_unchanged(dec):
    """hybrid_runs=False gives the bytes of an encode without the keyword, whatever the other bits."""
    for case in _routing_cases():
        for kw in ({}, {"dictionary": False}, {"delta_fallback": True, "dict_page_limit": 256}):
            for codec in (K.SNAPPY, K.UNCOMPRESSED):
                b0, c0 = _encode(dec, case, codec, **kw)
                b1, c1 = _encode(dec, case, codec, hybrid_runs=False, **kw)
                assert b0 == b1 and (c0.data_encoding, c0.fallback) == (c1.data_encoding, c1.fallback), (case.name, kw)
                assert c0.data_encoding != K.RLE


def test_routing_plain_and_delta_values_keep_hybrid_levels(dec, tmp_path):
    """1 | 4 with a dictionary over the limit: PLAIN values; 2 | 4: DELTA_BINARY_PACKED values; the levels of
    both are the reference stream, and the values sections are what they are without the bit."""
    case = _routing_cases()[0]
    for name, kw, enc, fb in (("plain", {"dictionary": True, "dict_page_limit": 256}, K.PLAIN, 1),
                              ("delta", {"dictionary": False, "delta_fallback": True}, K.DELTA_BINARY_PACKED, 0)):
        path = str(tmp_path / f"{name}.parquet")
        chunks = _write(dec, path, case.rows, [case], K.UNCOMPRESSED, hybrid_runs=True, **kw)
        assert chunks[0][:2] == (enc, fb), (name, chunks)
        got = _data_pages(path, 0)
        assert len(got) == 3
        for k, ((e, nv, nn, db, body), (present, vals, _ids)) in enumerate(zip(got, case.pages())):
            assert e == enc and nv - nn == len(vals)
            _same(body[:db], case.levels_stream(present), f"{name} page {k} levels")
            exp = K.plain(K.INT32, case.pagekit_vals(vals)) if enc == K.PLAIN else K.dbp([int(v) for v in vals], bits=32)
            _same(body[db:], exp, f"{name} page {k} values")
        assert got[1][3] == 3                                 # 1,000 rows without a null: three bytes of levels,
        assert got[1][4][:3] == bytes([0xd0, 0x0f, 0x01])     # varint(1000 << 1) and the value 1


def test_routing_boolean_is_rle(dec, oracle, tmp_path):
    """BOOLEAN with bit 4 alone: RLE pages (fallback 0; 3 when the dictionary bit was asked for), and the
    footer lists RLE and no PLAIN."""
    pq = pytest.importorskip("pyarrow.parquet")
    from pfloor import writer as W
    from pfloor.decoder import decode_file
    case = _routing_cases()[1]
    b4, c4 = _encode(dec, case, K.SNAPPY, dictionary=False, hybrid_runs=True)
    b5, c5 = _encode(dec, case, K.SNAPPY, dictionary=True, hybrid_runs=True)
    b7, c7 = _encode(dec, case, K.SNAPPY, dictionary=True, delta_fallback=True, hybrid_runs=True)
    assert (c4.data_encoding, c4.fallback) == (K.RLE, 0) and (c5.data_encoding, c5.fallback) == (K.RLE, 3)
    assert (c7.data_encoding, c7.fallback) == (K.RLE, 3) and b4 == b5 == b7
    path = str(tmp_path / "b.parquet")
    sch = W.MessageType("m", W.optional(W.BOOLEAN).named("flag"), W.required(W.BOOLEAN).named("req"))
    data, validity = case.row_arrays()
    w = W.ParquetWriter(sch, path, None, decoder=dec, hybrid_runs=True)
    w.write_columns({"flag": (data, validity), "req": data}, case.rows)
    assert [(e[1], e[2]) for e in w.last_chunks] == [(K.RLE, 3), (K.RLE, 3)]
    w.close()
    pf = pq.ParquetFile(path)
    for col in (0, 1):
        listed = pf.metadata.row_group(0).column(col).encodings
        assert "RLE" in listed and "PLAIN" not in listed, listed
    t = pf.read()
    assert t.column("flag").to_pylist() == case.pylist()
    assert t.column("req").to_pylist() == data.astype(bool).tolist()
    got = decode_file(path, decoder=dec)
    assert got["_status"] == 0, got["_error"]
    with oracle.open(path) as of:
        for col in (0, 1):
            assert_chunk_equal(got[(0, col)], of.decode(0, col), f"boolean c{col}")
    assert_chunk_equal(got[(0, 0)], case.expected(), "boolean [GPU reader]")


def test_routing_reference_write_read_test(dec, tmp_path):
    """ParquetReadWriteTest.java:28-83 with the encodings of parquet-mr's v2 writer: the reference's records
    through ParquetWriter(delta_fallback=True, hybrid_runs=True), the GPU reader and a Hydrator."""
    from pfloor import writer as W
    from pfloor.reader import Hydrator, HydratorSupplier, ParquetReader

    sch = W.MessageType("foo", W.required(W.INT64).named("id"), W.required(W.BINARY).as_string().named("email"))

    class Deh(W.Dehydrator):
        def dehydrate(self, record, vw):
            vw.write("id", record[0])
            vw.write("email", record[1])

    class MapHydrator(Hydrator):
        def start(self):
            return {}

        def add(self, target, heading, value):
            r = dict(target)
            r[heading] = value
            return r

        def finish(self, target):
            return target

    path = str(tmp_path / "foo.parquet")
    w = W.ParquetWriter.writeFile(sch, path, Deh(), decoder=dec, delta_fallback=True, hybrid_runs=True)
    w.write([1, "hello1@example.com"])
    w.write([2, "hello2@example.com"])
    w.close()
    assert [e[1] for e in w.last_chunks] == [K.RLE_DICTIONARY, K.RLE_DICTIONARY]
    rows = list(ParquetReader.streamContent(path, HydratorSupplier.constantly(MapHydrator())))
    assert rows == [{"id": 1, "email": "hello1@example.com"}, {"id": 2, "email": "hello2@example.com"}]
    rows = list(ParquetReader.streamContent(path, HydratorSupplier.constantly(MapHydrator()), ["id"]))
    assert rows == [{"id": 1}, {"id": 2}]


# ---------------------------------------------------------------- 4. size
def test_constant_optional_column_is_a_few_bytes(dec, tmp_path):
    """40,000 rows of one value without nulls: two pages whose levels are c0 b8 02 01 and whose ids are one
    RLE run at width 0; under 100 bytes of page bodies where the bit-packed form takes over 10,000."""
    n = 40000
    case = HC.Case("c", K.INT32, np.full(n, 12345, np.int32), present=np.ones(n, bool))
    path = str(tmp_path / "const.parquet")
    chunks = _write(dec, path, n, [case], K.UNCOMPRESSED, dictionary=True, hybrid_runs=True)
    assert chunks[0] == (K.RLE_DICTIONARY, 0, 2, 1)
    got = _data_pages(path, 0)
    assert len(got) == 2
    for _enc, nv, nn, db, body in got:
        assert (nv, nn, db) == (20000, 0, 4)
        assert body == bytes.fromhex("c0b80201") + bytes.fromhex("00c0b802")
    raw, c = _encode(dec, case, K.UNCOMPRESSED, dictionary=True, hybrid_runs=True)
    assert sum(len(b[4]) for b in got) + 4 < 100 and len(raw) < 200
    old, _c = _encode(dec, case, K.UNCOMPRESSED, dictionary=True)
    assert len(old) > 10000
