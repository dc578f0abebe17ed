"""DELTA_BINARY_PACKED / DELTA_BYTE_ARRAY pages written on the GPU (PF_ENCODE_DELTA_FALLBACK).

The expected bytes of every page are stated from its inputs alone: pagekit's CPU encoder over the
page's present values (parquet-mr's layout; test_write_delta_cpu.py reads those streams back with the
oracle and pyarrow). The encoder must produce them byte for byte, and the files it writes are read
back by three independent readers: pyarrow, the CPU oracle and the GPU read path. One file per test
id holds every case of that id (tests/delta_cases.py), written once per codec and shared."""
import ctypes as C

import numpy as np
import pytest

import delta_cases as DC
import pagekit as K
from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

PLAIN, DBP, DBA, RLE_DICT = K.PLAIN, K.DELTA_BINARY_PACKED, K.DELTA_BYTE_ARRAY, K.RLE_DICTIONARY
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


def _write(dec, path, rows, cases, codec):
    """The cases as one row group, every chunk with dictionary = PF_ENCODE_DELTA_FALLBACK (2)."""
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
        out = enc.encode(W.Field(case.name, case.ptype, case.optional), data, validity, rows, dictionary=False,
                         page_rows=case.page_rows, codec=codec, delta_fallback=True)
        chunks.append((out.data_encoding, out.fallback, out.n_data_pages, out.dict_entries))
        assert L.pf_writer_add_chunk(w, i, C.byref(out)) == 0
    assert L.pf_writer_end_row_group(w, rows) == 0
    assert L.pf_writer_close(w) == 0
    return chunks


@pytest.fixture(scope="module")
def written(dec, tmp_path_factory):
    """written(fid, codec) -> (path, [(data_encoding, fallback, n_data_pages, dict_entries)]); each file once."""
    root = tmp_path_factory.mktemp("delta")
    cache = {}

    def get(fid, codec):
        if (fid, codec) not in cache:
            rows, cases = DC.file_cases(fid)
            path = str(root / f"{fid}_{codec}.parquet")
            cache[(fid, codec)] = (path, _write(dec, path, rows, cases, codec))
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
    return [(enc, nv, nn, db, raw[off:off + cs]) for pt, off, cs, enc, nv, nn, db in pages if pt == PAGE_DATA_V2], raw


# ---------------------------------------------------------------- 1. exact bytes
@pytest.mark.parametrize("fid", DC.FILE_IDS)
def test_exact_bytes(dec, written, fid):
    """UNCOMPRESSED: the values section of every data page is pagekit's stream of the page's present values."""
    path, chunks = written(fid, K.UNCOMPRESSED)
    _rows, cases = DC.file_cases(fid)
    for col, case in enumerate(cases):
        exp_pages = case.pages()
        assert chunks[col][:3] == (case.encoding, 0, len(exp_pages)), (fid, case.name, chunks[col])
        got, raw = _data_pages(path, col)
        if case.rows == 0:   # the page walk of a chunk without values finds no page: look at the encoder's bytes
            raw, c = _encode(dec, case, K.UNCOMPRESSED, dictionary=False, delta_fallback=True)
            assert got == [] and c.data_encoding == case.encoding and c.n_data_pages == 1
            assert raw.endswith(case.stream([])) and len(raw) < 64, (fid, case.name, raw)   # header | empty stream
            continue
        assert len(got) == len(exp_pages), (fid, case.name)
        for k, ((enc, nv, nn, db, body), (present, vals)) in enumerate(zip(got, exp_pages)):
            label = f"{fid} {case.name} page {k}"
            assert enc == case.encoding, label
            assert nv - nn == len(vals), label
            exp = case.stream(vals)
            if body[db:] != exp:
                g, e = np.frombuffer(body[db:], np.uint8), np.frombuffer(exp, np.uint8)
                m = min(len(g), len(e))
                bad = np.flatnonzero(g[:m] != e[:m])
                raise AssertionError(f"{label}: {len(g)} bytes for {len(e)}, first difference at {bad[:1]}")


# ---------------------------------------------------------------- 2. round trip
@pytest.mark.parametrize("codec", [K.SNAPPY, K.UNCOMPRESSED], ids=["snappy", "uncompressed"])
@pytest.mark.parametrize("fid", DC.FILE_IDS)
def test_round_trip(dec, oracle, written, fid, codec):
    """pyarrow, the oracle and the GPU reader return the inputs: values, validity, offsets and chars."""
    pq = pytest.importorskip("pyarrow.parquet")
    from pfloor.decoder import decode_file
    path, chunks = written(fid, codec)
    rows, cases = DC.file_cases(fid)
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
def test_routing_dictionary_and_delta_bits(dec):
    """dictionary is a bit set: 3 falls back to DELTA_* (fallback 1) or keeps a dictionary that fits, with the
    bytes of dictionary = 1; 2 writes DELTA_* pages with fallback 0; 0 and 1 stay PLAIN on fallback."""
    for pt, fam in ((K.INT32, "uniform"), (K.INT64, "uniform"), (K.BYTE_ARRAY, "text")):
        case = DC.Case("c", pt, fam, 3000, "nulls", 1000)     # ~2100 distinct values
        delta = DBA if pt == K.BYTE_ARRAY else DBP
        b3, c3 = _encode(dec, case, K.SNAPPY, dictionary=True, delta_fallback=True, dict_page_limit=256)
        assert (c3.data_encoding, c3.fallback, c3.dict_entries, c3.dictionary_page_offset) == (delta, 1, 0, -1)
        b2, c2 = _encode(dec, case, K.SNAPPY, dictionary=False, delta_fallback=True)
        assert (c2.data_encoding, c2.fallback) == (delta, 0)
        assert b2 == b3                                       # the fallback chunk is the plain delta chunk
        b3f, c3f = _encode(dec, case, K.SNAPPY, dictionary=True, delta_fallback=True)
        b1f, c1f = _encode(dec, case, K.SNAPPY, dictionary=True)
        assert (c3f.data_encoding, c3f.fallback) == (RLE_DICT, 0) and c3f.dict_entries > 0
        assert b3f == b1f                                     # a chunk that keeps its dictionary is unchanged
        b1, c1 = _encode(dec, case, K.UNCOMPRESSED, dictionary=True, dict_page_limit=256)
        b0, c0 = _encode(dec, case, K.UNCOMPRESSED, dictionary=False)
        assert (c1.data_encoding, c1.fallback) == (PLAIN, 1) and (c0.data_encoding, c0.fallback) == (PLAIN, 0)
        assert b1 == b0
        # and those PLAIN bytes are what they always were: header | validity bits | PLAIN values, per page
        pos = 0
        for present, vals in case.pages():
            body = K.plain(pt, case.pagekit_vals(vals))
            k = b0.find(body, pos)
            assert k >= 0, "PLAIN values section not found"
            pos = k + len(body)
        assert pos == len(b0)


def test_routing_float_double_boolean_stay_plain(dec):
    """FLOAT, DOUBLE and BOOLEAN ignore the delta bit: bytes identical to the bit clear."""
    from pfloor import writer as W
    rng = np.random.default_rng(3)
    n = 3000
    validity = np.packbits(rng.random(n) >= 0.3, bitorder="little")
    cols = {W.FLOAT: rng.random(n).astype(np.float32), W.DOUBLE: rng.random(n), W.BOOLEAN: (rng.random(n) < 0.5).astype(np.uint8)}
    enc = W.GpuColumnEncoder(dec)
    for pt, arr in cols.items():
        for dictionary in (False, True):
            res = []
            for delta in (False, True):
                out = enc.encode(W.Field("c", pt, True), arr, validity, n, dictionary=dictionary, page_rows=1000,
                                 dict_page_limit=256, delta_fallback=delta)
                res.append((C.string_at(out.bytes, out.size), out.data_encoding, out.fallback))
            assert res[0] == res[1], (pt, dictionary)
            assert res[1][1] == PLAIN and res[1][2] == ((3 if pt == W.BOOLEAN else 1) if dictionary else 0)


# ---------------------------------------------------------------- 4. writer
def test_parquet_writer_delta_fallback(dec, oracle, tmp_path):
    """ParquetWriter(delta_fallback=True), two row groups of a mixed schema: columns whose dictionary is
    over the page limit come out DELTA_*, the others as before; pyarrow and the GPU reader return the rows."""
    pq = pytest.importorskip("pyarrow.parquet")
    from pfloor import writer as W
    from pfloor.decoder import decode_file
    sch = W.MessageType("m", W.required(W.INT64).named("key"), W.optional(W.INT32).named("qty"),
                        W.required(W.BINARY).as_string().named("comment"), W.required(W.DOUBLE).named("price"),
                        W.required(W.BOOLEAN).named("flag"), W.required(W.INT32).named("small"))
    path = str(tmp_path / "w.parquet")
    w = W.ParquetWriter(sch, path, None, decoder=dec, delta_fallback=True)
    groups, encs = [], []
    for seed, n in ((1, 150001), (2, 140000)):
        rng = np.random.default_rng(seed)
        present = rng.random(n) >= 0.3
        words = [b"note %09d %s" % (i * 7919 % 10**9, b"x" * (i % 11)) for i in range(n)]   # distinct: ~3 MB dictionary
        offs = np.zeros(n + 1, np.int32)
        np.cumsum([len(x) for x in words], out=offs[1:])
        cols = {"key": np.cumsum(rng.integers(1, 5, n)).astype(np.int64),                  # distinct: 1.2 MB dictionary
                "qty": (np.where(present, rng.integers(-2**31, 2**31 - 1, n), 0).astype(np.int32), np.packbits(present, bitorder="little")),
                "comment": (offs, np.frombuffer(b"".join(words), np.uint8)),
                "price": rng.random(n), "flag": (rng.random(n) < 0.5).astype(np.uint8),
                "small": rng.integers(0, 50, n).astype(np.int32)}
        w.write_columns(cols, n)
        encs.append([(e[1], e[2]) for e in w.last_chunks])
        groups.append((cols, present, words, n))
    w.close()
    # key, comment: dictionary over 1 MiB -> DELTA_*; qty: ~105,000 distinct INT32 = 420 KB dictionary kept;
    # price: 1.2 MB dictionary -> PLAIN (DOUBLE has no delta encoding); flag: BOOLEAN; small: dictionary
    for e in encs:
        assert e == [(DBP, 1), (RLE_DICT, 0), (DBA, 1), (PLAIN, 1), (PLAIN, 3), (RLE_DICT, 0)], e
    md = pq.ParquetFile(path).metadata
    assert "DELTA_BINARY_PACKED" in md.row_group(0).column(0).encodings and "PLAIN" not in md.row_group(0).column(0).encodings
    assert "DELTA_BYTE_ARRAY" in md.row_group(1).column(2).encodings
    t = pq.read_table(path)
    lo = 0
    for cols, present, words, n in groups:
        sl = t.slice(lo, n)
        lo += n
        assert np.array_equal(sl.column("key").to_numpy(), cols["key"])
        qty = sl.column("qty").to_numpy(zero_copy_only=False)
        assert np.array_equal(np.isnan(qty), ~present) and np.array_equal(qty[present].astype(np.int32), cols["qty"][0][present])
        assert [x.encode() for x in sl.column("comment").to_pylist()] == words
        assert np.array_equal(sl.column("price").to_numpy(), cols["price"])
        assert np.array_equal(sl.column("small").to_numpy(), cols["small"])
    got = decode_file(path, decoder=dec)
    assert got["_status"] == 0, got["_error"]
    with oracle.open(path) as of:
        for key, g in got.items():
            if isinstance(key, tuple):
                assert_chunk_equal(g, of.decode(*key), f"writer rg{key[0]} c{key[1]}")
    for rg, (cols, present, words, n) in enumerate(groups):
        assert np.array_equal(np.frombuffer(got[(rg, 0)]["values"].tobytes(), np.int64), cols["key"])
        assert got[(rg, 2)]["chars"].tobytes() == b"".join(words)
