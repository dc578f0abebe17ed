"""DELTA_BINARY_PACKED / DELTA_BYTE_ARRAY write path, host side (no GPU).

1. The expected bytes of the GPU tests (test_gpu_write_delta.py) are pagekit's streams of each page's
   present values. Here every case of tests/delta_cases.py is wrapped in hand-built v2 pages and read
   back to its inputs by the CPU oracle and by pyarrow: the expectation is validated by two readers
   that share no code with the encoder.
2. The file writer lists the encodings a chunk uses: a hand-built DELTA_* chunk added through
   pf_writer_add_chunk is read back by pyarrow and the oracle, and its ColumnMetaData.encodings name
   the delta encoding and not PLAIN."""
import ctypes as C

import numpy as np
import pytest

import delta_cases as DC
import pagekit as K
from golden_util import assert_chunk_equal


@pytest.mark.parametrize("fid", DC.FILE_IDS)
def test_expected_streams_read_by_oracle_and_pyarrow(oracle, tmp_path, fid):
    pq = pytest.importorskip("pyarrow.parquet")
    rows, cases = DC.file_cases(fid)
    chunks = []
    for case in cases:
        ch = K.Chunk(case.name, case.ptype, optional=case.optional, layout=K.LAYOUTS["e"])
        for present, vals in case.pages():
            ch.add_page(case.encoding, case.stream(vals), present=present, vals=case.pagekit_vals(vals))
        chunks.append(ch)
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
    t = pq.ParquetFile(path).read_row_group(0)
    assert t.num_rows == rows
    for case in cases:
        assert t.column(case.name).to_pylist() == case.pylist(), f"{fid} {case.name} [pyarrow]"


def _chunk(W, body, n, encoding):
    c = W.EncodedChunk()
    buf = C.create_string_buffer(body, len(body))
    c.bytes = C.cast(buf, C.c_void_p)
    c.size = len(body)
    c.total_uncompressed_size = len(body)
    c.num_values = n
    c.dictionary_page_offset = -1
    c.data_page_offset = 0
    c.n_data_pages = 1
    c.data_encoding = encoding
    c.codec = 0
    return c, buf


def test_writer_footer_lists_delta_encodings(oracle, tmp_path):
    """One uncompressed v2 page per chunk, values sections from pagekit: the footer written by
    pf_writer_* must name DELTA_BINARY_PACKED / DELTA_BYTE_ARRAY (and RLE for the levels), not PLAIN."""
    pq = pytest.importorskip("pyarrow.parquet")
    from pfloor import writer as W
    L = W.lib()
    n = 1000
    ids = DC.int_values("steps", 64, n)
    present = (np.arange(n) % 4) != 0
    vals = DC.int_values("outlier", 32, int(present.sum()))
    words = DC.string_values("sorted", n)
    groups = (n + 7) // 8
    defl = K._uvarint((groups << 1) | 1) + np.packbits(present, bitorder="little").tobytes()
    sa = K.dbp([int(v) for v in ids], bits=64)
    sb = K.dbp([int(v) for v in vals], bits=32)
    sc = K.delta_byte_array(words)
    bodies = [
        K.v2_page_header(n, 0, n, K.DELTA_BINARY_PACKED, 0, 0, False, len(sa), len(sa)) + sa,
        K.v2_page_header(n, int((~present).sum()), n, K.DELTA_BINARY_PACKED, len(defl), 0, False,
                         len(defl) + len(sb), len(defl) + len(sb)) + defl + sb,
        K.v2_page_header(n, 0, n, K.DELTA_BYTE_ARRAY, 0, 0, False, len(sc), len(sc)) + sc,
    ]
    encs = [K.DELTA_BINARY_PACKED, K.DELTA_BINARY_PACKED, K.DELTA_BYTE_ARRAY]
    fields = (W.WriteField * 3)(W.WriteField(b"id", W.INT64, 0, 0), W.WriteField(b"v", W.INT32, 1, 0),
                                W.WriteField(b"w", W.BINARY, 0, 0))
    path = str(tmp_path / "delta.parquet")
    w = C.c_void_p()
    assert L.pf_writer_open(path.encode(), fields, 3, C.byref(w)) == 0
    keep = []
    for i, (body, enc) in enumerate(zip(bodies, encs)):
        c, buf = _chunk(W, body, n, enc)
        keep.append(buf)
        assert L.pf_writer_add_chunk(w, i, C.byref(c)) == 0
    assert L.pf_writer_end_row_group(w, n) == 0
    assert L.pf_writer_close(w) == 0
    pf = pq.ParquetFile(path)
    names = {K.DELTA_BINARY_PACKED: "DELTA_BINARY_PACKED", K.DELTA_BYTE_ARRAY: "DELTA_BYTE_ARRAY"}
    for i, enc in enumerate(encs):
        listed = pf.metadata.row_group(0).column(i).encodings
        assert names[enc] in listed and "RLE" in listed and "PLAIN" not in listed, (i, listed)
    t = pf.read()
    assert np.array_equal(t.column("id").to_numpy(), ids)
    got = t.column("v").to_pylist()
    assert [g is not None for g in got] == list(present)
    assert [g for g in got if g is not None] == vals.tolist()
    assert t.column("w").to_pylist() == words
    with oracle.open(path) as of:
        a, b, c = of.decode(0, 0), of.decode(0, 1), of.decode(0, 2)
        assert a["status"] == 0 and b["status"] == 0 and c["status"] == 0, (a["error"], b["error"], c["error"])
        assert np.array_equal(np.frombuffer(a["values"].tobytes(), np.int64), ids)
        assert np.array_equal(np.frombuffer(b["values"].tobytes(), np.int32)[present], vals)
        assert c["chars"].tobytes() == b"".join(words)
