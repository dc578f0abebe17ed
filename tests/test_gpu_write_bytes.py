"""The default write route byte for byte: what pf_encode_chunk writes with no opt-in bit (k_enc_flags, k_enc_compact,
k_enc_heads, k_enc_mark, k_enc_ids, k_enc_pages on its bit-packed-run and PLAIN branches, the host's page assembly,
k_snappy_compress), against tests/write_cases.py.

The expected bytes of every page are stated from its inputs alone (write_cases.Case.plan; test_write_cases_cpu.py
reads them back with the oracle and pyarrow). A round trip cannot see a wrong id width, garbage in the padding of a
page's last group, values under nulls in the dictionary or a dictionary in another order; equal bytes can.
 1. UNCOMPRESSED chunks equal the reference page by page, header fields included; SNAPPY chunks hold the same
    bytes behind k_snappy_compress, whose streams keep the compressor's grammar (snappy_tokens.compressor_errors).
 2. The files are read back by pyarrow, the oracle and the GPU reader; on the GPU reader no Snappy job leaves the
    block-parallel path (FB_REDO, FB_SERIAL), and the literal-only codes of k_snappy_head (FB_INPLACE, FB_LITCOPY)
    sit on exactly the pages whose streams are literals.
 3. Inputs in device memory give the chunk host inputs give; ParquetWriter without a keyword is this route.
One file per row count holds every case of that count (write_cases.file_cases), written once per codec."""
import ctypes as C

import numpy as np
import pytest

import pagekit as K
import snappy_tokens as T
import write_cases as WC
from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

FB_OK, FB_WHOLE, FB_REDO, FB_SERIAL, FB_INPLACE, FB_LITCOPY = range(6)     # pf_snappy_par.h
LC_MAX = 32
CODECS = {"uncompressed": K.UNCOMPRESSED, "snappy": K.SNAPPY}


@pytest.fixture(scope="module")
def dec():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _settings(case):
    return {"dictionary": case.dictionary, "page_rows": case.page_rows, "dict_page_limit": case.dict_page_limit}


def _encode(dec, case, codec):
    """pf_encode_chunk of one case -> (chunk bytes, EncodedChunk copy)."""
    from pfloor import writer as W
    data, validity = case.row_arrays()
    out = W.GpuColumnEncoder(dec).encode(W.Field(case.name, case.ptype, case.optional), data, validity, case.rows,
                                         codec=codec, **_settings(case))
    return C.string_at(out.bytes, out.size), W.EncodedChunk.from_buffer_copy(out)


def _write(dec, path, rows, cases, codec):
    """The cases as one row group of a file -> [(chunk bytes, EncodedChunk copy)]."""
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
        out = enc.encode(W.Field(case.name, case.ptype, case.optional), data, validity, rows, codec=codec, **_settings(case))
        chunks.append((C.string_at(out.bytes, out.size), W.EncodedChunk.from_buffer_copy(out)))
        assert L.pf_writer_add_chunk(w, i, C.byref(out)) == 0
    assert L.pf_writer_end_row_group(w, rows) == 0
    assert L.pf_writer_close(w) == 0
    return chunks


@pytest.fixture(scope="module")
def written(dec, tmp_path_factory):
    """written(fid, codec) -> (path, chunks); each file once."""
    root = tmp_path_factory.mktemp("write_bytes")
    cache = {}

    def get(fid, codec):
        if (fid, codec) not in cache:
            rows, cases = WC.file_cases(fid)
            path = str(root / f"{fid}_{codec}.parquet")
            cache[(fid, codec)] = (path, _write(dec, path, rows, cases, codec))
        return cache[(fid, codec)]
    return get


def _diff(got, exp, label):
    if got == exp:
        return []
    g, e = np.frombuffer(got, np.uint8), np.frombuffer(exp, np.uint8)
    m = min(len(g), len(e))
    bad = np.flatnonzero(g[:m] != e[:m])
    at = int(bad[0]) if len(bad) else m
    return [f"{label}: {len(g)} bytes for {len(e)}, first difference at {at}: {got[at:at + 8].hex()} for {exp[at:at + 8].hex()}"]


def chunk_errors(case, raw, c, codec, oracle):
    """What is wrong with an encoded chunk: its pages and header fields against case.plan()."""
    p = case.plan()
    errs = []

    def same(what, got, exp):
        if got != exp:
            errs.append(f"{what}: {got} for {exp}")

    D = 0 if p["dict"] is None else len(p["dict"])
    pages = WC.read_pages(raw)
    same("size", c.size, len(raw))
    same("num_values", c.num_values, case.rows)
    same("n_data_pages", c.n_data_pages, len(p["pages"]))
    same("dict_entries", c.dict_entries, D)
    same("data_encoding", c.data_encoding, p["encoding"])
    same("fallback", c.fallback, p["fallback"])
    same("codec", c.codec, codec)
    same("dictionary_page_offset", c.dictionary_page_offset, 0 if D else -1)
    same("total_uncompressed_size", c.total_uncompressed_size, sum(g["header_len"] + g["usize"] for g in pages))

    def stored(body, usize, what):
        """The bytes a stored values / dictionary section stands for."""
        if codec != K.SNAPPY:
            return body
        errs.extend(f"{what}: {e}" for e in T.compressor_errors(body, usize)[:3])
        out = oracle.snappy_uncompress(body)
        return out if isinstance(out, bytes) else b""

    if D:
        d = pages.pop(0)
        same("dictionary page (type, num_values, encoding, uncompressed_size, crc)",
             (d["type"], d["num_values"], d["encoding"], d["usize"], d["crc"]), (WC.PAGE_DICTIONARY, D, K.PLAIN, len(p["dict_bytes"]), None))
        errs += _diff(stored(d["body"], d["usize"], "dictionary page"), p["dict_bytes"], "dictionary page")
        same("data_page_offset", c.data_page_offset, d["header_len"] + d["csize"])
    else:
        same("data_page_offset", c.data_page_offset, 0)
    same("data pages", len(pages), len(p["pages"]))
    for k, (got, exp) in enumerate(zip(pages, p["pages"])):
        label = f"page {k}"
        if got["type"] != WC.PAGE_DATA_V2:
            errs.append(f"{label}: page type {got['type']}")
            continue
        fields = ("num_values", "num_nulls", "num_rows", "encoding", "def_bytes", "rep_bytes", "usize", "is_compressed", "crc", "statistics")
        same(f"{label} {fields}", tuple(got[f] for f in fields),
             (exp["rows"], exp["nulls"], exp["rows"], p["encoding"], len(exp["levels"]), 0, len(exp["levels"]) + len(exp["values"]),
              codec == K.SNAPPY, None, None))
        db = len(exp["levels"])
        errs += _diff(got["body"][:db], exp["levels"], label + " levels")
        errs += _diff(stored(got["body"][db:], len(exp["values"]), label + " values"), exp["values"], label + " values")
    return errs


# ---------------------------------------------------------------- 1. exact bytes
@pytest.mark.parametrize("codec", list(CODECS))
@pytest.mark.parametrize("fid", WC.FILE_IDS)
def test_exact_bytes(dec, oracle, written, fid, codec):
    _path, chunks = written(fid, CODECS[codec])
    _rows, cases = WC.file_cases(fid)
    wrong = []
    for case, (raw, c) in zip(cases, chunks):
        wrong += [f"{fid} {case.name}: {e}" for e in chunk_errors(case, raw, c, CODECS[codec], oracle)[:6]]
    assert not wrong, f"{len(wrong)} differences\n" + "\n".join(wrong[:60])


def test_fallbacks_and_widths_of_the_cases(written):
    """What the cases are there for did happen: ids of every width 1..20, and all four fallback codes but the
    string-hash collision."""
    widths, fallbacks = set(), set()
    for fid in WC.FILE_IDS:
        _path, chunks = written(fid, K.UNCOMPRESSED)
        for case, (raw, c) in zip(WC.file_cases(fid)[1], chunks):
            fallbacks.add(c.fallback)
            if c.data_encoding == K.RLE_DICTIONARY:
                first = [g for g in WC.read_pages(raw) if g["type"] == WC.PAGE_DATA_V2][0]
                widths.add(first["body"][first["def_bytes"]])
    assert widths == set(range(1, 21)) and fallbacks == {0, 1, 3}


# ---------------------------------------------------------------- 2. round trip
def _snappy_jobs(dec):
    """[[fallback, src_len, dst_len, chunk, page]] per Snappy job of the last decode."""
    from pfloor import _native
    L = _native.lib()
    L.pf_debug_snappy_fallback.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    nj = L.pf_debug_snappy_fallback(dec.h, None, 0)
    rec = (C.c_int * (5 * max(nj, 1)))()
    assert L.pf_debug_snappy_fallback(dec.h, rec, nj) == nj
    return [list(rec[5 * j:5 * j + 5]) for j in range(nj)]


def _expected_codes(stream, is_dict):
    """The pf_debug_snappy_fallback codes k_snappy_head (pf_snappy_head.hip) may leave on a page with this stream:
    a data page that is one literal is read in place; a stream of 1..LC_MAX literals and nothing else is copied by
    k_snappy_litcopy (a dictionary page always, a data page because it did not compress); anything else goes
    through the parse and the block-parallel executor (0, or 1 when it wrote into the column)."""
    _n, toks = T.parse(stream)
    literals = bool(toks) and all(t[0] == T.LITERAL for t in toks)
    if literals and len(toks) == 1 and not is_dict:
        return {FB_INPLACE}
    if literals and len(toks) <= LC_MAX:
        return {FB_LITCOPY}
    return {FB_OK, FB_WHOLE}


@pytest.mark.parametrize("codec", list(CODECS))
@pytest.mark.parametrize("fid", [f for f in WC.FILE_IDS if f != "r0"])
def test_round_trip(dec, oracle, written, fid, codec):
    """pyarrow, the oracle and the GPU reader return the inputs: values bit for bit and validity."""
    pq = pytest.importorskip("pyarrow.parquet")
    from pfloor.decoder import decode_file
    path, chunks = written(fid, CODECS[codec])
    rows, cases = WC.file_cases(fid)
    with oracle.open(path) as of:          # the CPU readers first: the GPU reader is not handed a file they refuse
        for col, case in enumerate(cases):
            o = of.decode(0, col)
            assert o["status"] == 0, (fid, case.name, o["error"])
            assert_chunk_equal(o, case.expected(), f"{fid} {case.name} [oracle]")
    got = decode_file(path, decoder=dec)
    assert got["_status"] == 0, got["_error"]
    jobs = _snappy_jobs(dec) if codec == "snappy" else []
    for col, case in enumerate(cases):
        assert_chunk_equal(got[(0, col)], case.expected(), f"{fid} {case.name} [GPU reader]")
    t = pq.ParquetFile(path).read_row_group(0)
    assert t.num_rows == rows
    for case in cases:
        case.check_arrow(t.column(case.name), f"{fid} {case.name} [pyarrow]")
    if codec != "snappy":
        return
    # the read path of every compressed page: which codes its stream allows
    allowed = {}
    for col, (raw, _c) in enumerate(chunks):
        for g in WC.read_pages(raw):
            db = g.get("def_bytes", 0)
            key = (col, g["csize"] - db, g["usize"] - db)
            allowed.setdefault(key, set()).update(_expected_codes(g["body"][db:], g["type"] == WC.PAGE_DICTIONARY))
    assert len(jobs) == sum(len(WC.read_pages(raw)) for raw, _c in chunks)
    wrong = [(cases[ck].name, fb, src, dst) for fb, src, dst, ck, _pg in jobs if fb not in allowed.get((ck, src, dst), set())]
    assert not wrong, f"pf_debug_snappy_fallback (case, code, compressed, uncompressed): {wrong[:20]}"
    assert not [j for j in jobs if j[0] in (FB_REDO, FB_SERIAL)]


# ---------------------------------------------------------------- 3. device inputs, the writer's default
@pytest.mark.parametrize("name", ["i64_dict_nulls30", "ba_dict_nulls30"])
def test_on_device_inputs(dec, oracle, name):
    """The column's arrays in device memory (pf_device_alloc, pf_memcpy_h2d) and on_device = 1: the chunk host arrays give."""
    from pfloor import writer as W
    L = W.lib()
    case = next(c for c in WC.file_cases(f"r{WC.N_ROWS}")[1] if c.name == name)
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
    c.physical_type, c.max_def, c.num_rows = case.ptype, 1, case.rows
    try:
        c.validity = upload(validity)
        if case.ptype == K.BYTE_ARRAY:
            c.offsets, c.chars, c.chars_len = upload(data[0]), upload(data[1]), data[1].size
        else:
            c.values = upload(data)
        # the uploads are asynchronous on the context's stream; an encode ends with the stream synchronised
        want, _c = _encode(dec, case, K.SNAPPY)
        c.dictionary, c.page_rows, c.codec = 1, case.page_rows, K.SNAPPY
        out = W.EncodedChunk()
        assert L.pf_encode_chunk(dec.h, C.byref(c), 1, C.byref(out)) == 0, L.pf_last_error(dec.h)
        got = C.string_at(out.bytes, out.size)
    finally:
        for p, _arr in held:
            L.pf_device_free(dec.h, p)
    assert got == want
    assert not chunk_errors(case, got, out, K.SNAPPY, oracle)


def test_parquet_writer_without_a_keyword_is_this_route(dec, tmp_path):
    """ParquetWriter(schema, path, None) -- SNAPPY, 20,000-row pages, 1 MiB dictionary limit -- writes the chunks
    pf_encode_chunk gives for the same columns, whose bytes test_exact_bytes pins."""
    from pfloor import writer as W
    from pfloor.decoder import ParquetFile
    cases = [c for c in WC.file_cases(f"r{WC.N_ROWS}")[1] if c.name in ("i32_pagerows0", "ba_pagerows0")]
    assert len(cases) == 2 and all(c.page_rows == 0 and c.dict_page_limit == 0 and c.dictionary for c in cases)
    sch = W.MessageType("m", *[W.Field(c.name, c.ptype, True) for c in cases])
    path = str(tmp_path / "default.parquet")
    cols = {}
    for c in cases:
        data, validity = c.row_arrays()
        cols[c.name] = (data[0], data[1], validity) if c.ptype == K.BYTE_ARRAY else (data, validity)
    w = W.ParquetWriter(sch, path, None, decoder=dec)
    w.write_columns(cols, WC.N_ROWS)
    w.close()
    with open(path, "rb") as f:
        blob = f.read()
    with ParquetFile(path) as pf:
        ranges = [pf.chunk_range(0, i) for i in range(len(cases))]
    for c, (start, size) in zip(cases, ranges):
        assert blob[start:start + size] == _encode(dec, c, K.SNAPPY)[0], c.name
