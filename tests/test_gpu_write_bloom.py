"""Split-block Bloom filters hashed and filled on the GPU (pf_encode_column.bloom_bytes, k_enc_bloom).

Every case runs pf_encode_chunk and requires EncodedChunk.bloom_filter() to equal bloom_cases' reference bit for bit:
the reference states the format's rules from the present values alone and test_write_bloom_cpu.py pins it to the bytes
pyarrow writes. A case's hashes are computed once (bloom_cases caches them) and shared by the tests that use it."""
import ctypes as C

import numpy as np
import pytest

import bloom_cases as B
import pagekit as K

pytestmark = pytest.mark.gpu

CODECS = {"snappy": K.SNAPPY, "uncompressed": K.UNCOMPRESSED}


@pytest.fixture(scope="module")
def dec():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _encode(dec, case, bloom_bytes, codec=K.SNAPPY, **kw):
    """pf_encode_chunk of one case -> (EncodedChunk copy, chunk bytes, filter bytes or None)."""
    from pfloor import writer as W
    data, validity = case.row_arrays()
    kw.setdefault("page_rows", case.page_rows)
    out = W.GpuColumnEncoder(dec).encode(W.Field(case.name, case.ptype, case.optional), data, validity, case.rows,
                                         codec=codec, bloom_bytes=bloom_bytes, **kw)
    return W.EncodedChunk.from_buffer_copy(out), C.string_at(out.bytes, out.size), out.bloom_filter()


def _diff(got, want):
    """Where two filters differ, for the assertion message."""
    if got is None or len(got) != len(want):
        return f"length {None if got is None else len(got)} for {len(want)}"
    g, w = np.frombuffer(got, "<u4"), np.frombuffer(want, "<u4")
    bad = np.flatnonzero(g != w)
    return f"{len(bad)} of {len(w)} words differ, first at word {bad[0]}: {g[bad[0]]:#x} for {w[bad[0]]:#x}" if len(bad) else "equal"


def _check(dec, case, nbytes, label="", **kw):
    out, _body, got = _encode(dec, case, nbytes, **kw)
    want = case.filter(nbytes)
    assert got == want, f"{case.name} {label} {nbytes} bytes: {_diff(got, want)}"
    assert out.bloom_len == nbytes
    return out


# ---------------------------------------------------------------- 1. type x route x codec
_ROUTE_ENCODING = {"plain": {K.PLAIN}, "dictionary": {K.RLE_DICTIONARY}, "dict_over_limit": {K.PLAIN},
                   "delta_fallback": {K.DELTA_BINARY_PACKED, K.DELTA_BYTE_ARRAY, K.PLAIN}, "all_bits": {K.RLE_DICTIONARY}}


@pytest.mark.parametrize("codec", list(CODECS))
@pytest.mark.parametrize("route", list(B.ROUTES))
@pytest.mark.parametrize("tname", list(B.TYPES))
def test_type_route_codec(dec, tname, route, codec):
    """The same values give the same filter on every route: PLAIN, dictionary (first occurrences only are hashed),
    a dictionary over the page limit (fallback 1), DELTA_* pages, and all option bits at once; with and without nulls."""
    for nulls in (False, True):
        case = B.typed(tname, nulls)
        out = _check(dec, case, 1024, f"{route} {codec}", codec=CODECS[codec], **B.ROUTES[route])
        assert out.data_encoding in _ROUTE_ENCODING[route], (route, out.data_encoding)   # the route was taken
        assert out.fallback == (1 if route == "dict_over_limit" else 0)
        if route in ("dictionary", "all_bits"):
            assert out.dict_entries == case.distinct()
        if route == "delta_fallback" and tname in ("int32", "int64", "binary"):
            assert out.data_encoding != K.PLAIN


# ---------------------------------------------------------------- 2. filter sizes
@pytest.mark.parametrize("nbytes", B.SIZES)
@pytest.mark.parametrize("tname", ["int64", "binary"])
def test_filter_sizes(dec, tname, nbytes):
    """32 bytes: one block, every value in block 0. 64: two blocks, the smallest size at which a wrong block index
    shows. 1,024. 1 MiB."""
    case = B.typed(tname, True)
    _check(dec, case, nbytes, "plain", dictionary=False)
    _check(dec, case, nbytes, "dictionary", dictionary=True)
    if nbytes == 64:   # both blocks are in use: a block index stuck at 0 would fail
        words = np.frombuffer(case.filter(64), "<u4")
        assert words[:8].any() and words[8:].any()


# ---------------------------------------------------------------- 3. value counts
@pytest.mark.parametrize("nulls", [False, True], ids=["required", "nulls30"])
@pytest.mark.parametrize("n", B.COUNTS)
def test_value_counts(dec, n, nulls):
    """0 rows; 1; around a wave (63 / 64 / 65) and a workgroup (255 / 256 / 257); 4,097; 70,000 (four pages, 274
    workgroups), as distinct INT64 values and as strings (70,000: INT64 only)."""
    case = B.counted(n, nulls)
    _check(dec, case, 4096, "plain", dictionary=False)
    _check(dec, case, 4096, "dictionary", dictionary=True)
    if n == 0:
        assert case.filter(4096) == bytes(4096)
    if n <= 4097:
        strings = B.counted_strings(n, nulls)
        _check(dec, strings, 2048, "plain", dictionary=False)
        _check(dec, strings, 2048, "dictionary", dictionary=True)


# ---------------------------------------------------------------- 4. nulls and repetition
@pytest.mark.parametrize("tname", list(B.TYPES))
def test_all_null_column(dec, tname):
    """No present value: an all-zero filter of the requested size, whatever the null rows hold."""
    case = B.all_null(tname)
    for route in ("plain", "dictionary", "all_bits"):
        _out, _body, got = _encode(dec, case, 256, **B.ROUTES[route])
        assert got == bytes(256), (tname, route)


@pytest.mark.parametrize("tname", ["int32", "double", "binary"])
def test_three_values_twenty_thousand_times(dec, tname):
    case = B.three_values(tname)
    out = _check(dec, case, 64, "dictionary", dictionary=True)
    assert out.dict_entries == 3 and out.data_encoding == K.RLE_DICTIONARY
    _check(dec, case, 64, "plain", dictionary=False)
    assert sum(bin(w).count("1") for w in np.frombuffer(case.filter(64), "<u4")) <= 24   # three values, eight bits each


def test_every_value_route_of_a_dictionary_chunk(switches):
    """A dictionary-encoded chunk's filter is filled from the first occurrences of its values; the
    diagnostics build's PF_BLOOM_FIRST=0 hashes every value instead, as a chunk that is not dictionary-encoded does.
    The same bits either way."""
    from pfloor.decoder import GpuDecoder
    with switches(PF_BLOOM_FIRST=0):
        d = GpuDecoder(0)
        try:
            for case in (B.typed("int32", True), B.typed("binary", True), B.three_values("double")):
                out = _check(d, case, 1024, "every value", dictionary=True)
                assert out.data_encoding == K.RLE_DICTIONARY
        finally:
            d.close()


# ---------------------------------------------------------------- 5. floats
@pytest.mark.parametrize("route", ["plain", "dictionary", "all_bits"])
@pytest.mark.parametrize("tname", ["float", "double"])
def test_float_bits(dec, tname, route):
    """NaNs of both signs and several payloads, +-0.0, +-inf, subnormals: each is a value of its own, hashed as its bits."""
    case = B.float_specials(tname)
    assert case.distinct() == 13
    out = _check(dec, case, 128, route, **B.ROUTES[route])
    if route != "plain":
        assert out.dict_entries == 13


# ---------------------------------------------------------------- 6. strings
@pytest.mark.parametrize("route", ["plain", "dictionary", "delta_fallback"])
@pytest.mark.parametrize("name", ["lengths_0_70", "long_among_short", "bytes_00_ff", "empty_present_and_null", "only_empty"])
def test_strings(dec, name, route):
    """Every length 0..70 (all tail branches, the 32-byte loop's boundaries) at every address alignment; values of 255,
    256, 1,000 and 4,097 bytes among short ones; \\x00 and \\xff; empty strings, present and null."""
    case = B.string_cases()[name]
    _check(dec, case, 512, route, **B.ROUTES[route])
    if name == "only_empty":
        assert case.filter(512) == B.build_filter(np.array([0xEF46DB3751D8E999], np.uint64), 512)


# ---------------------------------------------------------------- 7. inputs in device memory
@pytest.mark.parametrize("tname", ["int64", "binary"])
def test_on_device_inputs(dec, tname):
    """The column's arrays in device memory (pf_device_alloc, pf_memcpy_h2d) and on_device = 1: the same filter and the
    same chunk as from host arrays."""
    from pfloor import writer as W
    L = W.lib()
    case = B.typed(tname, True)
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
        _encode(dec, B.counted(1, False), 0)
        c.dictionary, c.page_rows, c.codec, c.bloom_bytes = 1, case.page_rows, K.SNAPPY, 1024
        out = W.EncodedChunk()
        assert L.pf_encode_chunk(dec.h, C.byref(c), 1, C.byref(out)) == 0, L.pf_last_error(dec.h)
        got, body = out.bloom_filter(), C.string_at(out.bytes, out.size)
    finally:
        for p, _arr in held:
            L.pf_device_free(dec.h, p)
    want = case.filter(1024)
    assert got == want, _diff(got, want)
    assert body == _encode(dec, case, 1024, dictionary=True)[1]


# ---------------------------------------------------------------- 8. the chunk itself is unchanged
_FIELDS = ("size", "total_uncompressed_size", "num_values", "dictionary_page_offset", "data_page_offset", "n_data_pages",
           "dict_entries", "data_encoding", "fallback", "codec", "snappy_in", "snappy_out", "stats_flags", "stat_min_len",
           "stat_max_len", "null_count")


@pytest.mark.parametrize("route", list(B.ROUTES))
@pytest.mark.parametrize("tname", ["int32", "double", "binary"])
def test_chunk_bytes_are_unchanged(dec, tname, route):
    case = B.typed(tname, True)
    off, body_off, f_off = _encode(dec, case, 0, **B.ROUTES[route])
    st_off = off.statistics()
    on, body_on, f_on = _encode(dec, case, 1024, **B.ROUTES[route])
    assert f_off is None and off.bloom_len == 0 and not off.bloom and off.bloom_ms == 0.0
    assert len(f_on) == 1024 and body_on == body_off
    for name in _FIELDS:
        assert getattr(on, name) == getattr(off, name), name
    assert on.statistics() == st_off


# ---------------------------------------------------------------- 9. size validation
def test_size_validation(dec):
    from pfloor import writer as W
    case = B.counted(65, False)
    for bad in (31, 48, 1 << 28, -64):
        with pytest.raises(W.PfError) as e:
            _encode(dec, case, bad)
        assert e.value.code == -1, bad
    _check(dec, case, 32, "after the errors")            # the context is still usable
    flags = np.arange(100, dtype=np.uint8) % 2
    out = W.GpuColumnEncoder(dec).encode(W.Field("b", W.BOOLEAN), flags, None, 100, bloom_bytes=1024)
    assert out.bloom_len == 0 and out.bloom_filter() is None


# ---------------------------------------------------------------- 10. ParquetWriter end to end
def _own_rows(path):
    from pfloor.decoder import decode_file
    got = decode_file(path, device=0)
    assert got["_status"] == 0, got["_error"]
    return got


@pytest.mark.parametrize("parallel", [False, True], ids=["one_context", "two_contexts"])
def test_parquet_writer_end_to_end(dec, tmp_path, parallel):
    """Two row groups, five fields, filters on three: one by ndv, one True (bloom_max_bytes), one {"bytes": 64}. pyarrow
    and our reader read the rows back; each filter blob is the blob pyarrow writes for the same column at the same
    size; every present value is found in its row group's filter through pf_file_chunk_bloom, pf_xxh64 and
    pf_bloom_check."""
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    from pfloor import writer as W
    from pfloor.decoder import GpuDecoder
    L = W.lib()
    rows = (3000, 1097)
    cases = {"id": B.counted(4097, False), "qty": B.typed("int32", True), "price": B.typed("double", True),
             "word": B.typed("binary", True), "note": B.counted_strings(4097, True)}
    schema = W.MessageType("t", W.required(W.INT64).named("id"), W.optional(W.INT32).named("qty"),
                           W.optional(W.DOUBLE).named("price"), W.optional(W.BINARY).as_string().named("word"),
                           W.optional(W.BINARY).as_string().named("note"))
    spec = {"id": 3000, "word": True, "note": {"bytes": 64}}
    want_bytes = {"id": B.optimal_bytes(3000, 0.01), "word": 4096, "note": 64}
    assert want_bytes["id"] == 4096

    def group(name, g):
        """Rows of row group g of a case, as a Case of its own."""
        case, r0 = cases[name], sum(rows[:g])
        sl = slice(r0, r0 + rows[g])
        return B.Case(f"{name}_{g}", case.ptype, case.values[sl], None if case.present is None else case.present[sl])

    path = str(tmp_path / "e2e.parquet")
    second = GpuDecoder(0) if parallel else None
    try:
        w = W.ParquetWriter(schema, path, None, decoder=None if parallel else dec, decoders=[dec, second] if parallel else None,
                            bloom_filters=spec, bloom_fpp=0.01, bloom_max_bytes=4096)
        for g in range(2):
            cols = {}
            for name in cases:
                data, validity = group(name, g).row_arrays()
                cols[name] = data if validity is None else ((data[0], data[1], validity) if isinstance(data, tuple) else (data, validity))
            w.write_columns(cols, rows[g])
        w.close()
    finally:
        if second is not None:
            second.close()
    # rows: pyarrow and our reader
    t = pq.read_table(path)
    got = _own_rows(path)
    names = list(cases)
    for g in range(2):
        for c, name in enumerate(names):
            sub = group(name, g)
            col = t.column(name).slice(sum(rows[:g]), rows[g])
            assert col.to_pylist() == sub.arrow().cast(col.type).to_pylist(), (name, g)
            mine = got[(g, c)]
            pv = sub.present_values()
            if sub.ptype == K.BYTE_ARRAY:
                offs, chars = mine["offsets"], mine["chars"].tobytes()
                valid = np.ones(rows[g], bool) if sub.present is None else sub.present
                assert [chars[offs[i]:offs[i + 1]] for i in range(rows[g]) if valid[i]] == pv, (name, g)
            else:
                vals = np.frombuffer(mine["values"].tobytes(), pv.dtype)
                assert np.array_equal(vals if sub.present is None else vals[sub.present], pv), (name, g)
    # filters: the footer's offsets, pyarrow's own blob, and the host probe
    md = pq.ParquetFile(path).metadata
    f = C.c_void_p()
    assert L.pf_file_open(path.encode(), C.byref(f)) == 0
    last_end = 0
    for g in range(2):
        for c, name in enumerate(names):
            off, ln = C.c_int64(0), C.c_int32(0)
            assert L.pf_file_chunk_bloom(f, g, c, C.byref(off), C.byref(ln)) == 0
            col = md.row_group(g).column(c)
            if name not in spec:
                assert (off.value, ln.value) == (-1, -1) and col.bloom_filter_offset is None
                continue
            sub, nbytes = group(name, g), want_bytes[name]
            assert (off.value, ln.value) == (col.bloom_filter_offset, col.bloom_filter_length)
            assert off.value >= last_end and ln.value == len(B.header(nbytes)) + nbytes
            last_end = off.value + ln.value
            blob = np.zeros(ln.value, np.uint8)
            assert L.pf_file_read(f, off.value, ln.value, blob.ctypes.data) == 0
            blob = blob.tobytes()
            assert blob == B.header(nbytes) + sub.filter(nbytes), (name, g, _diff(blob[-nbytes:], sub.filter(nbytes)))
            ref = str(tmp_path / f"ref_{name}_{g}.parquet")
            opts = B.pyarrow_options(nbytes, sub.distinct())
            pq.write_table(pa.table({name: sub.arrow()}), ref, bloom_filter_options={name: opts})
            rc = pq.ParquetFile(ref).metadata.row_group(0).column(0)
            theirs = open(ref, "rb").read()[rc.bloom_filter_offset:rc.bloom_filter_offset + rc.bloom_filter_length]
            assert blob == theirs, (name, g, opts)
            bits = blob[-nbytes:]
            pv = sub.present_values()
            for v in pv:
                raw = v if sub.ptype == K.BYTE_ARRAY else v.tobytes()
                assert L.pf_bloom_check(bits, nbytes, L.pf_xxh64(raw, len(raw), 0)) == 1, (name, g, v)
    L.pf_file_close(f)
    assert md.row_group(1).column(4).data_page_offset < md.row_group(0).column(0).bloom_filter_offset   # behind the last row group
