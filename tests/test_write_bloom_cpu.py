"""Split-block Bloom filters of the write path, host side (no GPU): the reference of the GPU tests (bloom_cases.py) pinned
to the bytes pyarrow writes, the host hash and probe (pf_xxh64, pf_bloom_check: the kernel's arithmetic, one header),
the size formula, the file writer on hand-built chunks and the read side (pf_file_chunk_bloom)."""
import ctypes as C
import struct

import numpy as np
import pytest

import bloom_cases as B
import pagekit as K
import stats_cases as S


@pytest.fixture(scope="module")
def W():
    from pfloor import writer
    writer.lib()
    return writer


def _pyarrow_blobs(path, n_cols):
    """[(offset, length, bytes)] of row group 0's filters as pyarrow's metadata locates them."""
    import pyarrow.parquet as pq
    md = pq.ParquetFile(path).metadata
    raw = open(path, "rb").read()
    out = []
    for c in range(n_cols):
        col = md.row_group(0).column(c)
        off, ln = col.bloom_filter_offset, col.bloom_filter_length
        out.append((off, ln, raw[off:off + ln] if off is not None and ln is not None else None))
    return out


# ---------------------------------------------------------------- 1. the reference against pyarrow's writer
_PINNED = [("int32", False), ("int32", True), ("int64", False), ("int64", True), ("float", False), ("float", True),
           ("double", False), ("double", True), ("binary", False), ("binary", True)]


@pytest.mark.parametrize("tname,nulls", _PINNED, ids=[f"{t}{'_nulls' if n else ''}" for t, n in _PINNED])
def test_reference_is_what_pyarrow_writes(tmp_path, tname, nulls):
    """pyarrow's filter bytes (header and bitset, cut by bloom_filter_offset / bloom_filter_length) are the reference's,
    for every type with and without nulls; the columns hold 600 distinct values in 5,000 rows, so pyarrow writes them
    dictionary-encoded, and the specials of FLOAT / DOUBLE ride along."""
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    cases = [B.typed(tname, nulls)]
    if tname in ("float", "double"):
        cases.append(B.float_specials(tname))
    for case in cases:
        nbytes = case.pyarrow_bytes(case.rows, 0.01)
        path = str(tmp_path / f"{case.name}.parquet")
        pq.write_table(pa.table({"c": case.arrow()}), path, bloom_filter_options={"c": {"ndv": case.rows, "fpp": 0.01}})
        (off, ln, blob), = _pyarrow_blobs(path, 1)
        assert blob == B.header(nbytes) + case.filter(nbytes), f"{case.name}: {ln} bytes at {off}"


def test_reference_plain_and_strings_against_pyarrow(tmp_path):
    """The same for PLAIN pages (use_dictionary=False) and for the string cases: every length 0..70, long values,
    arbitrary bytes, empty strings."""
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    cases = [B.counted(4097, True), B.counted_strings(257, True)] + list(B.string_cases().values())
    for case in cases:
        nbytes = case.pyarrow_bytes(case.rows, 0.05)
        path = str(tmp_path / f"{case.name}.parquet")
        pq.write_table(pa.table({"c": case.arrow()}), path, use_dictionary=False,
                       bloom_filter_options={"c": {"ndv": case.rows, "fpp": 0.05}})
        (_off, _ln, blob), = _pyarrow_blobs(path, 1)
        assert blob == B.header(nbytes) + case.filter(nbytes), case.name


def test_reference_probe():
    case = B.counted(4097, False)
    bits = case.filter(1024)
    assert all(B.might_contain(bits, int(h)) for h in case.hashes())
    assert not B.might_contain(bytes(1024), int(case.hashes()[0]))


# ---------------------------------------------------------------- 2. the size formula
_NDV = (1, 10, 1000, 5000, 10 ** 5, 10 ** 6)
_FPP = (0.001, 0.01, 0.05, 0.5)


@pytest.mark.parametrize("ndv", _NDV)
def test_optimal_bytes_is_pyarrows_choice(W, tmp_path, ndv):
    """bloom_optimal_bytes(ndv, fpp) is the numBytes pyarrow writes, for every ndv x fpp of the table: all 24 pairs,
    none dropped.

    The column has `ndv` distinct rows, not the 100 or fewer one would like: pyarrow 25 sizes the filter for
    min(ndv, distinct values of the chunk) -- 50 rows with ndv = 5,000, fpp = 0.01 give 64 bytes, 5,000 distinct rows
    give 8,192 -- so only a column of at least ndv distinct values shows what the options alone choose. The cap is
    128 MiB on both sides."""
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    col = pa.array(np.arange(ndv, dtype=np.int32))
    for fpp in _FPP:
        path = str(tmp_path / f"s_{fpp}.parquet")
        pq.write_table(pa.table({"c": col}), path, bloom_filter_options={"c": {"ndv": ndv, "fpp": fpp}})
        (_off, ln, blob), = _pyarrow_blobs(path, 1)
        got = W.bloom_optimal_bytes(ndv, fpp, 128 << 20)
        assert blob[:ln - got] == B.header(got) and len(blob) == len(B.header(got)) + got, (ndv, fpp, got, ln)
        assert got == B.optimal_bytes(ndv, fpp)


def test_optimal_bytes_bounds(W):
    assert W.bloom_optimal_bytes(5000, 0.01) == 8192 and W.bloom_optimal_bytes(1000, 0.01) == 2048
    assert W.bloom_optimal_bytes(0, 0.01) == 32 and W.bloom_optimal_bytes(1, 0.5) == 32
    assert W.bloom_optimal_bytes(10 ** 6, 0.01) == 1 << 20            # the default cap, parquet.bloom.filter.max.bytes
    assert W.bloom_optimal_bytes(10 ** 6, 0.01, 1 << 22) == 1 << 21
    assert W.bloom_optimal_bytes(10 ** 6, 0.01, 100000) == 65536     # a cap that is no power of two: rounded down
    assert W.bloom_optimal_bytes(10 ** 12, 0.001, 1 << 40) == 128 << 20
    for bad in (dict(ndv=10, fpp=0.0), dict(ndv=10, fpp=1.0), dict(ndv=-1, fpp=0.1), dict(ndv=1, fpp=0.1, max_bytes=16)):
        with pytest.raises(ValueError):
            W.bloom_optimal_bytes(**bad)


# ---------------------------------------------------------------- 3. pf_xxh64, pf_bloom_check
def test_pf_xxh64_is_the_reference(W):
    """Every length 0..100 and 255, 256, 257, 1000, 4097 at source alignments 0..7, seeds 0 and one other."""
    L = W.lib()
    rng = np.random.default_rng(5)
    lengths = list(range(101)) + [255, 256, 257, 1000, 4097]
    raw = np.zeros(4097 + 64, np.uint8)
    base = raw.ctypes.data
    lead = (-base) % 8                                   # raw[lead] is 8-byte aligned
    want = {}
    for align in range(8):
        payload = rng.integers(0, 256, 4097, dtype=np.uint8)
        raw[lead + align:lead + align + 4097] = payload
        data = payload.tobytes()
        for n in lengths:
            for seed in (0, 0x0123456789ABCDEF):
                ref = want.setdefault((align, n, seed), B.xxh64(data[:n], seed))
                assert (base + lead + align) % 8 == align
                assert L.pf_xxh64(base + lead + align, n, seed) == ref, (align, n, seed)
    assert L.pf_xxh64(None, 0, 0) == 0xEF46DB3751D8E999
    assert L.pf_xxh64(b"abc", 3, 0) == 0x44BC2CF5AD770999


def test_pf_xxh64_fixed_width_keys(W):
    """The 4- and 8-byte inputs the kernel hashes in closed form: the general function gives the vectorised reference."""
    L = W.lib()
    for case in (B.typed("int32"), B.typed("double"), B.float_specials("float"), B.float_specials("double")):
        vals = case.present_values()
        got = [L.pf_xxh64(vals[i:i + 1].tobytes(), vals.dtype.itemsize, 0) for i in range(0, len(vals), 7)]
        assert got == [int(h) for h in case.hashes()[::7]], case.name


def test_pf_bloom_check(W):
    L = W.lib()
    case = B.counted(4097, False)
    for nbytes in (32, 64, 1024):                        # 32: a single block
        bits = case.filter(nbytes)
        assert all(L.pf_bloom_check(bits, nbytes, int(h)) == 1 for h in case.hashes())
        empty = bytes(nbytes)
        assert all(L.pf_bloom_check(empty, nbytes, int(h)) == 0 for h in case.hashes()[:50])
    few = B.counted(63, False)
    bits = few.filter(1 << 20)
    assert all(L.pf_bloom_check(bits, 1 << 20, int(h)) == 1 for h in few.hashes())
    absent = [int(h) for h in case.hashes() if not B.might_contain(bits, int(h))]
    assert len(absent) > 4000 and all(L.pf_bloom_check(bits, 1 << 20, h) == 0 for h in absent)
    one_short = bytearray(case.filter(64))               # one cleared bit of a value's eight: not found
    h0 = int(case.hashes()[0])
    blk = (((h0 >> 32) * 2) >> 32) * 32
    bit = (((h0 & 0xffffffff) * B.SALT[5]) & 0xffffffff) >> 27
    word = struct.unpack_from("<I", one_short, blk + 20)[0] & ~(1 << bit)
    struct.pack_into("<I", one_short, blk + 20, word)
    assert L.pf_bloom_check(bytes(one_short), 64, h0) == 0
    for bad in (0, 31, 48, 96):
        assert L.pf_bloom_check(bytes(128), bad, h0) == -1, bad
    assert L.pf_bloom_check(None, 64, h0) == -1


# ---------------------------------------------------------------- 4. the file writer and the read side
def _chunk(W, body, n, bloom=None):
    c = W.EncodedChunk()
    keep = [C.create_string_buffer(body, len(body))]
    c.bytes = C.cast(keep[0], C.c_void_p)
    c.size = c.total_uncompressed_size = len(body)
    c.num_values = n
    c.dictionary_page_offset = -1
    c.data_page_offset = 0
    c.n_data_pages = 1
    if bloom is not None:
        keep.append(C.create_string_buffer(bloom, len(bloom)))
        c.bloom = C.cast(keep[1], C.c_void_p)
        c.bloom_len = len(bloom)
    return c, keep


def _groups():
    """Two row groups x three REQUIRED fields (INT64, DOUBLE, BYTE_ARRAY), one uncompressed v2 PLAIN page each; the
    DOUBLE field has no filter. -> [[(page bytes, rows, filter bytes or None)]]"""
    out = []
    for g, n in enumerate((1000, 700)):
        ids = np.arange(n, dtype=np.int64) * 3 - 700 + 10 ** 6 * g
        prices = np.arange(n) * 0.25 - 10.0 * g
        words = [b"w%d-%d" % (g, k % 97) for k in range(n)]
        vals = [ids.tobytes(), prices.tobytes(), b"".join(struct.pack("<I", len(w)) + w for w in words)]
        filters = [B.build_filter(B.hashes_fixed(ids), 2048 >> g), None, B.build_filter(B.hashes_bytes(words), 64 << g)]
        out.append([(S.w_page_header_v2(n, 0, 0, 0, len(v)) + v, n, f) for v, f in zip(vals, filters)])
    return out


def _write_groups(W, path, groups, with_filters):
    L = W.lib()
    fields = (W.WriteField * 3)(W.WriteField(b"id", K.INT64, 0, 0), W.WriteField(b"price", K.DOUBLE, 0, 0),
                                W.WriteField(b"word", K.BYTE_ARRAY, 0, 1))
    w = C.c_void_p()
    assert L.pf_writer_open(path.encode(), fields, 3, C.byref(w)) == 0
    for chunks in groups:
        for i, (body, n, flt) in enumerate(chunks):
            c, _keep = _chunk(W, body, n, flt if with_filters else None)
            assert L.pf_writer_add_chunk(w, i, C.byref(c)) == 0, L.pf_writer_last_error()
        assert L.pf_writer_end_row_group(w, chunks[0][1]) == 0
    assert L.pf_writer_close(w) == 0, L.pf_writer_last_error()


def _chunk_bloom(W, f, rg, col):
    off, ln = C.c_int64(7), C.c_int32(7)
    rc = W.lib().pf_file_chunk_bloom(f, rg, col, C.byref(off), C.byref(ln))
    return rc, off.value, ln.value


def test_writer_places_filters_behind_the_row_groups(W, tmp_path):
    pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    L = W.lib()
    groups = _groups()
    path, bare = str(tmp_path / "f.parquet"), str(tmp_path / "bare.parquet")
    _write_groups(W, path, groups, True)
    _write_groups(W, bare, groups, False)
    raw, raw_bare = open(path, "rb").read(), open(bare, "rb").read()
    md = pq.ParquetFile(path).metadata
    pages_end = 4 + sum(len(body) for chunks in groups for body, _n, _f in chunks)
    foot_len = struct.unpack("<I", raw[-8:-4])[0]
    foot_at = len(raw) - 8 - foot_len
    f = C.c_void_p()
    assert L.pf_file_open(path.encode(), C.byref(f)) == 0
    cursor = pages_end                                   # the filters: back to back, row group then column order
    for g, chunks in enumerate(groups):
        for c, (_body, _n, flt) in enumerate(chunks):
            col = md.row_group(g).column(c)
            if flt is None:
                assert col.bloom_filter_offset is None and col.bloom_filter_length is None
                assert _chunk_bloom(W, f, g, c) == (0, -1, -1)
                continue
            blob = B.header(len(flt)) + flt
            assert (col.bloom_filter_offset, col.bloom_filter_length) == (cursor, len(blob)), (g, c)
            assert raw[cursor:cursor + len(blob)] == blob, (g, c)
            assert _chunk_bloom(W, f, g, c) == (0, cursor, len(blob))
            cursor += len(blob)
    assert cursor == foot_at                             # between the last page and the footer, nothing else
    assert _chunk_bloom(W, f, 2, 0)[0] == -1 and _chunk_bloom(W, f, 0, 3)[0] == -1
    assert L.pf_file_chunk_bloom(f, 0, 0, None, None) == -1
    L.pf_file_close(f)
    # without filters: the same pages, then the footer at once
    assert raw[:pages_end] == raw_bare[:pages_end]
    assert len(raw_bare) - 8 - struct.unpack("<I", raw_bare[-8:-4])[0] == pages_end
    fm, fm_bare = S.footer(path), S.footer(bare)
    for g in range(2):
        for c in range(3):
            with_f = dict(fm[4][g][1][c][3])
            assert (14 in with_f) == (groups[g][c][2] is not None) and 14 not in fm_bare[4][g][1][c][3]
            with_f.pop(14, None)
            with_f.pop(15, None)
            assert with_f == fm_bare[4][g][1][c][3]
    t, t_bare = pq.read_table(path), pq.read_table(bare)
    assert t.equals(t_bare) and t.num_rows == 1700
    f2 = C.c_void_p()
    assert L.pf_file_open(bare.encode(), C.byref(f2)) == 0
    assert all(_chunk_bloom(W, f2, g, c) == (0, -1, -1) for g in range(2) for c in range(3))
    L.pf_file_close(f2)


def test_chunk_bloom_on_a_pyarrow_file(W, tmp_path):
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    L = W.lib()
    a, b = B.typed("int64"), B.typed("binary", True)
    path = str(tmp_path / "pa.parquet")
    pq.write_table(pa.table({"a": a.arrow(), "plain": a.arrow(), "b": b.arrow()}), path, row_group_size=2500,
                   bloom_filter_options={"a": {"ndv": 2500, "fpp": 0.05}, "b": {"ndv": 300, "fpp": 0.01}})
    md = pq.ParquetFile(path).metadata
    f = C.c_void_p()
    assert L.pf_file_open(path.encode(), C.byref(f)) == 0
    assert md.num_row_groups == 2
    for g in range(2):
        for c in range(3):
            col = md.row_group(g).column(c)
            if c == 1:
                assert _chunk_bloom(W, f, g, c) == (0, -1, -1)
                continue
            rc, off, ln = _chunk_bloom(W, f, g, c)
            assert (rc, off, ln) == (0, col.bloom_filter_offset, col.bloom_filter_length)
            blob = np.zeros(ln, np.uint8)
            assert L.pf_file_read(f, off, ln, blob.ctypes.data) == 0
            case = a if c == 0 else b
            rows = slice(2500 * g, 2500 * (g + 1))
            if c == 0:
                hs = B.hashes_fixed(case.values[rows])
            else:
                hs = B.hashes_bytes([v for v, p in zip(case.values[rows], case.present[rows]) if p])
            nbytes = B.optimal_bytes(min(2500 if c == 0 else 300, len(np.unique(hs))), 0.05 if c == 0 else 0.01)
            hdr = B.header(nbytes)
            assert blob.tobytes()[:len(hdr)] == hdr and ln == len(hdr) + nbytes
            bits = blob.tobytes()[len(hdr):]
            assert bits == B.build_filter(hs, nbytes)
            assert all(L.pf_bloom_check(bits, nbytes, int(h)) == 1 for h in hs[::11])
    L.pf_file_close(f)


def test_chunk_bloom_outside_the_file_is_an_error(W, tmp_path):
    """A footer whose bloom_filter_offset or bloom_filter_length points outside the file: PF_ERR_IO, as
    pf_file_chunk_range gives for a chunk outside the file. A footer without field 15 (parquet-mr 1.12.2): length -1."""
    L = W.lib()
    groups = _groups()
    path = str(tmp_path / "f.parquet")
    _write_groups(W, path, groups, True)
    raw = open(path, "rb").read()
    foot_len = struct.unpack("<I", raw[-8:-4])[0]
    foot = raw[-8 - foot_len:-8]
    blob_len = len(B.header(2048)) + 2048
    off = 4 + sum(len(body) for chunks in groups for body, _n, _f in chunks)
    # ColumnMetaData of chunk (0, 0) ends ... 9 data_page_offset, 14 (delta 5, i64), 15 (delta 1, i32)
    fields = b"\x56" + S.w_zz(off) + b"\x15" + S.w_zz(blob_len)
    assert foot.count(fields) == 1

    def variant(name, new_fields):
        p = str(tmp_path / name)
        nf = foot.replace(fields, new_fields)
        open(p, "wb").write(raw[:-8 - foot_len] + nf + struct.pack("<I", len(nf)) + b"PAR1")
        f = C.c_void_p()
        assert L.pf_file_open(p.encode(), C.byref(f)) == 0
        got = _chunk_bloom(W, f, 0, 0)
        rest = _chunk_bloom(W, f, 0, 2)
        L.pf_file_close(f)
        assert rest[0] == 0 and rest[1] > 0              # the neighbours are not affected
        return got

    assert variant("same.parquet", fields) == (0, off, blob_len)
    assert variant("no15.parquet", b"\x56" + S.w_zz(off)) == (0, off, -1)
    assert variant("far.parquet", b"\x56" + S.w_zz(len(raw) + 5) + b"\x15" + S.w_zz(blob_len))[0] == -8
    assert variant("neg.parquet", b"\x56" + S.w_zz(-3) + b"\x15" + S.w_zz(blob_len))[0] == -8
    assert variant("long.parquet", b"\x56" + S.w_zz(off) + b"\x15" + S.w_zz(len(raw)))[0] == -8
    assert variant("neglen.parquet", b"\x56" + S.w_zz(off) + b"\x15" + S.w_zz(-2))[0] == -8


@pytest.mark.parametrize("bad", [-32, 1, 31, 48, 96, 1000])
def test_writer_rejects_a_malformed_filter(W, tmp_path, bad):
    L = W.lib()
    fields = (W.WriteField * 1)(W.WriteField(b"id", K.INT64, 0, 0))
    w = C.c_void_p()
    assert L.pf_writer_open(str(tmp_path / "x.parquet").encode(), fields, 1, C.byref(w)) == 0
    body = S.w_page_header_v2(4, 0, 0, 0, 32) + bytes(32)
    c, _keep = _chunk(W, body, 4, bytes(2048))
    c.bloom_len = bad
    assert L.pf_writer_add_chunk(w, 0, C.byref(c)) == -1, bad
    c.bloom_len = 64
    c.bloom = None
    assert L.pf_writer_add_chunk(w, 0, C.byref(c)) == -1   # a length without the bytes
    c, _keep = _chunk(W, body, 4, bytes(64))
    assert L.pf_writer_add_chunk(w, 0, C.byref(c)) == 0     # the writer is still usable
    assert L.pf_writer_end_row_group(w, 4) == 0
    assert L.pf_writer_close(w) == 0


def test_parquet_writer_options(W):
    """bloom_filters -> bytes per field, without touching the GPU."""
    sch = W.MessageType("m", W.required(W.INT64).named("a"), W.optional(W.BINARY).as_string().named("s"),
                        W.required(W.BOOLEAN).named("flag"), W.required(W.DOUBLE).named("d"))
    size = W.ParquetWriter._bloom_sizes
    assert size(sch, None, 0.01, 1 << 20) == [0, 0, 0, 0]
    assert size(sch, {"a": 5000, "s": True, "d": {"bytes": 64}}, 0.01, 1 << 20) == [8192, 1 << 20, 0, 64]
    assert size(sch, {"a": 5000, "s": True, "flag": True}, 0.05, 4096) == [4096, 4096, 0, 0]   # BOOLEAN: accepted, no filter
    with pytest.raises(ValueError):
        size(sch, {"nope": 10}, 0.01, 1 << 20)
    with pytest.raises(ValueError):
        size(sch, {"a": {"bytes": 48}}, 0.01, 1 << 20)
    with pytest.raises(ValueError):
        W.ParquetWriter(sch, "/nonexistent-dir/x.parquet", None, bloom_filters={"nope": True})


def test_constants_match_the_header(W):
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "parquet-floor_amd", "csrc", "pf_xxh64.h")).read()
    salts = [int(x, 16) for x in re.search(r"SALT\[8\] = \{([^}]*)\}", src).group(1).replace("u", "").split(",")]
    assert tuple(salts) == B.SALT
    assert (W.BLOOM_MIN_BYTES, W.BLOOM_MAX_BYTES) == (B.MIN_BYTES, B.MAX_BYTES) == (32, 128 << 20)
