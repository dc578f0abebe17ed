"""k_snappy_head / k_snappy_litcopy and the executor's direct output on hand-built Snappy pages.

pyarrow-written files reach these only with the tokens Google's compressor chooses. Here every page's
compressed body is assembled token by token (snappy_tokens.py) behind a hand-written v1 page header,
the chunk is written with the product's host file writer (pf_writer_*, codec = SNAPPY) the way
test_short_runs.py does, and one decode carries jobs of every class at once. Values and validity are
compared with the numpy source (the assembler's expected bytes) and with the oracle; per job
pf_debug_snappy_fallback and per page pf_debug_page_direct must be the code read off k_snappy_head
(pf_snappy_head.hip) -- the table in _pages() names the line that decides each.

Columns: REQUIRED INT64 PLAIN, 5000 values a page (no level section: dlo = 0); OPTIONAL INT64 PLAIN with
every value present (the page statistics say null_count = 0, as parquet-mr's and Arrow's do, except on
one page), 8192 values a page: the v1 level section is a 4-byte length plus one RLE run,
4 + 4 = 8 bytes at 8192 values (the run header is a 3-byte varint from 8192 values on). k_snappy_head
only takes a page as DIRECT_VALUES when values - L is 4-byte aligned ("gran == 0: return"), which the
7-byte section of a 5000-value page is not; 8 + 65536 bytes also puts a 64 KiB piece mark in the page."""
import ctypes as C

import numpy as np
import pytest

import snappy_tokens as T
from golden_util import assert_chunk_equal
from test_short_runs import _ci32, _uvarint

pytestmark = pytest.mark.gpu

DIRECT_NONE, DIRECT_VALUES, DIRECT_INPLACE = 0, 1, 2
FB_OK, FB_REDO, FB_INPLACE, FB_LITCOPY = 0, 2, 4, 5      # pf_snappy_par.h
LC_MAX = 32                                              # pf_snappy_par.h: literals of a FB_LITCOPY job
NV_REQ, NV_OPT = 5000, 8192


def _levels(nv):
    run = _uvarint(nv << 1) + b"\x01"                     # one RLE run of nv ones (bit width 1)
    return len(run).to_bytes(4, "little") + run


def _page_header(ptype, usize, csize, inner_field_delta, inner):
    return _ci32(1, ptype) + _ci32(1, usize) + _ci32(1, csize) + bytes([(inner_field_delta << 4) | 12]) + inner + b"\x00\x00"


def _data_page(stream, usize, nv, encoding=0, statistics=False):
    dph = _ci32(1, nv) + _ci32(1, encoding) + _ci32(1, 3) + _ci32(1, 3)      # def / rep levels: RLE
    if statistics:
        dph += bytes([(1 << 4) | 12, (3 << 4) | 6, 0, 0])                    # 5: Statistics { 3: null_count = 0 }
    return _page_header(0, usize, len(stream), 2, dph) + stream


def _dict_page(stream, usize, n):
    dph = _ci32(1, n) + _ci32(1, 0)                                          # PLAIN
    return _page_header(2, usize, len(stream), 4, dph) + stream


# ---- page bodies: fn(s, head, total) appends tokens whose output is `head` (the level section, or
# nothing) followed by value bytes, `total` bytes in all

def _end(s, total):
    """Literals up to `total`, with a token at the 64 KiB mark if the page crosses it."""
    if total > T.BLOCK > s.opos:
        s.fill_output_to(T.BLOCK)
    if total > s.opos:
        s.lit(s.rand(total - s.opos))
    assert s.opos == total


def _one_literal(nb=None):
    return lambda s, head, total: s.lit(head + s.rand(total - len(head)), nb=nb)


def _literals(k, tail_copy=False):
    def fn(s, head, total):
        body = total - (4 if tail_copy else 0)
        cuts = [body * i // k for i in range(k + 1)]
        assert cuts[1] > len(head) + 8
        for a, b in zip(cuts, cuts[1:]):
            s.lit((head + s.rand(b - len(head))) if a == 0 else s.rand(b - a))
        if tail_copy:
            s.copy(2, 8, 4)
        assert s.opos == total
    return fn


def _compressible(straddle=False, split_head=False):
    """Near copies and far copies (the value pattern repeats about every 5000 bytes, beyond XRING = 4096).
    straddle: one far copy whose source spans the last level bytes and the first value bytes
    (a < dlo < a + len). split_head: the first literal is 3 bytes, so the level section is split."""
    def fn(s, head, total):
        if split_head:
            s.lit(head[:3]).lit(head[3:] + s.rand(5000))
        else:
            s.lit(head + s.rand(5000))
        s.lit(s.rand(300))                  # (keeps every other far source clear of the level section)
        if straddle:
            s.copy(2, s.opos - (len(head) - 4), 8)
        while s.opos < total - 400 and (s.opos > T.BLOCK or s.room() > 400):
            s.copy(2, 5000 + 8 * int(s.rng.integers(0, 4)), int(s.rng.integers(8, 65)))      # far
            s.lit(s.rand(int(s.rng.integers(1, 24))))
            s.copy(1, 8 * int(s.rng.integers(1, 12)), 8).copy(2, 16, 48)                      # near, overlapping
            if s.opos < total - 3000 and s.opos % T.BLOCK < T.BLOCK - 3000 and s.rng.random() < 0.3:
                s.lit(s.rand(int(s.rng.integers(100, 1500))))
        _end(s, total)
    return fn


def _pages(optional):
    """[(name, body builder, pf_debug_snappy_fallback, pf_debug_page_direct)] with the line of
    k_snappy_head (pf_snappy_head.hip) that decides."""
    pages = [
        # "if (one) { pg.body = in + data; pg.direct = DIRECT_INPLACE; fb[j] = FB_INPLACE; }"
        ("one_literal", _one_literal(), FB_INPLACE, DIRECT_INPLACE),
        ("one_literal_nb3", _one_literal(3), FB_INPLACE, DIRECT_INPLACE),      # snap_tok reads the 3-byte length
        # literal-only streams are longer than their output, so the host flags them (dflags & 2) and
        # "if (p == n && o == J.dst_len && cnt > 0) ... fb[j] = FB_LITCOPY" takes up to LC_MAX literals
        ("literals_2", _literals(2), FB_LITCOPY, DIRECT_NONE),
        ("literals_32", _literals(LC_MAX), FB_LITCOPY, DIRECT_NONE),
        # "while (p < n && cnt < LC_MAX)" stops short of n: "a data page still gets the VALUES setup below"
        ("literals_33", _literals(LC_MAX + 1), FB_OK, DIRECT_VALUES),
        # "if (u.kind != 0 ...) break": not a literal-only stream after all
        ("literals_32_copy", _literals(LC_MAX, tail_copy=True), FB_OK, DIRECT_VALUES),
        # "pg.direct = DIRECT_VALUES": the executor writes the values into the column
        ("compressible", _compressible(), FB_OK, DIRECT_VALUES),
    ]
    if optional:
        pages += [
            # exec5_piece "bad ... far[h] && a[h] < od.dlo && a[h] + ol[h] > od.dlo" rejects the piece, the page
            # is redone whole into its scratch body (FB_REDO); k_snappy_head had already set DIRECT_VALUES
            ("far_copy_straddles_dlo", _compressible(straddle=True), FB_REDO, DIRECT_VALUES),
            # "if (lv > 60u || 4u + lv > t.ol) return;   // the level section must sit in the first literal"
            ("level_section_split", _compressible(split_head=True), FB_OK, DIRECT_NONE),
            # "if (pg.lvltab != nullptr) return;": the only page here without statistics. Its null count is
            # unknown to the host, which gives it a level table; k_page_null then decodes it from its scratch
            # body, so it must not be direct. (It was, and its values came out as the scratch's zeros.)
            ("compressible_no_statistics", _compressible(), FB_OK, DIRECT_NONE),
        ]
    return pages


def _write(path, ptype, optional, body, num_values, n_data_pages, dict_len=-1, dict_entries=0, unc=0):
    from pfloor import _native
    from pfloor.writer import EncodedChunk, WriteField
    L = _native.lib()
    buf = C.create_string_buffer(bytes(body), len(body))
    ch = EncodedChunk()
    ch.bytes = C.cast(buf, C.c_void_p)
    ch.size = len(body)
    ch.total_uncompressed_size = unc
    ch.num_values = num_values
    ch.dictionary_page_offset = 0 if dict_len >= 0 else -1
    ch.data_page_offset = max(dict_len, 0)
    ch.n_data_pages = n_data_pages
    ch.dict_entries = dict_entries
    ch.data_encoding = 8 if dict_len >= 0 else 0
    ch.codec = 1                                                             # SNAPPY
    fields = (WriteField * 1)(WriteField(b"v", ptype, int(optional), 0))
    w = C.c_void_p()
    assert L.pf_writer_open(path.encode(), C.cast(fields, C.c_void_p), 1, C.byref(w)) == 0
    assert L.pf_writer_add_chunk(w, 0, C.byref(ch)) == 0
    assert L.pf_writer_end_row_group(w, num_values) == 0
    assert L.pf_writer_close(w) == 0


def _debug(dec):
    """({page: [fallback, src_len, dst_len, chunk, page]} per Snappy job, [direct] per page)."""
    from pfloor import _native
    L = _native.lib()
    L.pf_debug_snappy_fallback.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    L.pf_debug_page_direct.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    nj = L.pf_debug_snappy_fallback(dec.h, None, 0)
    rec = (C.c_int * (5 * nj))()
    assert L.pf_debug_snappy_fallback(dec.h, rec, nj) == nj
    n = L.pf_debug_page_direct(dec.h, None, 0)
    out = (C.c_int * max(n, 1))()
    assert L.pf_debug_page_direct(dec.h, out, n) == n
    return {rec[5 * j + 4]: list(rec[5 * j:5 * j + 5]) for j in range(nj)}, list(out)[:n]


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


@pytest.mark.parametrize("optional", [False, True], ids=["required", "optional"])
def test_hand_built_plain_pages(decoder, oracle, tmp_path, optional):
    from pfloor.decoder import decode_file
    nv = NV_OPT if optional else NV_REQ
    head = _levels(nv) if optional else b""
    assert len(head) % 4 == 0
    total = len(head) + 8 * nv
    table = _pages(optional)
    body, values, unc = bytearray(), [], 0
    for i, (name, build, _fb, _direct) in enumerate(table):
        s = T.Stream(700 + i)
        build(s, head, total)
        stream, exp = s.finish()
        assert len(exp) == total and exp[:len(head)] == head, name
        values.append(np.frombuffer(exp[len(head):], dtype=np.int64))
        page = _data_page(stream, total, nv, statistics=optional and not name.endswith("_no_statistics"))
        body += page
        unc += len(page) - len(stream) + total
    path = str(tmp_path / f"snappy_pages_{int(optional)}.parquet")
    _write(path, 2, optional, body, nv * len(table), len(table), unc=unc)
    expect = np.concatenate(values)

    got = decode_file(path, decoder=decoder)
    assert got["_status"] == 0, got["_error"]
    g = got[(0, 0)]
    jobs, direct = _debug(decoder)
    assert sorted(jobs) == list(range(len(table))) and len(direct) == len(table)
    gv = np.frombuffer(g["values"].tobytes(), np.int64)
    assert len(gv) == len(expect)
    diff = []
    for p, (name, _b, _fb, _dr) in enumerate(table):
        ne = np.flatnonzero(gv[p * nv:(p + 1) * nv] != values[p])
        if len(ne):
            diff.append(f"{name}: {len(ne)} values differ, first {ne[0]}, last {ne[-1]} (fallback {jobs[p][0]}, direct {direct[p]})")
    assert not diff, "\n".join(diff)
    if optional:
        assert np.unpackbits(g["validity"], bitorder="little")[:len(expect)].all()
    with oracle.open(path) as of:
        ref = of.decode(0, 0)
        assert ref["status"] == 0, ref["error"]
        assert_chunk_equal(g, ref, "hand-built pages")
    wrong =[(name, jobs[p][0], direct[p]) for p, (name, _b, fb, dr) in enumerate(table) if (jobs[p][0], direct[p]) != (fb, dr)]
    assert not wrong, f"(page, fallback, direct) not as pinned: {wrong}"


@pytest.mark.parametrize("dict_literals", [1, LC_MAX + 1])
def test_hand_built_dictionary_page(decoder, oracle, tmp_path, dict_literals):
    """Dictionary pages always go to the literal table ("Dictionary pages always take this"): one literal is
    FB_LITCOPY, never read in place ("one && !(pg.flags & PG_DICT)"); 33 literals overflow LC_MAX and
    "if (pg.flags & PG_DICT) return;" leaves the job to the block-parallel path (code 0). The data page
    (bit-packed ids) is one literal: FB_INPLACE."""
    from pfloor.decoder import decode_file
    rng = np.random.default_rng(9)
    nd, nv = 2000, 4096
    dict_values = rng.integers(-2**62, 2**62, nd).astype(np.int64)
    s = T.Stream(800)
    raw = dict_values.tobytes()
    cuts = [len(raw) * i // dict_literals for i in range(dict_literals + 1)]
    for a, b in zip(cuts, cuts[1:]):
        s.lit(raw[a:b])
    dstream, dexp = s.finish()
    assert dexp == raw
    ids = rng.integers(0, nd, nv)
    bw = 11
    acc = 0
    for k, v in enumerate(ids):
        acc |= int(v) << (k * bw)
    ids_body = bytes([bw]) + _uvarint(((nv // 8) << 1) | 1) + acc.to_bytes(nv * bw // 8, "little")
    s = T.Stream(801)
    s.lit(ids_body)
    pstream, _ = s.finish()
    dp = _dict_page(dstream, len(raw), nd)
    page = _data_page(pstream, len(ids_body), nv, encoding=8)
    path = str(tmp_path / f"snappy_dict_{dict_literals}.parquet")
    _write(path, 2, False, dp + page, nv, 1, dict_len=len(dp), dict_entries=nd,
           unc=len(dp) - len(dstream) + len(raw) + len(page) - len(pstream) + len(ids_body))

    got = decode_file(path, decoder=decoder)
    assert got["_status"] == 0, got["_error"]
    g = got[(0, 0)]
    assert np.array_equal(np.frombuffer(g["values"].tobytes(), np.int64), dict_values[ids])
    with oracle.open(path) as of:
        ref = of.decode(0, 0)
        assert ref["status"] == 0, ref["error"]
        assert_chunk_equal(g, ref, "hand-built dictionary page")
    jobs, direct = _debug(decoder)
    assert sorted(jobs) == [0, 1] and len(direct) == 2
    assert (jobs[0][0], direct[0]) == (FB_LITCOPY if dict_literals == 1 else FB_OK, DIRECT_NONE)
    assert (jobs[1][0], direct[1]) == (FB_INPLACE, DIRECT_INPLACE)


def test_written_file_without_page_statistics(decoder, oracle, tmp_path):
    """The same page as compressible_no_statistics from a real writer: Arrow with write_statistics=False
    leaves the v1 pages of an OPTIONAL column without a null count. k_snappy_head took such PLAIN pages as
    DIRECT_VALUES although k_page_null decodes them from the scratch body, and every value came out 0."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from pfloor.decoder import decode_file
    n = 40_000
    v = (np.arange(n, dtype=np.int64) // 3) * 1_000_003
    path = str(tmp_path / "no_statistics.parquet")
    pq.write_table(pa.table({"v": pa.array(v)}), path, compression="snappy", data_page_version="1.0",
                   use_dictionary=False, write_statistics=False, data_page_size=64 << 10)
    got = decode_file(path, decoder=decoder)
    assert got["_status"] == 0, got["_error"]
    g = got[(0, 0)]
    assert np.array_equal(np.frombuffer(g["values"].tobytes(), np.int64), v)
    with oracle.open(path) as of:
        assert_chunk_equal(g, of.decode(0, 0), "no page statistics")
    jobs, direct = _debug(decoder)
    assert len(jobs) >= 2 and all(j[0] == FB_OK for j in jobs.values()), jobs
    assert direct == [DIRECT_NONE] * len(direct)
