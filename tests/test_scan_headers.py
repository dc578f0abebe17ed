"""The page-header walk on hand-assembled Thrift headers (tests/thrift_cases.py): every header of
test_scan.py came out of pyarrow, which writes the fields in one order, in short form, as i32, without unknown
fields or INDEX pages. Here the three parsers - the host walk (pf_file_chunk_desc, csrc/pf_meta.cpp), the oracle
(pfo_chunk_pages) and the GPU scan (pf_scan_pages: k_page_scan / k_page_crc, csrc/pf_scan.hip) - are held to
the descriptors and the (status, err_page) each case was constructed with, field for field and exactly.

CPU: host walk and oracle over every case, the chunks of a group being the columns of one file; the
containers of 2^62 elements in a 40-byte chunk, which must be refused at once. GPU: one pf_scan_pages call
per group (a wave per chunk) at chunk alignments 0..3, from host and from device memory, with and without
CRC verification; the one-byte damages of every valid header differentially against the host walk, which
runs over all of them first on the CPU; reuse of a context's scan buffers."""
import ctypes as C
import os

import numpy as np
import pytest

import pagekit as K
import thrift_cases as T
from test_scan import PAGE_FIELDS

STATS = {"mutants": 0, "mutants_cpu_only": 0, "agree_ok": 0, "agree_corrupt": 0}
ORACLE_FIELDS = ("offset", "compressed_size", "uncompressed_size", "page_type", "encoding", "num_values")
MUTANT_GROUPS = sorted({c.group for c in T.mutant_bases()})


def test_case_tables():
    assert T.PAGE_FIELDS == PAGE_FIELDS
    v, i = T.valid_cases(), T.invalid_cases()
    assert all(c.status == T.OK and 1 <= c.n_pages for c in v)
    assert all(c.status in (T.CORRUPT, T.CAPACITY) and c.err_page >= 0 for c in i)
    # every stated window offset is met: the byte after a long min / max on 480..530, a header start on 490..515
    assert {c.name for c in v if c.group == "stats_sweep"} >= {f"after_{k}" for k in range(480, 531)}
    assert {c.name for c in v if c.group == "window"} == {f"start_{k}" for k in range(490, 516)}
    for c in v:
        if c.group == "window":
            assert c.headers[1][0] == int(c.name.split("_")[1])


def test_writer_known_answers():
    """The writer against bytes written out by hand from the compact protocol's definition."""
    W = T.TW
    assert W().integer(1, 3).done() == b"\x15\x06\x00"                          # short form: delta 1, i32; zigzag(3) = 6
    assert W().integer(1, 3, long=True).done() == b"\x05\x02\x06\x00"            # long form: type, zigzag(id)
    assert W().integer(1, -1, t=3).integer(2, -2, t=4).integer(3, 64, t=6).done() == b"\x13\xff\x14\x03\x16\x80\x01\x00"
    assert W().integer(20, 1).integer(3, 1).done() == b"\x05\x28\x02\x05\x06\x02\x00"  # delta 20 and a negative delta: long
    assert W().integer(65541, 0).integer(6, 0).done() == b"\x05\x8a\x80\x08\x00\x15\x00\x00"   # a reader's last id is 5
    assert W().integer(1, 3, pad=5).done() == b"\x15\x86\x80\x80\x80\x00\x00"
    assert T.uvarint(1, 10) == b"\x81" + b"\x80" * 8 + b"\x00" and T.uvarint(300) == b"\xac\x02"
    assert W().double(1, 1.0).done() == b"\x17" + b"\x00" * 6 + b"\xf0\x3f\x00"
    assert W().binary(2, b"ab").binary(3, b"", pad=2).done() == b"\x28\x02ab\x18\x80\x00\x00"
    assert W().list_(1, 5, [T.e_int(1), T.e_int(-1)]).done() == b"\x19\x25\x02\x01\x00"
    assert W().list_(1, 5, [T.e_int(1)], long=True).done() == b"\x19\xf5\x01\x02\x00"
    assert W().list_(1, 6, [T.e_int(0)] * 15, set_=True).done() == b"\x1a\xf6\x0f" + b"\x00" * 15 + b"\x00"
    assert W().list_(1, 1, [T.e_bool(True), T.e_bool(False)]).done() == b"\x19\x21\x01\x02\x00"   # container bools: a byte each
    assert W().map_(1, 5, 8, []).done() == b"\x1b\x00\x00"                       # the empty map: no key / value type byte
    assert W().map_(1, 1, 1, [(T.e_bool(True), T.e_bool(False))]).done() == b"\x1b\x01\x11\x01\x02\x00"
    assert W().struct(1, [T.I(1, 1), T.S(2, [T.F(1, 1), T.F(2, 2)])]).done() == b"\x1c\x15\x02\x1c\x11\x12\x00\x00\x00"
    assert T.nest(3) == b"\x1c\x1c\x00\x00\x00" and T.nest_mixed(3) == b"\x1c\x19\x15\x0e\x00"
    p = T.v1_page(b"xyz", 2, enc=8)
    assert p.header() == b"\x15\x00\x15\x14\x15\x06\x2c\x15\x04\x15\x10\x15\x06\x15\x08\x00\x00"


# ---------------------------------------------------------------- files of chunks
def _file(tmp, name, items):
    """items: [(chunk bytes, num_values)] as the columns of one file (pagekit.build_file over Chunks whose
    pages are set directly). Returns its path."""
    chunks = []
    for i, (data, nv) in enumerate(items):
        ch = K.Chunk(f"c{i}", K.INT32, layout=K.LAYOUTS["a"])
        ch.pages, ch.value_spans, ch.num_entries, ch.usize = [data], [(0, 0)], nv, len(data)
        ch.encodings.add(K.PLAIN)
        chunks.append(ch)
    raw, _ = K.build_file(chunks, 1)
    path = os.path.join(str(tmp), name + ".parquet")
    with open(path, "wb") as f:
        f.write(raw)
    return path


def _host_walk(pf, col):
    """(status, raw pf_page_desc bytes) of pf_file_chunk_desc."""
    from pfloor._native import ChunkDesc, PageDesc, lib
    d = ChunkDesc()
    rc = lib().pf_file_chunk_desc(pf.h, 0, col, 0, C.byref(d))
    if rc != 0:
        return rc, b""
    return 0, C.string_at(d.pages, d.n_pages * C.sizeof(PageDesc)) if d.n_pages else b""


def _descs(raw):
    from pfloor._native import PageDesc
    n = len(raw) // C.sizeof(PageDesc)
    arr = (PageDesc * max(n, 1)).from_buffer_copy(raw.ljust(C.sizeof(PageDesc), b"\0"))
    return [{f: getattr(arr[i], f) for f in PAGE_FIELDS} for i in range(n)]


@pytest.fixture(scope="module")
def group_files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scan_headers")
    groups = {}
    for c in T.valid_cases() + T.invalid_cases() + T.huge_count_cases():
        groups.setdefault(c.group, []).append(c)
    return {g: (_file(tmp, g, [(c.data, c.num_values) for c in cs]), cs) for g, cs in groups.items()}


def _check_cpu(oracle, path, col, c):
    from pfloor.decoder import ParquetFile
    with ParquetFile(path) as pf:
        rc, raw = _host_walk(pf, col)
    with oracle.open(path) as of:
        n, err, pages = of.chunk_pages(0, col, verify_crc=False, cap=c.page_cap)
        nv, errv, _ = of.chunk_pages(0, col, verify_crc=True, cap=c.page_cap)
    if c.status == T.OK:
        assert rc == 0, (c, "host walk")
        assert _descs(raw) == c.pages, (c, "host walk")
        assert (n, err) == (c.n_pages, -1), (c, "oracle")
        for p, want, has in zip(pages, c.pages, c.has_crc):
            assert {f: p[f] & 0xFFFFFFFF if f.endswith("_size") else p[f] for f in ORACLE_FIELDS} == {f: want[f] for f in ORACLE_FIELDS}, (c, "oracle")
            assert p["has_crc"] == has, (c, "oracle has_crc")
        bad = [k for k, p in enumerate(pages) if not p["crc_ok"]]
        if c.crc_status == T.OK:
            assert bad == [] and (nv, errv) == (c.n_pages, -1), (c, "oracle crc")
        else:
            assert bad == [c.crc_err_page] and (nv, errv) == (c.crc_status, c.crc_err_page), (c, "oracle crc")
    else:
        if c.status == T.CORRUPT:      # the host walk has no slot limit
            assert rc == T.CORRUPT, (c, "host walk")
        assert (n, err) == (c.status, c.err_page), (c, "oracle")


@pytest.mark.parametrize("case", T.valid_cases(), ids=repr)
def test_host_walk_and_oracle_valid(oracle, group_files, case):
    path, cs = group_files[case.group]
    _check_cpu(oracle, path, cs.index(case), case)


@pytest.mark.parametrize("case", T.invalid_cases(), ids=repr)
def test_host_walk_and_oracle_invalid(oracle, group_files, case):
    path, cs = group_files[case.group]
    _check_cpu(oracle, path, cs.index(case), case)


@pytest.mark.parametrize("case", T.huge_count_cases(), ids=repr)
def test_huge_counts_refused_at_once(oracle, group_files, case):
    """A container of 2^62 elements in a 40-byte chunk: every element costs a byte, so the walk ends where the
    chunk does (a parser in which an element is free would still be counting when the machine is retired)."""
    assert len(case.data) == 40 and not case.gpu
    path, cs = group_files[case.group]
    _check_cpu(oracle, path, cs.index(case), case)


@pytest.mark.parametrize("group", MUTANT_GROUPS)
def test_mutants_oracle_matches_host_walk(oracle, tmp_path, group):
    """The one-byte damages of every header, CPU side: the oracle's walk and the host walk give the same
    status and, where that is OK, the same pages."""
    from pfloor.decoder import ParquetFile
    for base in (c for c in T.mutant_bases() if c.group == group):
        gpu, cpu_only = T.mutants(base)
        path = _file(tmp_path, "m", [(m, base.num_values) for _, m in gpu + cpu_only])
        with ParquetFile(path) as pf, oracle.open(path) as of:
            for col, (name, _) in enumerate(gpu + cpu_only):
                rc, raw = _host_walk(pf, col)
                n, _, pages = of.chunk_pages(0, col, cap=64)
                if rc != T.OK:
                    assert n == rc, name
                    continue
                want = _descs(raw)
                assert n == len(want), name
                assert [{f: p[f] & 0xFFFFFFFF for f in ORACLE_FIELDS} for p in pages] == \
                    [{f: w[f] & 0xFFFFFFFF for f in ORACLE_FIELDS} for w in want], name


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dec():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _layout(datas, align=0):
    """One buffer of the chunks, every chunk start at byte alignment `align` (mod 4), the last chunk ending the
    buffer. Returns (bytes, [offset])."""
    buf = bytearray()
    offs = []
    for d in datas:
        buf += bytes((align - len(buf)) % 4)
        offs.append(len(buf))
        buf += d
    return bytes(buf), offs


def _scan(dec, buf, chunks, verify_crc=False, device_ptr=None):
    """pf_scan_pages over chunks = [(offset, size, num_values, page_base, page_cap)]: (rc, [(status, err_page,
    n_pages, crc_pages, raw descriptors of the n_pages slots)])."""
    from pfloor._native import PageDesc, ScanChunk, ScanResult, lib
    n = len(chunks)
    sc = (ScanChunk * max(n, 1))(*[ScanChunk(*c) for c in chunks])
    slots = max([c[3] + c[4] for c in chunks], default=0)
    pages = (PageDesc * max(slots, 1))()
    C.memset(pages, 0x5A, C.sizeof(pages))
    res = (ScanResult * max(n, 1))()
    host = np.frombuffer(buf, np.uint8) if len(buf) else np.zeros(1, np.uint8)
    ptr = device_ptr if device_ptr is not None else host.ctypes.data
    rc = lib().pf_scan_pages(dec.h, sc, n, C.c_void_p(ptr), len(buf), int(device_ptr is not None), int(verify_crc), pages, res)
    raw = bytes(pages)
    sz = C.sizeof(PageDesc)
    out = []
    for i, c in enumerate(chunks):
        r = res[i]
        assert 0 <= r.n_pages <= c[4]
        out.append((r.status, r.err_page, r.n_pages, r.crc_pages, raw[c[3] * sz:(c[3] + r.n_pages) * sz]))
    return rc, out


def _chunks_of(cases, offs):
    out, base = [], 0
    for c, off in zip(cases, offs):
        out.append((off, len(c.data), c.num_values, base, c.page_cap))
        base += c.page_cap
    return out


def _check_gpu(cases, res, verify_crc):
    for c, (st, err, n, ncrc, raw) in zip(cases, res):
        want = (c.crc_status, c.crc_err_page) if verify_crc else (c.status, c.err_page)
        assert (st, err) == want, (c, verify_crc)
        assert n == c.n_pages, c
        assert _descs(raw) == c.pages, c
        assert ncrc == (c.crc_pages() if verify_crc else 0), c


def _ending(cases, align, want):
    """The cases reordered so that the buffer of _layout(align) has a length of `want` mod 4."""
    k = next(i for i, c in enumerate(cases) if (align + len(c.data)) % 4 == want)
    return cases[:k] + cases[k + 1:] + [cases[k]]


@pytest.mark.gpu
@pytest.mark.parametrize("align,ends", [(0, 1), (1, 2), (2, 3), (3, 1)])
def test_gpu_valid_chunks(dec, align, ends):
    """Every valid chunk in one call, a wave each, page_cap = n_pages exactly; chunk starts at byte alignment
    `align`, the last chunk ending a buffer whose length is `ends` mod 4; verify_crc off and on."""
    cases = _ending(list(T.valid_cases()), align, ends)
    buf, offs = _layout([c.data for c in cases], align)
    assert len(buf) % 4 == ends and all(o % 4 == align for o in offs) and offs[-1] + len(cases[-1].data) == len(buf)
    for verify in (False, True):
        rc, res = _scan(dec, buf, _chunks_of(cases, offs), verify)
        assert rc == (T.CORRUPT if verify else T.OK)      # the crc_bad chunks
        _check_gpu(cases, res, verify)


@pytest.mark.gpu
def test_gpu_valid_chunks_from_device_memory(dec):
    from pfloor._native import check, lib
    cases = _ending(list(T.valid_cases()), 1, 3)
    buf, offs = _layout([c.data for c in cases], 1)
    L = lib()
    dptr = C.c_void_p()
    check(L.pf_device_alloc(dec.h, len(buf), C.byref(dptr)), dec.h)
    try:
        host = np.frombuffer(buf, np.uint8)
        check(L.pf_memcpy_h2d(dec.h, dptr, host.ctypes.data, len(buf)), dec.h)
        check(L.pf_sync(dec.h), dec.h)
        for verify in (False, True):
            rc, res = _scan(dec, buf, _chunks_of(cases, offs), verify, device_ptr=dptr.value)
            _check_gpu(cases, res, verify)
    finally:
        L.pf_device_free(dec.h, dptr)


@pytest.mark.gpu
def test_gpu_invalid_chunks(dec):
    cases = [c for c in T.invalid_cases() if c.gpu]
    assert len(cases) == len(T.invalid_cases())
    buf, offs = _layout([c.data for c in cases], 3)
    for verify in (False, True):
        rc, res = _scan(dec, buf, _chunks_of(cases, offs), verify)
        assert rc == cases[0].status
        _check_gpu(cases, res, verify)
    # the capacity case with one slot more is the valid chunk
    c = next(c for c in cases if c.name == "page_cap_one_short")
    rc, res = _scan(dec, c.data, [(0, len(c.data), c.num_values, 0, c.page_cap + 1)])
    assert rc == 0 and res[0][:3] == (0, -1, c.page_cap + 1) and _descs(res[0][4])[:c.page_cap] == c.pages


@pytest.mark.gpu
@pytest.mark.parametrize("group", MUTANT_GROUPS)
def test_gpu_mutants_match_host_walk(dec, tmp_path, group):
    """Every one-byte damage of every header of the group's chunks. Per base chunk: its mutants are the
    columns of one file, the host walk runs over all of them on the CPU, and only then does one pf_scan_pages
    call see them. Same status; where that is OK, the same descriptors."""
    from pfloor.decoder import ParquetFile
    for base in (c for c in T.mutant_bases() if c.group == group):
        gpu, cpu_only = T.mutants(base)
        assert gpu
        path = _file(tmp_path, "m", [(m, base.num_values) for _, m in gpu + cpu_only])
        with ParquetFile(path) as pf:
            host = [_host_walk(pf, col) for col in range(len(gpu) + len(cpu_only))]
        assert all(rc in (T.OK, T.CORRUPT) for rc, _ in host)
        buf, offs = _layout([m for _, m in gpu], 1)
        cap = 64                          # far more pages than a damaged chunk of this size can hold
        rc, res = _scan(dec, buf, [(off, len(m), base.num_values, i * cap, cap) for i, (off, (_, m)) in enumerate(zip(offs, gpu))])
        for (name, _), (hrc, hraw), (st, err, n, _, raw) in zip(gpu, host, res):
            assert st == hrc, (name, st, err, hrc)
            if st == T.OK:
                assert raw == hraw, (name, _descs(raw), _descs(hraw))
                STATS["agree_ok"] += 1
            else:
                STATS["agree_corrupt"] += 1
        STATS["mutants"] += len(gpu)
        STATS["mutants_cpu_only"] += len(cpu_only)


@pytest.mark.gpu
def test_gpu_scan_buffers_carry_nothing_over(dec):
    """The context's scan buffers are reused from call to call: the largest group, a one-chunk group and the
    largest again give what they gave first; chunks without values, of size 0, and scattered page_bases."""
    big = list(T.valid_cases()) + list(T.invalid_cases())
    buf, offs = _layout([c.data for c in big], 2)
    chunks = _chunks_of(big, offs)
    first = _scan(dec, buf, chunks, True)
    one = [c for c in T.valid_cases() if c.name == "two_small"]
    first_one = _scan(dec, one[0].data, _chunks_of(one, [0]), True)
    _check_gpu(one, first_one[1], True)
    assert _scan(dec, buf, chunks, True) == first
    assert _scan(dec, one[0].data, _chunks_of(one, [0]), True) == first_one
    _check_gpu(big, first[1], True)
    # num_values = 0 (nothing is read, whatever the bytes), size 0, and page_bases out of order with gaps
    a, b = T.valid_cases()[0], T.valid_cases()[1]
    buf, offs = _layout([a.data, b"\xff" * 33, b.data], 0)
    chunks = [(offs[0], len(a.data), a.num_values, 40, a.page_cap), (offs[1], 33, 0, 7, 1), (len(buf), 0, 0, 0, 0),
              (offs[2], len(b.data), b.num_values, 11, b.page_cap), (offs[1], 0, 0, 3, 2)]
    rc, res = _scan(dec, buf, chunks, True)
    assert rc == 0
    _check_gpu([a], res[:1], True)
    _check_gpu([b], res[3:4], True)
    for k in (1, 2, 4):
        assert res[k] == (0, -1, 0, 0, b"")


@pytest.mark.gpu
def test_scan_headers_report():
    """Counts (run after the tests above): neither class of agreement may be empty."""
    print(f"scan headers: {len(T.valid_cases())} valid chunks, {len(T.invalid_cases())} invalid chunks, {STATS['mutants']} mutants on the GPU "
          f"(+ {STATS['mutants_cpu_only']} host walk only: a damaged container count above {T.MAX_GPU_COUNT})")
    print(f"host walk and GPU scan agreed on OK for {STATS['agree_ok']} mutants, on corrupt for {STATS['agree_corrupt']}")
    assert STATS["agree_ok"] > 0 and STATS["agree_corrupt"] > 0
