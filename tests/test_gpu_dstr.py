"""k_flat_dstr (pf_flat_dstr.hip): flat dictionary BYTE_ARRAY pages with a small dictionary of short values, decoded one
FBLK block per workgroup with 16 consecutive entries per thread.

Every case is a file of one or more chunks assembled by tests/pagekit.py (run layouts, id widths, page layouts chosen
here) or written by pyarrow. It is decoded three times: by the product library, by the diagnostics build with its
defaults, and by the diagnostics build with PF_FLAT_DSTR=0 (k_flat_all decodes the pages, as before this kernel).
Each chunk must equal the CPU oracle's bit for bit every time. pf_debug_dstr_counts gives {blocks k_flat_dstr
decoded, pages it declined}: by the kernel's rule (all levels present, a run table of at most RUN_CAP runs, at most
256 dictionary entries, a dictionary page body of at most 4096 bytes, no value over 32 bytes) every page of a case is
either taken, block by block, or declined, and the counters must say so. A page with an id outside the dictionary
must give the status and the error of the PF_FLAT_DSTR=0 run."""
import ctypes as C
import os

import numpy as np
import pytest

import pagekit as K
from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

FBLK = 4096
RUN_CAP = 256
COUNTS = (1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 1)


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _dstr_counts():
    """(blocks taken, pages declined) since the last call; diagnostics build only (call inside switches())."""
    from pfloor import _native
    f = _native.lib().pf_debug_dstr_counts
    f.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    buf = (C.c_ulonglong * 2)()
    assert f(buf, 1) == 0
    return int(buf[0]), int(buf[1])


# ---------------------------------------------------------------- dictionaries
def _mixed_dict(n):
    """n values of 0 to 24 bytes, the empty string among them (256 of them: a 4039-byte dictionary page)."""
    return [bytes([65 + (i + k) % 26 for k in range(i % 25)]) for i in range(n)]


DICTS = {
    "one": [b"N"],                                            # id width 0
    "flag2": [b"O", b"F"],                                    # all of length 1
    "flag3": [b"A", b"N", b"R"],
    "mode7": [b"REG AIR", b"AIR", b"RAIL", b"SHIP", b"TRUCK", b"MAIL", b"FOB"],
    "mixed256": _mixed_dict(256),
    "all17": [bytes([97 + i]) * 17 for i in range(5)],
    "empty_only": [b""],
    "mixed25": _mixed_dict(25),
    # declined
    "d257": [bytes([48 + i % 64, 48 + i // 64]) for i in range(257)],
    "big_body": [bytes([65 + i % 26]) * 24 for i in range(200)],   # 200 x (4 + 24) = 5600 bytes
    "long33": [b"ab", b"c" * 33, b"def"],
}
DECLINED_DICTS = ("d257", "big_body", "long33")


def _bw(n):
    return max(n - 1, 0).bit_length()


# ---------------------------------------------------------------- id streams with chosen runs
def _alternating(n, dn, bw, rle_len, rng):
    """RLE runs of rle_len values and one-group bit-packed runs in turn: (ids, stream). 16 consecutive entries
    straddle two or three runs; 2 runs per rle_len + 8 values."""
    ids, out, nb = [], bytearray(), (bw + 7) // 8
    while len(ids) < n:
        v, c = int(rng.integers(dn)), min(rle_len, n - len(ids))
        out += K._uvarint(c << 1) + v.to_bytes(nb, "little")
        ids += [v] * c
        if len(ids) < n:
            g = rng.integers(0, dn, 8)
            out += b"\x03" + K._pack_le(g, bw)
            ids += [int(x) for x in g[:min(8, n - len(ids))]]
    return np.asarray(ids, np.uint64), bytes(out)


def _page(ch, dvals, ids, bw, style="mr", rng=None, present=None, stream=None, encoding=K.RLE_DICTIONARY):
    """One dictionary data page of ch; ids index dvals (an id past the dictionary is kept in the stream and gives
    the last value in the expectation, which such a case never compares)."""
    body = bytes([bw]) + (stream if stream is not None else K.hybrid(ids, bw, style, rng))
    vals = [dvals[min(int(i), len(dvals) - 1)] for i in ids]
    ch.add_page(encoding, body, present=present, vals=vals)


class Case:
    def __init__(self, name, build, taken, declined, bad=False):
        self.name, self.build, self.taken, self.declined, self.bad = name, build, taken, declined, bad


def _blocks(n):
    return max(1, (n + FBLK - 1) // FBLK)


def _simple(dname, counts, style="mr", layout=K.LAYOUTS["a"], optional=False, bw=None, encoding=K.RLE_DICTIONARY, seed=1):
    """One chunk per entry count, one page each, random ids."""
    dvals = DICTS[dname]

    def build(compress):
        rng = np.random.default_rng(seed)
        chunks = []
        for n in counts:
            ch = K.Chunk(f"{dname}_{n}", K.BYTE_ARRAY, optional=optional, layout=layout, compress=compress)
            ch.set_dictionary(dvals, encoding=K.PLAIN if encoding == K.RLE_DICTIONARY else K.PLAIN_DICTIONARY)
            ids = rng.integers(0, len(dvals), n).astype(np.uint64)
            _page(ch, dvals, ids, _bw(len(dvals)) if bw is None else bw, style, rng,
                  present=np.ones(n, bool) if optional else None, encoding=encoding)
            chunks.append(ch)
        return chunks
    declined = dname in DECLINED_DICTS
    return build, (0 if declined else sum(_blocks(n) for n in counts)), (len(counts) if declined else 0)


def _cases():
    out = []
    V1S = K.Layout("v1s", False, K.SNAPPY)
    # entry counts at thread-group and block edges, over the dictionaries and length mixes
    for dname in ("one", "flag2", "flag3", "mode7", "mixed256", "all17", "empty_only", "mixed25"):
        b, t, d = _simple(dname, COUNTS)
        out.append(Case(f"counts-{dname}", b, t, d))
    for dname in DECLINED_DICTS:
        b, t, d = _simple(dname, (17, 4097))
        out.append(Case(f"declined-{dname}", b, t, d))
    # all RLE runs (runs of 1 included: few values, so the table holds them), non-minimal id widths
    b, t, d = _simple("flag3", (1, 17, 200), style="rle")
    out.append(Case("rle-only", b, t, d))
    for bw in (8, 13, 32):
        b, t, d = _simple("mode7", (17, 4097), bw=bw, seed=bw)
        out.append(Case(f"width-{bw}", b, t, d))
    # layouts: v1 / v2, Snappy / uncompressed, PLAIN_DICTIONARY pages
    for lname, lay in (("e", K.LAYOUTS["e"]), ("c", K.LAYOUTS["c"]), ("d", K.LAYOUTS["d"]), ("v1s", V1S)):
        b, t, d = _simple("mixed25", (17, 4097, 2 * 4096 + 1), layout=lay, seed=7)
        out.append(Case(f"layout-{lname}", b, t, d))
    b, t, d = _simple("mode7", (17, 4097), encoding=K.PLAIN_DICTIONARY)
    out.append(Case("plain-dictionary", b, t, d))
    # an OPTIONAL column with every value present is taken; with nulls it is declined
    for lname in ("a", "c"):
        # (from 8 entries on the assembler writes the levels as one RLE run, which is what "all present" reads)
        b, t, d = _simple("mode7", (8, 17, 31, 33, 4097, 2 * 4096 + 1), layout=K.LAYOUTS[lname], optional=True)
        out.append(Case(f"optional-all-present-{lname}", b, t, d))

    def nulls(compress):
        rng = np.random.default_rng(3)
        dvals = DICTS["mode7"]
        ch = K.Chunk("nulls", K.BYTE_ARRAY, optional=True, layout=K.LAYOUTS["a"], compress=compress)
        ch.set_dictionary(dvals)
        present = rng.random(5000) < 0.8
        _page(ch, dvals, rng.integers(0, 7, int(present.sum())).astype(np.uint64), 3, present=present)
        return [ch]
    out.append(Case("optional-nulls", nulls, 0, 1))

    # run layouts
    def rle_three_blocks(compress):
        rng = np.random.default_rng(4)
        dvals = DICTS["mode7"]
        n = 3 * FBLK + 100
        ids = rng.integers(0, 7, n).astype(np.uint64)
        ids[FBLK - 50:2 * FBLK + 50] = 5          # one RLE run over the end of block 0, block 1, the start of block 2
        ch = K.Chunk("rle3", K.BYTE_ARRAY, layout=K.LAYOUTS["a"], compress=compress)
        ch.set_dictionary(dvals)
        _page(ch, dvals, ids, 3)
        return [ch]
    out.append(Case("rle-run-over-three-blocks", rle_three_blocks, _blocks(3 * FBLK + 100), 0))

    def boundary_on_block(compress):
        rng = np.random.default_rng(5)
        dvals = DICTS["mixed25"]
        chunks = []
        for first_rle in (False, True):
            n = 2 * FBLK + 9
            ids = rng.integers(0, 25, n).astype(np.uint64)
            # no long repeats by chance, so the packed runs are cut only where the RLE run starts or ends
            ids = (ids + np.arange(n, dtype=np.uint64) % 2 * 3) % 25
            if first_rle:
                ids[:FBLK] = 11                    # an RLE run that ends exactly where block 1 starts
            else:
                ids[FBLK:FBLK + 64] = 11           # packed groups up to the block boundary, an RLE run from it
            ch = K.Chunk(f"edge_{int(first_rle)}", K.BYTE_ARRAY, layout=K.LAYOUTS["a"], compress=compress)
            ch.set_dictionary(dvals)
            _page(ch, dvals, ids, 5)
            chunks.append(ch)
        return chunks
    out.append(Case("run-boundary-on-block-boundary", boundary_on_block, 2 * _blocks(2 * FBLK + 9), 0))

    def alternating(compress):
        rng = np.random.default_rng(6)
        chunks = []
        for dname, rle_len, n in (("mode7", 5, 1500), ("mode7", 8, 2000), ("mixed25", 3, 1200), ("flag2", 1, 1100),
                                  ("one", 5, 1500)):
            dvals = DICTS[dname]
            bw = _bw(len(dvals))
            ids, stream = _alternating(n, len(dvals), bw, rle_len, rng)
            assert 2 * (n // (rle_len + 8) + 1) <= RUN_CAP
            ch = K.Chunk(f"alt_{dname}_{rle_len}", K.BYTE_ARRAY, layout=K.LAYOUTS["a"], compress=compress)
            ch.set_dictionary(dvals)
            _page(ch, dvals, ids, bw, stream=stream)
            chunks.append(ch)
        return chunks
    out.append(Case("alternating-rle-packed", alternating, 5, 0))

    def too_many_runs(compress):
        rng = np.random.default_rng(8)
        dvals = DICTS["mode7"]
        ch = K.Chunk("mixed", K.BYTE_ARRAY, layout=K.LAYOUTS["a"], compress=compress)
        ch.set_dictionary(dvals)
        _page(ch, dvals, rng.integers(0, 7, 4097).astype(np.uint64), 3, style="mixed", rng=rng)   # > 1000 runs
        return [ch]
    out.append(Case("more-runs-than-the-table", too_many_runs, 0, 1))

    # several pages per chunk: chars bases across pages, page starts that are no multiple of 16 or 4
    def pages(compress):
        rng = np.random.default_rng(9)
        chunks = []
        for lname, lay in (("a", K.LAYOUTS["a"]), ("c", K.LAYOUTS["c"])):
            dvals = DICTS["mixed25"]
            ch = K.Chunk(f"pages_{lname}", K.BYTE_ARRAY, layout=lay, compress=compress)
            ch.set_dictionary(dvals)
            for n in (5001, 17, 4096, 1, 9003):
                _page(ch, dvals, rng.integers(0, 25, n).astype(np.uint64), 5)
            chunks.append(ch)
        return chunks
    out.append(Case("several-pages", pages, 2 * sum(_blocks(n) for n in (5001, 17, 4096, 1, 9003)), 0))

    # errors: one id past the dictionary in the first, a middle and the last block
    for where, pos in (("first", 100), ("middle", FBLK + 2000), ("last", 2 * FBLK)):
        def bad(compress, pos=pos):
            rng = np.random.default_rng(10)
            dvals = DICTS["mode7"]
            ids = rng.integers(0, 7, 2 * FBLK + 1).astype(np.uint64)
            ids = (ids + np.arange(len(ids), dtype=np.uint64) % 2 * 3) % 7
            ids[pos] = 7
            good = K.Chunk("good", K.BYTE_ARRAY, layout=K.LAYOUTS["a"], compress=compress)
            good.set_dictionary(dvals)
            _page(good, dvals, np.where(ids == 7, 0, ids), 3)
            ch = K.Chunk("bad", K.BYTE_ARRAY, layout=K.LAYOUTS["a"], compress=compress)
            ch.set_dictionary(dvals)
            _page(ch, dvals, ids, 3)
            return [good, ch]
        out.append(Case(f"bad-id-{where}-block", bad, None, None, bad=True))
    return out


CASES = {c.name: c for c in _cases()}


def _compare(got, exp, case, tag):
    """Chunks against the oracle; a chunk the oracle rejects must fail on the GPU. Returns {col: (status)}."""
    for c, e in enumerate(exp):
        g = got[(0, c)]
        where = f"{case.name} [{tag}] chunk {c}"
        if e["status"] != 0:
            assert case.bad and g["status"] != 0, f"{where}: the oracle rejects it ({e['error']}), the GPU reports {g['status']}"
            continue
        assert g["status"] == 0, f"{where}: status {g['status']} ({got['_error']})"
        assert_chunk_equal(g, e, where)
    if not case.bad:
        assert got["_status"] == 0, (case.name, tag, got["_error"])


@pytest.mark.parametrize("name", list(CASES))
def test_dstr_case(name, oracle, decoder, switches, tmp_path):
    from pfloor.decoder import GpuDecoder, decode_file
    case = CASES[name]
    chunks = case.build(oracle.snappy_compress)
    data, _info = K.build_file(chunks, max(ch.num_entries for ch in chunks))
    path = os.path.join(str(tmp_path), "dstr.parquet")
    with open(path, "wb") as fh:
        fh.write(data)
    with oracle.open(data=data) as of:
        exp = [of.decode(0, c) for c in range(len(chunks))]
    if not case.bad:   # the assembler's own expectation agrees with the oracle
        for c, ch in enumerate(chunks):
            assert_chunk_equal(exp[c], ch.expected(), f"{name}: oracle against the construction, chunk {c}")
    _compare(decode_file(path, decoder=decoder), exp, case, "product library")
    seen = {}
    for env, tag in (({}, "diagnostics build"), ({"PF_FLAT_DSTR": 0}, "diagnostics build PF_FLAT_DSTR=0")):
        with switches(**env), GpuDecoder(0) as d:
            _dstr_counts()
            got = decode_file(path, decoder=d)
            counts = _dstr_counts()
        print(f"{name} [{tag}]: blocks taken {counts[0]}, pages declined {counts[1]}")
        _compare(got, exp, case, tag)
        seen[tag] = ([got[(0, c)]["status"] for c in range(len(chunks))], got["_status"], got["_error"])
        if env:
            assert counts == (0, 0), f"{name} [{tag}]: the kernel ran ({counts})"
        elif not case.bad:
            assert counts == (case.taken, case.declined), f"{name} [{tag}]: taken, declined {counts}, by the rule " \
                                                          f"{(case.taken, case.declined)}"
    if case.bad:   # status and error as without the kernel
        assert seen["diagnostics build"] == seen["diagnostics build PF_FLAT_DSTR=0"], seen


def test_pyarrow_flags(oracle, switches, tmp_path):
    """lineitem's four small-dictionary string columns as pyarrow writes them (Snappy, v1 and v2 pages, pages of
    20,000 rows) beside a 1000-value vocabulary, which is declined."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from pfloor.decoder import GpuDecoder, decode_file
    rng = np.random.default_rng(11)
    n = 50001
    cols = {
        "l_returnflag": DICTS["flag3"], "l_linestatus": DICTS["flag2"], "l_shipmode": DICTS["mode7"],
        "l_shipinstruct": [b"DELIVER IN PERSON", b"COLLECT COD", b"NONE", b"TAKE BACK RETURN"],
        "vocab": [b"w%04d" % i for i in range(1000)],
    }
    table = pa.table({k: pa.array([v[i] for i in rng.integers(0, len(v), n)], pa.binary()) for k, v in cols.items()})
    for version in ("1.0", "2.0"):
        path = os.path.join(str(tmp_path), f"flags_{version}.parquet")
        pq.write_table(table, path, compression="snappy", use_dictionary=True, data_page_version=version,
                       data_page_size=20000, write_statistics=False)
        with oracle.open(path) as of:
            exp = [of.decode(0, c) for c in range(len(cols))]
        for env in ({}, {"PF_FLAT_DSTR": 0}):
            with switches(**env), GpuDecoder(0) as d:
                _dstr_counts()
                got = decode_file(path, decoder=d)
                counts = _dstr_counts()
            print(f"pyarrow {version} {env}: blocks taken {counts[0]}, pages declined {counts[1]}")
            assert got["_status"] == 0, got["_error"]
            for c in range(len(cols)):
                assert_chunk_equal(got[(0, c)], exp[c], f"pyarrow {version} {env} column {c}")
            if env:
                assert counts == (0, 0)
            else:   # every page of the four flag columns is taken, every page of the vocabulary declined
                assert counts[0] >= 4 * _blocks(n) and counts[1] >= 1, counts
