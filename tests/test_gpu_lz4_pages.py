"""LZ4_RAW-compressed pages through the whole read path. pyarrow writes each table four times --
LZ4 (parquet-format codec 7, LZ4_RAW), uncompressed, Snappy, ZSTD -- with the same page layout; the
expected arrays are the oracle's decode of the uncompressed twin (the oracle knows no LZ4), pyarrow's
own read of the LZ4 file is the second witness. 50,000 rows: INT32 / INT64 / DOUBLE / BOOLEAN /
strings, dictionary and PLAIN, 30 % nulls, a LIST column, v1 and v2 pages; the PLAIN INT64 and DOUBLE
chunks are single 400 KB pages, so offsets reach back over more than 32 KiB of output."""
import re

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import lz4_blocks as L
from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

ROWS = 50_000
DICT_COLS = ["i32_d", "s_d"]
FLAT = ["i32_d", "i32_p", "i64_p", "f64_p", "flag", "s_d", "s_p"]
LZ4_RAW = 7


def _table():
    rng = np.random.default_rng(31)
    null = rng.random(ROWS) < 0.3
    words = np.array([f"w{int(k)}" * (1 + int(k) % 4) for k in range(5000)], dtype=object)
    cols = {
        "i32_d": pa.array(rng.integers(0, 200, ROWS).astype(np.int32), mask=null),
        "i32_p": pa.array(rng.integers(0, 1 << 20, ROWS).astype(np.int32), mask=null),
        "i64_p": pa.array(np.cumsum(rng.integers(0, 9, ROWS)).astype(np.int64)),
        "f64_p": pa.array(np.round(rng.normal(0, 50, ROWS), 1), mask=null),
        "flag": pa.array(rng.random(ROWS) < 0.2, mask=null),
        "s_d": pa.array(words[rng.integers(0, 40, ROWS)], mask=null, type=pa.string()),
        "s_p": pa.array(words[rng.zipf(1.4, ROWS) % 5000], mask=null, type=pa.string()),
        "lst": pa.array([None if null[i] else list(range(i % 5)) for i in range(ROWS)], type=pa.list_(pa.int32())),
    }
    return pa.table(cols)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("lz4_pages")
    t = _table()
    out = {}
    for ver in ("1.0", "2.0"):
        for codec in ("LZ4", "NONE", "SNAPPY", "ZSTD"):
            p = str(d / f"t_{codec}_{ver}.parquet")
            pq.write_table(t, p, compression=codec, data_page_version=ver, use_dictionary=DICT_COLS,
                           data_page_size=1 << 20, max_rows_per_page=ROWS, row_group_size=ROWS, write_statistics=True,
                           write_page_index=True)
            out[(codec, ver)] = p
    # a column without a value: its v2 pages have an empty values section
    nulls = pa.table({"n": pa.array([None] * 3000, type=pa.int32()), "x": pa.array(np.arange(3000, dtype=np.int32))})
    out["nulls"] = str(d / "nulls.parquet")
    pq.write_table(nulls, out["nulls"], compression="NONE", data_page_version="2.0", use_dictionary=False)
    return t, out


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _pages(path):
    from pfloor.decoder import ParquetFile
    with ParquetFile(path) as pf:
        descs = [pf.chunk_desc(0, c, 0) for c in range(pf.num_columns)]
        return [d.codec for d in descs], [[(d.pages[i].page_type, d.pages[i].num_values, d.pages[i].uncompressed_size)
                                           for i in range(d.n_pages)] for d in descs]


@pytest.mark.parametrize("ver", ["1.0", "2.0"])
def test_lz4_file_equals_uncompressed_twin(files, decoder, oracle, ver):
    from pfloor.decoder import decode_file
    t, paths = files
    z, n = paths[("LZ4", ver)], paths[("NONE", ver)]
    (cz, pz), (cn, pn) = _pages(z), _pages(n)
    assert set(cz) == {LZ4_RAW} and set(cn) == {0}                       # pf_file_chunk_desc reports codec 7
    assert pz == pn                                                      # the same pages per chunk
    assert any(u > 300_000 for ch in pz for _, _, u in ch)               # a 400 KB page
    assert pq.ParquetFile(z).metadata.row_group(0).column(0).compression == "LZ4"
    assert pq.read_table(z).equals(t)                                    # second witness: the file holds the table
    got = decode_file(z, decoder=decoder)
    assert got["_status"] == 0, got["_error"]
    with oracle.open(n) as of:
        for key, g in got.items():
            if isinstance(key, tuple):
                assert g["status"] == 0, key
                assert_chunk_equal(g, of.decode(*key), f"lz4 v{ver} {key}")
    # pyarrow's values of the REQUIRED column against ours, directly
    i64 = got[(0, t.column_names.index("i64_p"))]
    assert np.array_equal(np.frombuffer(i64["values"].tobytes(), np.int64), t["i64_p"].to_numpy())


def _batch(dec, parts, tweak=None):
    """One decode call over chunks of several files: parts = [(ParquetFile, column)]."""
    sizes = [pf.chunk_range(0, col) for pf, col in parts]
    offs, total = [], 0
    for _, nb in sizes:
        offs.append(total)
        total += (nb + 255) // 256 * 256
    buf = dec.staging(total)
    arr = buf.array(np.uint8, total)
    descs = []
    for (pf, col), (s, nb), off in zip(parts, sizes, offs):
        pf.read_into(s, nb, buf.ptr.value + off)
        descs.append(pf.chunk_desc(0, col, off))
    if tweak:
        tweak(descs, arr)
    dec.decode(descs, buf.ptr.value, total)
    rc = dec.wait()
    return rc, [dec.fetch(i, pf.columns[col].physical_type, pf.columns[col].max_def, pf.columns[col].max_rep)
                for i, (pf, col) in enumerate(parts)]


def test_one_call_mixes_lz4_zstd_snappy_and_uncompressed(files, decoder, oracle):
    from pfloor.decoder import ParquetFile
    t, paths = files
    with ParquetFile(paths[("LZ4", "2.0")]) as fl, ParquetFile(paths[("SNAPPY", "1.0")]) as fs, \
            ParquetFile(paths[("NONE", "2.0")]) as fn, ParquetFile(paths[("ZSTD", "1.0")]) as fz, \
            ParquetFile(paths[("LZ4", "1.0")]) as fl1, \
            oracle.open(paths[("NONE", "2.0")]) as o2, oracle.open(paths[("NONE", "1.0")]) as o1:
        parts = [(fl, 0), (fs, 1), (fn, 2), (fz, 3), (fl, 6), (fs, 7), (fl1, 3), (fz, 5), (fl, 7), (fl1, 2)]
        rc, got = _batch(decoder, parts)
        assert rc == 0, decoder.error()
        for (pf, col), g in zip(parts, got):
            assert_chunk_equal(g, (o1 if pf in (fs, fz, fl1) else o2).decode(0, col), f"mixed c{col}")


def test_v2_page_stored_uncompressed_in_an_lz4_chunk(files, decoder, oracle):
    """DataPageHeaderV2.is_compressed = false inside an LZ4_RAW chunk: the uncompressed twin's chunk
    presented with codec 7 and every data page's flag cleared (the chunks here are PLAIN)."""
    from pfloor.decoder import ParquetFile
    t, paths = files
    cols = [t.column_names.index(c) for c in ("i32_p", "s_p", "lst")]

    def tweak(descs, arr):
        for d in descs:
            d.codec = LZ4_RAW
            for i in range(d.n_pages):
                assert d.pages[i].page_type == 3
                d.pages[i].is_compressed = 0

    with ParquetFile(paths[("NONE", "2.0")]) as fn, oracle.open(paths[("NONE", "2.0")]) as of:
        rc, got = _batch(decoder, [(fn, c) for c in cols], tweak)
        assert rc == 0, decoder.error()
        for c, g in zip(cols, got):
            assert_chunk_equal(g, of.decode(0, c), f"v2 stored c{c}")


def test_all_null_v2_page_flagged_compressed(files, decoder, oracle):
    """A v2 page without a value, presented as a writer may store it: is_compressed = 1 and no byte
    behind the levels. Nothing is decompressed; the page is its levels."""
    from pfloor.decoder import ParquetFile
    _, paths = files
    seen = []

    def tweak(descs, arr):
        for d in descs:
            d.codec = LZ4_RAW
        d = descs[0]
        for i in range(d.n_pages):
            pg = d.pages[i]
            assert pg.page_type == 3 and pg.compressed_size == pg.rep_bytes + pg.def_bytes == pg.uncompressed_size
            pg.is_compressed = 1
            seen.append(i)
        for i in range(descs[1].n_pages):
            descs[1].pages[i].is_compressed = 0

    with ParquetFile(paths["nulls"]) as fn, oracle.open(paths["nulls"]) as of:
        rc, got = _batch(decoder, [(fn, 0), (fn, 1)], tweak)
        assert rc == 0 and seen, decoder.error()
        for c, g in enumerate(got):
            assert_chunk_equal(g, of.decode(0, c), f"all null c{c}")


def test_damaged_page_fails_its_chunk_alone(files, decoder, oracle):
    from pfloor.decoder import ParquetFile
    t, paths = files
    hit = {}

    def tweak(descs, arr):
        d = descs[1]
        pg = d.pages[d.n_pages - 1]          # the chunk's last page: its first offset is made to reach back 65,535 bytes
        at = d.chunk_offset + pg.offset
        block = bytes(arr[at:at + pg.compressed_size])
        assert L.model(block, pg.uncompressed_size) is not None
        o = L.first_offset_at(block)
        arr[at + o] = arr[at + o + 1] = 0xFF
        damaged = bytes(arr[at:at + pg.compressed_size])
        why = []
        assert L.model(damaged, pg.uncompressed_size, why) is None and why == ["offset past the bytes produced"]
        hit["page"] = sum(x.n_pages for x in descs[:1]) + d.n_pages - 1

    with ParquetFile(paths[("LZ4", "1.0")]) as fz, oracle.open(paths[("NONE", "1.0")]) as of:
        cols = [0, 2, 1]                     # (the damaged chunk is i64_p: i32_p's pages are one literal run, no offset)
        rc, got = _batch(decoder, [(fz, c) for c in cols], tweak)
        assert rc == -2
        assert [g["status"] for g in got] == [0, -2, 0]
        m = re.search(r"chunk (\d+): decode failed \(status (-?\d+), page (\d+)\)", decoder.error())
        assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (1, -2, hit["page"]), decoder.error()
        for i in (0, 2):
            assert_chunk_equal(got[i], of.decode(0, cols[i]), f"neighbour c{cols[i]}")


def test_refused_codecs_stay_refused(files, decoder):
    """GZIP, LZO, BROTLI and the Hadoop-framed LZ4 (5) are still PF_ERR_UNSUPPORTED_CODEC, beside an LZ4_RAW chunk that decodes."""
    from pfloor.decoder import ParquetFile
    _, paths = files
    for codec in (2, 3, 4, 5):
        def tweak(descs, arr, codec=codec):
            descs[0].codec = codec

        with ParquetFile(paths[("LZ4", "1.0")]) as fl:
            rc, got = _batch(decoder, [(fl, 0), (fl, 1)], tweak)
            assert rc == -4 and [g["status"] for g in got] == [-4, 0], (codec, rc)


def test_reader_rows_equal_the_snappy_twin(files):
    from pfloor.reader import Hydrator, HydratorSupplier, ParquetReader

    class Rows(Hydrator):
        def start(self):
            return []

        def add(self, t, h, v):
            t.append((h, v))
            return t

        def finish(self, t):
            return tuple(t)

    _, paths = files

    def rows(p):
        with ParquetReader.streamContent(p, HydratorSupplier.constantly(Rows()), set(FLAT) - {"i32_p"}) as s:
            return s.collect()

    z, s = rows(paths[("LZ4", "2.0")]), rows(paths[("SNAPPY", "2.0")])
    assert len(z) == ROWS and z == s


def test_row_range_and_filter_equal_the_uncompressed_twin(files, decoder):
    from pfloor.decoder import decode_file
    from pfloor.predicate import NotNull, Range
    t, paths = files
    cols = [t.column_names.index(c) for c in FLAT]
    i64 = t["i64_p"].to_numpy()
    for ver in ("1.0", "2.0"):
        z, n = paths[("LZ4", ver)], paths[("NONE", ver)]
        for kw in (dict(rows=(12_345, 31_007)),
                   dict(where=[Range("i64_p", int(i64[20_000]), int(i64[29_000])), NotNull("f64_p")]),
                   dict(rows=(5_000, 45_000), where=[Range("i32_p", 1000, 500_000)])):
            a, b = decode_file(z, columns=cols, decoder=decoder, **kw), decode_file(n, columns=cols, decoder=decoder, **kw)
            assert a["_status"] == 0 and b["_status"] == 0, (a["_error"], b["_error"])
            assert set(a) == set(b)
            for key in a:
                if isinstance(key, tuple):
                    assert a[key]["num_rows"] > 1000
                    assert_chunk_equal(a[key], b[key], f"v{ver} {sorted(kw)} {key}")
                elif key == "_selection":
                    assert a[key][0] == b[key][0] and np.array_equal(a[key][1], b[key][1])
                else:
                    assert a[key] == b[key], key
