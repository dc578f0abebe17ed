"""ZSTD-compressed pages through the whole read path. pyarrow writes each table three times --
ZSTD, uncompressed, Snappy -- with the same page layout; the expected arrays are the oracle's decode
of the uncompressed twin (the oracle knows no ZSTD), pyarrow's own read of the ZSTD file is the
second witness. 50,000 rows: INT32 / INT64 / DOUBLE / BOOLEAN / strings, dictionary and PLAIN, 30 %
nulls, a LIST column, v1 and v2 pages; the PLAIN INT64 and DOUBLE chunks are single 400 KB pages, so
their frames have several 128 KiB blocks."""
import ctypes as C
import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

ROWS = 50_000
DICT_COLS = ["i32_d", "s_d"]


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
    d = tmp_path_factory.mktemp("zstd_pages")
    t = _table()
    out = {}
    for ver in ("1.0", "2.0"):
        for codec in ("ZSTD", "NONE", "SNAPPY"):
            p = str(d / f"t_{codec}_{ver}.parquet")
            pq.write_table(t, p, compression=codec, data_page_version=ver, use_dictionary=DICT_COLS,
                           data_page_size=1 << 20, row_group_size=ROWS, write_statistics=True)
            out[(codec, ver)] = p
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
        return [[(pf.chunk_desc(0, c, 0).pages[i].page_type, pf.chunk_desc(0, c, 0).pages[i].num_values,
                  pf.chunk_desc(0, c, 0).pages[i].uncompressed_size) for i in range(pf.chunk_desc(0, c, 0).n_pages)]
                for c in range(pf.num_columns)]


@pytest.mark.parametrize("ver", ["1.0", "2.0"])
def test_zstd_file_equals_uncompressed_twin(files, decoder, oracle, ver):
    from pfloor.decoder import decode_file
    t, paths = files
    z, n = paths[("ZSTD", ver)], paths[("NONE", ver)]
    pz, pn = _pages(z), _pages(n)
    assert pz == pn                                                      # the same pages per chunk
    assert any(u > (128 << 10) for ch in pz for _, _, u in ch)            # a page of several blocks
    assert pq.ParquetFile(z).metadata.row_group(0).column(0).compression == "ZSTD"
    assert pq.read_table(z).equals(t)                                    # second witness: the file holds the table
    got = decode_file(z, decoder=decoder)
    assert got["_status"] == 0, got["_error"]
    with oracle.open(n) as of:
        for key, g in got.items():
            if isinstance(key, tuple):
                assert g["status"] == 0, key
                assert_chunk_equal(g, of.decode(*key), f"zstd v{ver} {key}")
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


def test_one_call_mixes_zstd_snappy_and_uncompressed(files, decoder, oracle):
    from pfloor.decoder import ParquetFile
    t, paths = files
    with ParquetFile(paths[("ZSTD", "2.0")]) as fz, ParquetFile(paths[("SNAPPY", "1.0")]) as fs, \
            ParquetFile(paths[("NONE", "2.0")]) as fn, oracle.open(paths[("NONE", "2.0")]) as o2, \
            oracle.open(paths[("NONE", "1.0")]) as o1:
        parts = [(fz, 0), (fs, 1), (fn, 2), (fz, 6), (fs, 7), (fz, 3)]
        rc, got = _batch(decoder, parts)
        assert rc == 0, decoder.error()
        for (pf, col), g in zip(parts, got):
            assert_chunk_equal(g, (o1 if pf is fs else o2).decode(0, col), f"mixed c{col}")


def test_v2_page_stored_uncompressed_in_a_zstd_chunk(files, decoder, oracle):
    """DataPageHeaderV2.is_compressed = false inside a ZSTD chunk: the uncompressed twin's chunk
    presented with codec ZSTD and every data page's flag cleared (dictionary pages have none: the
    chunks here are PLAIN)."""
    from pfloor.decoder import ParquetFile
    t, paths = files
    cols = [t.column_names.index(c) for c in ("i32_p", "s_p", "lst")]

    def tweak(descs, arr):
        for d in descs:
            d.codec = 6
            for i in range(d.n_pages):
                assert d.pages[i].page_type == 3
                d.pages[i].is_compressed = 0

    with ParquetFile(paths[("NONE", "2.0")]) as fn, oracle.open(paths[("NONE", "2.0")]) as of:
        rc, got = _batch(decoder, [(fn, c) for c in cols], tweak)
        assert rc == 0, decoder.error()
        for c, g in zip(cols, got):
            assert_chunk_equal(g, of.decode(0, c), f"v2 stored c{c}")


def test_damaged_page_fails_its_chunk_alone(files, decoder, oracle):
    from pfloor.decoder import ParquetFile
    t, paths = files
    hit = {}

    def tweak(descs, arr):
        d = descs[1]
        pg = d.pages[d.n_pages - 1]          # the chunk's last page: block type 3 in its first block header
        at = d.chunk_offset + pg.offset
        assert bytes(arr[at:at + 4]) == b"\x28\xb5\x2f\xfd"
        fhd = arr[at + 4]
        hdr = 5 + (0 if fhd & 32 else 1) + ((fhd >> 5) & 1, 2, 4, 8)[fhd >> 6]
        arr[at + hdr] |= 6
        hit["page"] = sum(x.n_pages for x in descs[:1]) + d.n_pages - 1

    with ParquetFile(paths[("ZSTD", "1.0")]) as fz, oracle.open(paths[("NONE", "1.0")]) as of:
        rc, got = _batch(decoder, [(fz, 0), (fz, 1), (fz, 2)], tweak)
        assert rc == -2
        assert [g["status"] for g in got] == [0, -2, 0]
        m = re.search(r"chunk (\d+): decode failed \(status (-?\d+), page (\d+)\)", decoder.error())
        assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (1, -2, hit["page"]), decoder.error()
        for c in (0, 2):
            assert_chunk_equal(got[c], of.decode(0, c), f"neighbour c{c}")


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
    flat = {"i32_d", "i64_p", "f64_p", "flag", "s_d", "s_p"}

    def rows(p):
        with ParquetReader.streamContent(p, HydratorSupplier.constantly(Rows()), flat) as s:
            return s.collect()

    z, s = rows(paths[("ZSTD", "2.0")]), rows(paths[("SNAPPY", "2.0")])
    assert len(z) == ROWS and z == s
