"""ParquetWriter(codec=ZSTD): files whose page sections are ZSTD frames compressed on the GPU (k_zstd_compress;
DESIGN 4.31). A flat schema of all six writable types, required and optional with 30 % nulls, 45,000 rows in one
row group (two full pages and a short one) with one chunk whose dictionary falls back, a file of one row and a
file with an all-null column; without options and with every option at once. pyarrow (libzstd) and this
project's reader return the input, the footer says ZSTD, pf_scan_pages verifies every page CRC, and the same
data written with SNAPPY decodes to the same rows."""
import numpy as np
import pytest

from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

ALL_OPTIONS = dict(delta_fallback=True, hybrid_runs=True, statistics=True, page_checksums=True,
                   bloom_filters={"i64_req": {"bytes": 1024}})
OPTIONS = pytest.mark.parametrize("options", [{}, ALL_OPTIONS], ids=["plain", "all_options"])
PF_ERR_UNSUPPORTED_CODEC = -4


@pytest.fixture(scope="module")
def dec():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _table(n, seed, all_null=False):
    """(schema, write_columns input, {name: (kind, values, present)}) for n rows."""
    from pfloor import writer as W
    rng = np.random.default_rng(seed)
    numeric = {"bool": (W.BOOLEAN, lambda: rng.integers(0, 2, n).astype(np.uint8)),
               "i32": (W.INT32, lambda: rng.integers(-500, 500, n).astype(np.int32)),
               "i64": (W.INT64, lambda: (10**12 + np.cumsum(rng.integers(0, 9, n))).astype(np.int64)),
               "f32": (W.FLOAT, lambda: rng.integers(0, 2000, n).astype(np.float32) / 4),
               "f64": (W.DOUBLE, lambda: np.round(rng.normal(100.0, 20.0, n), 2))}
    fields, cols, exp = [], {}, {}
    for opt in (False, True):
        present = (rng.random(n) >= (1.0 if all_null else 0.3)) if opt else np.ones(n, bool)
        bits = np.packbits(present, bitorder="little")
        for name, (ptype, make) in numeric.items():
            vals = np.where(present, make(), 0).astype(make().dtype)
            key = f"{name}_{'opt' if opt else 'req'}"
            fields.append((W.optional if opt else W.required)(ptype).named(key))
            cols[key] = (vals, bits) if opt else vals
            exp[key] = ("num", vals, present)
        words = [(b"word-%d" % (i % 211)) if present[i] else b"" for i in range(n)]
        key = f"str_{'opt' if opt else 'req'}"
        offs = np.zeros(n + 1, np.int32)
        np.cumsum([len(x) for x in words], out=offs[1:])
        chars = np.frombuffer(b"".join(words) or b"\0", np.uint8)
        fields.append((W.optional if opt else W.required)(W.BINARY).as_string().named(key))
        cols[key] = (offs, chars, bits) if opt else (offs, chars)
        exp[key] = ("str", words, present)
    # distinct 30-byte strings: 34 bytes a dictionary entry, over the 1 MiB dictionary page from 30,841 rows on
    uniq = [b"unique-value-%017d" % (i * 7919) for i in range(n)]
    offs = np.arange(n + 1, dtype=np.int32) * 30
    fields.append(W.required(W.BINARY).as_string().named("uniq"))
    cols["uniq"] = (offs, np.frombuffer(b"".join(uniq), np.uint8))
    exp["uniq"] = ("str", uniq, np.ones(n, bool))
    return W.MessageType("flat", *fields), cols, exp


def _write(dec, path, table, n, codec, options):
    from pfloor import writer as W
    schema, cols, _exp = table
    w = W.ParquetWriter(schema, path, None, decoder=dec, codec=codec, **options)
    w.write_columns(cols, n)
    chunks = list(w.last_chunks)
    w.close()
    return chunks


def _check_pyarrow(path, exp, n, codec_name, checksums):
    pq = pytest.importorskip("pyarrow.parquet")
    t = pq.read_table(path, page_checksum_verification=True) if checksums else pq.read_table(path)
    assert t.num_rows == n
    md = pq.ParquetFile(path).metadata
    assert md.num_row_groups == 1
    for c in range(md.num_columns):
        assert md.row_group(0).column(c).compression == codec_name, (c, md.row_group(0).column(c).compression)
    for name, (kind, vals, present) in exp.items():
        col = t.column(name).combine_chunks()
        assert np.array_equal(~np.asarray(col.is_null()), present), name
        if kind == "num":
            got = col.drop_null().to_numpy(zero_copy_only=False)
            want = vals[present].astype(bool) if name.startswith("bool") else vals[present]
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), name
        else:
            assert [x.encode() for x in col.drop_null().to_pylist()] == [w for w, p in zip(vals, present) if p], name


def _check_crcs(dec, path, n):
    from pfloor.decoder import ParquetFile
    with open(path, "rb") as f:
        data = f.read()
    with ParquetFile(path) as pf:
        ranges = [pf.chunk_range(0, c) for c in range(pf.num_columns)]
    rc, res = dec.scan_pages(data, [(s, k, n) for s, k in ranges], verify_crc=True)
    assert rc == 0
    for c, (status, err_page, crc_pages, pages) in enumerate(res):
        assert (status, err_page) == (0, -1), c
        assert crc_pages == len(pages) >= 1, (c, crc_pages, len(pages))


def _check_files(dec, tmp_path, table, n, options):
    """The table written with ZSTD and with SNAPPY: pyarrow reads the input out of both, the footer names the
    codec, this project's reader returns the same chunks from both, every page CRC verifies."""
    from pfloor import writer as W
    from pfloor.decoder import decode_file
    pz, ps = str(tmp_path / "zstd.parquet"), str(tmp_path / "snappy.parquet")
    chunks = _write(dec, pz, table, n, W.ZSTD, options)
    assert _write(dec, ps, table, n, W.SNAPPY, options) == chunks   # the codec changes no encoding decision
    checksums = bool(options.get("page_checksums"))
    _check_pyarrow(pz, table[2], n, "ZSTD", checksums)
    _check_pyarrow(ps, table[2], n, "SNAPPY", checksums)
    gz, gs = decode_file(pz, decoder=dec), decode_file(ps, decoder=dec)
    assert gz["_status"] == 0, gz["_error"]
    assert gs["_status"] == 0, gs["_error"]
    for c in range(len(table[2])):
        assert_chunk_equal(gz[(0, c)], gs[(0, c)], f"col {c} ZSTD against SNAPPY")
    if checksums:
        _check_crcs(dec, pz, n)
    return chunks


@OPTIONS
def test_three_pages_all_types(dec, tmp_path, options):
    n = 45_000
    chunks = _check_files(dec, tmp_path, _table(n, 1), n, options)
    assert chunks[-1][2] == 1, chunks[-1]                # uniq: the dictionary fell back
    assert any(c[0] > 0 for c in chunks[:-1]), chunks    # and others are dictionary-encoded


@OPTIONS
def test_one_row(dec, tmp_path, options):
    _check_files(dec, tmp_path, _table(1, 2), 1, options)


@OPTIONS
def test_all_null_optional_columns(dec, tmp_path, options):
    n = 3000
    table = _table(n, 3, all_null=True)
    assert not table[2]["i64_opt"][2].any()
    _check_files(dec, tmp_path, table, n, options)


def test_other_codecs_are_still_refused(dec):
    from pfloor import writer as W
    vals = np.arange(100, dtype=np.int64)
    for codec in (2, 5):   # GZIP, LZ4
        with pytest.raises(W.PfError) as e:
            W.GpuColumnEncoder(dec).encode(W.Field("v", W.INT64, False), vals, None, 100, codec=codec)
        assert e.value.code == PF_ERR_UNSUPPORTED_CODEC
    out = W.GpuColumnEncoder(dec).encode(W.Field("v", W.INT64, False), vals, None, 100, codec=W.ZSTD)
    assert out.codec == W.ZSTD and out.snappy_in > 0 and out.snappy_out > 0
