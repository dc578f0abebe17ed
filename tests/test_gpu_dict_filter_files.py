"""Kept dictionaries under rows= and where= on whole files: decode_file(dictionaries=True, rows=..., where=...) on the
golden fixtures and on one file of the GPU writer with a page index and a Bloom filter must give, after materialize(),
what the same call gives without the flag (the indexed route of ParquetFile.plan_rows included), and
ParquetReader.streamContent(..., dictionaries=True, rows=..., where=...) must yield the rows and filter_stats of the run
without the flag while its cursors hold indices."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

DICT_ENCODINGS = (2, 8)   # PLAIN_DICTIONARY, RLE_DICTIONARY


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _first_value(path, decoder, name):
    """(column index, physical type, the first present value of the named column in row group 0 as Python value)."""
    from pfloor.decoder import ParquetFile, decode_file
    with ParquetFile(path) as pf:
        col = next(c for c in pf.columns if c.path[0] == name)
    g = decode_file(path, row_groups=[0], columns=[col.index], decoder=decoder)[(0, col.index)]
    n = g["num_slots"]
    valid = np.unpackbits(g["validity"], bitorder="little")[:n].astype(bool) if "validity" in g else np.ones(n, bool)
    s = int(np.flatnonzero(valid)[len(np.flatnonzero(valid)) // 2])
    if col.physical_type == 6:
        return col, bytes(g["chars"][g["offsets"][s]:g["offsets"][s + 1]])
    dt = {1: np.int32, 2: np.int64, 4: np.float32, 5: np.float64}[col.physical_type]
    return col, g["values"].view(dt)[s].item()


def _compare(path, decoder, label, **kw):
    """decode_file with and without dictionaries=True; returns the keys that came back kept."""
    from pfloor.decoder import ParquetFile, decode_file, materialize
    plain = decode_file(path, decoder=decoder, **kw)
    got = decode_file(path, decoder=decoder, dictionaries=True, **kw)
    assert got["_status"] == plain["_status"] == 0, (label, got["_error"], plain["_error"])
    assert set(got) == set(plain), label
    kept = []
    with ParquetFile(path) as pf:
        for key, g in got.items():
            if not isinstance(key, tuple):
                continue
            pt = pf.columns[key[1]].physical_type
            if "indices" in g:
                kept.append(key)
                assert g["num_chars"] == 0 and g["width"] in (1, 2, 4), (label, key)
            assert_chunk_equal(materialize(g, pt), plain[key], f"{label} {key}")
    if "_selection" in plain:
        assert got["_selection"][0] == plain["_selection"][0] and np.array_equal(got["_selection"][1], plain["_selection"][1]), label
        assert got["_range"] == plain["_range"], label
    return kept


@pytest.mark.parametrize("name,pred_col", [("c2_lineitem", "l_shipmode"), ("c2_lineitem", "l_quantity"), ("c1_flat_snappy_v2", None),
                                           ("edge_types_v2", None), ("c4_wide", None)])
def test_decode_file_rows_and_where(name, pred_col, decoder):
    from pfloor.decoder import ParquetFile
    from pfloor.predicate import Eq, NotNull, Range
    path = os.path.join(GOLDEN, name + ".parquet")
    with ParquetFile(path) as pf:
        rows = pf.row_group_rows(0)
        if pred_col is None:   # the first flat column with a range-able type
            pred_col = next(c.path[0] for c in pf.columns if c.max_rep == 0 and c.physical_type in (1, 2, 4, 5, 6))
    lo, hi = rows // 5 + 3, rows - rows // 7
    kept = _compare(path, decoder, f"{name} rows", row_groups=[0], rows=(lo, hi))
    col, v = _first_value(path, decoder, pred_col)
    for label, where in (("eq", [Eq(pred_col, v)]), ("range + not null", [Range(pred_col, v, None), NotNull(pred_col)]),
                         ("below", [Range(pred_col, None, v)])):
        kept += _compare(path, decoder, f"{name} where {label}", row_groups=[0], where=where)
        kept += _compare(path, decoder, f"{name} rows + where {label}", row_groups=[0], rows=(lo, hi), where=where)
    print(f"{name}: {len(kept)} kept chunks over the calls, predicate column {pred_col} = {v!r}")
    assert kept, name
    if pred_col == "l_shipmode":   # the predicate chunk itself was kept: its predicate went through the dictionary
        assert any(k[1] == col.index for k in kept)


class _Rows:
    def start(self):
        return []

    def add(self, target, heading, value):
        target.append((heading, value))
        return target

    def finish(self, target):
        return tuple(target)


def _collect(path, **kw):
    from pfloor.reader import HydratorSupplier, ParquetReader
    with ParquetReader.streamContent(path, HydratorSupplier.constantly(_Rows()), **kw) as s:
        got = s.collect()
        held = {cur.col.path[0] for cur in (s.reader.cursors or []) if cur.indices is not None}
        return got, dict(s.reader.filter_stats), held


def _same_rows(a, b, label):
    assert len(a) == len(b), (label, len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y), (label, i)
        for (hx, vx), (hy, vy) in zip(x, y):
            assert hx == hy and type(vx) is type(vy) and (vx == vy or (vx != vx and vy != vy)), (label, i, hx, vx, vy)


def test_reader_lineitem(decoder):
    from pfloor.predicate import Eq, Range
    path = os.path.join(GOLDEN, "c2_lineitem.parquet")
    _col, mode = _first_value(path, decoder, "l_shipmode")
    whole, _s, _h = _collect(path)
    n = len(whole)
    small = {"l_returnflag", "l_linestatus", "l_shipinstruct", "l_shipmode"}
    for label, kw in (("rows", {"rows": (n // 7, n - n // 5)}), ("where", {"where": [Eq("l_shipmode", mode)]}),
                      ("rows + where", {"rows": (n // 7, n - n // 5), "where": [Eq("l_shipmode", mode), Range("l_quantity", None, 25)]})):
        a, sa, ha = _collect(path, **kw)
        b, sb, hb = _collect(path, dictionaries=True, **kw)
        print(f"c2_lineitem {label}: {len(a)} rows, stats {sb}, cursors over indices: {sorted(hb)}")
        _same_rows(a, b, label)
        assert sa == sb and len(a) > 0 and not ha, label
        assert small <= hb, (label, hb)   # the last row group was windowed or filtered and still came as indices


def test_reader_written_file(decoder, tmp_path):
    """One file of the GPU writer with page index and Bloom filter: pruning is untouched, the rows are the same."""
    from pfloor import writer as W
    from pfloor.decoder import ParquetFile
    from pfloor.predicate import Eq, NotNull, Range
    rows, groups = 3000, 3
    schema = W.MessageType("dictfilter", W.required(W.INT64).named("k"), W.optional(W.DOUBLE).named("d"),
                           W.optional(W.BINARY).as_string().named("s"), W.required(W.INT32).named("m"))
    path = str(tmp_path / "written.parquet")
    w = W.ParquetWriter(schema, path, None, decoder=decoder, page_index=True, page_rows=500, bloom_filters={"k": True})
    rng = np.random.default_rng(5)
    ks = []
    for g in range(groups):
        k = 1_000_000 * g + 3 * np.arange(rows, dtype=np.int64) + 7
        d = np.round(rng.random(rows) * 16) / 16
        dv = rng.random(rows) >= 0.2
        sv = rng.random(rows) >= 0.25
        words = [b"s%d" % (i % 23) for i in range(rows)]
        offs = np.zeros(rows + 1, np.int32)
        np.cumsum([len(x) if ok else 0 for x, ok in zip(words, sv)], out=offs[1:])
        chars = np.frombuffer(b"".join(x for x, ok in zip(words, sv) if ok), np.uint8)
        w.write_columns({"k": k, "d": (d, np.packbits(dv, bitorder="little")), "s": (offs, chars, np.packbits(sv, bitorder="little")),
                         "m": (np.arange(rows) % 300).astype(np.int32)}, rows)
        ks += [int(x) for x in k]
    w.close()
    with ParquetFile(path) as pf:   # which columns the rule keeps when a row group is read whole
        rule = set()
        for c in pf.columns:
            dsc = pf.chunk_desc(0, c.index, 0)
            pages = [dsc.pages[i] for i in range(dsc.n_pages)]
            data = [p for p in pages if p.page_type in (0, 3)]
            if c.physical_type != 0 and any(p.page_type == 2 for p in pages) and data and all(p.encoding in DICT_ENCODINGS for p in data):
                rule.add(c.path[0])
    print(f"written file: dictionary-encoded throughout: {sorted(rule)}")
    assert {"s", "m"} <= rule, rule
    at = rows + 1234
    for label, kw in (("eq on the indexed key", {"where": [Eq("k", ks[at])]}), ("absent key (Bloom)", {"where": [Eq("k", ks[at] + 1)]}),
                      ("string range", {"where": [Range("s", "s10", "s19"), NotNull("d")]}),
                      ("rows", {"rows": (700, 2 * rows + 900)}),
                      ("rows + where", {"rows": (700, 2 * rows + 900), "where": [Range("m", 10, 200), Eq("s", "s7")]})):
        a, sa, _ha = _collect(path, **kw)
        b, sb, hb = _collect(path, dictionaries=True, **kw)
        print(f"written file {label}: {len(a)} rows, stats {sb}, cursors over indices: {sorted(hb)}")
        _same_rows(a, b, label)
        assert sa == sb, (label, sa, sb)
        if a:
            assert {"s", "m"} <= hb, (label, hb)
    for kw in ({"rows": (100, 2100)}, {"where": [Range("m", 10, 200), Range("s", "s1", "s5")]},
               {"rows": (100, 2100), "where": [Eq("s", "s3")]}):
        kept = _compare(path, decoder, f"written file {kw}", row_groups=[1], **kw)
        assert {2, 3} <= {k[1] for k in kept}, kept
