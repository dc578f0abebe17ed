"""Kept dictionaries on whole files: the golden fixtures decoded with dictionaries=True (which chunks are kept is the
rule of include/pfloor.h applied to the page descriptors; materialize() of every chunk equals the .npz expectation),
the batch copy of a kept decode (equal to fetch, and strictly smaller than the expanding decode's), and
ParquetReader.streamContent(..., dictionaries=True), which must yield the rows of the default."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from golden_util import assert_chunk_equal, load_expected

pytestmark = pytest.mark.gpu

FILES = ("c2_lineitem", "c4_wide", "edge_types_v1", "edge_types_v2", "c1_flat_snappy_v2", "edge_encodings", "c5_nested")
DICT_ENCODINGS = (2, 8)   # PLAIN_DICTIONARY, RLE_DICTIONARY


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _rule(pf, rg, col):
    """The eligibility rule of pf_decode_row_group_dict on the chunk's page descriptors."""
    c = pf.columns[col]
    d = pf.chunk_desc(rg, col, 0)
    pages = [d.pages[i] for i in range(d.n_pages)]
    data = [p for p in pages if p.page_type in (0, 3)]
    return (c.max_rep == 0 and c.physical_type != 0 and any(p.page_type == 2 for p in pages) and len(data) > 0 and
            all(p.encoding in DICT_ENCODINGS for p in data))


@pytest.mark.parametrize("name", FILES)
def test_golden_kept(name, decoder):
    from pfloor.decoder import ParquetFile, decode_file, materialize
    path = os.path.join(GOLDEN, name + ".parquet")
    exp = load_expected(name)
    got = decode_file(path, decoder=decoder, dictionaries=True)
    assert got["_status"] == 0, got["_error"]
    kept = []
    with ParquetFile(path) as pf:
        for key, e in exp.items():
            g = got[key]
            want = _rule(pf, *key)
            assert ("indices" in g) == want, f"{name} {key} ({e['path']}): kept {'indices' in g}, by the rule {want}"
            if want:
                kept.append(key)
                assert g["width"] in (1, 2, 4) and g["width"] == (1 if g["dictionary"]["n_entries"] <= 256 else
                                                                  2 if g["dictionary"]["n_entries"] <= 65536 else 4), (name, key)
            assert_chunk_equal(materialize(g, pf.columns[key[1]].physical_type), e, f"{name} {key} ({e['path']})")
        print(f"{name}: {len(kept)} of {len(exp)} chunks kept")
        if name in ("edge_encodings", "c5_nested"):
            assert not kept, (name, kept)
        if name == "c2_lineitem":
            small = [c.index for c in pf.columns if c.path[0] in ("l_returnflag", "l_linestatus", "l_shipinstruct", "l_shipmode")]
            assert len(small) == 4
            for rg in range(pf.num_row_groups):
                for col in small:
                    g = got[(rg, col)]
                    assert "indices" in g and g["width"] == 1 and g["dictionary"]["n_entries"] <= 7, (rg, col)


def test_lineitem_batch_copy(decoder):
    """fetch_batch after a kept decode equals fetch, and the batch is strictly smaller than the expanding decode's."""
    from pfloor import _native
    from pfloor.decoder import ParquetFile
    path = os.path.join(GOLDEN, "c2_lineitem.parquet")
    sizes = {}
    with ParquetFile(path) as pf:
        cols = list(range(pf.num_columns))
        items, total = pf.plan(list(range(pf.num_row_groups)), cols)
        buf = decoder.staging(total)
        descs = []
        for rg, col, s, n, off in items:
            if n:
                pf.read_into(s, n, buf.ptr.value + off)
            descs.append(pf.chunk_desc(rg, col, off))
        types = [(pf.columns[col].physical_type, pf.columns[col].max_def, pf.columns[col].max_rep) for _rg, col, *_r in items]
        for tag, keep in (("expanded", None), ("kept", [True] * len(descs))):
            decoder.decode(descs, buf.ptr.value, max(total, 1), keep=keep)
            assert decoder.wait() == 0, decoder.error()
            n = C.c_size_t()
            _native.check(_native.lib().pf_batch_bytes(decoder.h, C.byref(n)), decoder.h, "pf_batch_bytes")
            sizes[tag] = n.value
            one = [decoder.fetch(i, *t) for i, t in enumerate(types)]
            batch = decoder.fetch_batch(types)
            batch_pageable = decoder.fetch_batch(types, pageable=True)
            for i, g in enumerate(one):
                for other in (batch[i], batch_pageable[i]):
                    assert set(g) == set(other), (tag, i)
                    for k, v in g.items():
                        if k == "dictionary":
                            for dk, dv in v.items():
                                assert np.array_equal(dv, other[k][dk]), (tag, i, dk)
                        else:
                            assert np.array_equal(v, other[k]), (tag, i, k)
            if keep:
                assert any("indices" in g for g in one)
    print(f"c2_lineitem pf_batch_bytes: kept {sizes['kept']}, expanded {sizes['expanded']}")
    assert sizes["kept"] < sizes["expanded"], sizes


class _Rows:
    """Hydrator that records every (heading, value) of every row."""

    def start(self):
        return []

    def add(self, target, heading, value):
        target.append((heading, value))
        return target

    def finish(self, target):
        return tuple(target)


@pytest.mark.parametrize("name", ("c2_lineitem", "ref_roundtrip", "edge_types_v2"))
def test_reader_rows(name):
    from pfloor.reader import HydratorSupplier, ParquetReader
    path = os.path.join(GOLDEN, name + ".parquet")
    rows, kept = {}, {}
    for flag in (False, True):
        with ParquetReader.streamContent(path, HydratorSupplier.constantly(_Rows()), dictionaries=flag) as s:
            rows[flag] = s.collect()
            # the cursors of the last row group: which of them read through a kept dictionary
            kept[flag] = {cur.col.path[0] for cur in s.reader.cursors if cur.indices is not None}
    print(f"{name}: columns read through a kept dictionary: {sorted(kept[True])}")
    assert not kept[False], (name, kept[False])
    if name == "c2_lineitem":   # the kept route ran: the small-dictionary string columns came as indices
        assert {"l_returnflag", "l_linestatus", "l_shipinstruct", "l_shipmode"} <= kept[True], kept[True]
    if name == "edge_types_v2":
        assert kept[True], name
    assert len(rows[True]) == len(rows[False]) and len(rows[False]) > 0
    for i, (a, b) in enumerate(zip(rows[False], rows[True])):
        assert len(a) == len(b), (name, i)
        for (ha, va), (hb, vb) in zip(a, b):
            assert ha == hb and type(va) is type(vb) and (va == vb or (va != va and vb != vb)), (name, i, ha, va, vb)
