"""Kept dictionaries on the GPU (pf_decode_row_group_dict; k_flat_ids, k_dict_offsets, k_dict_pack: pf_flat_ids.hip).

Every case of tests/dict_cases.py is a file assembled by tests/pagekit.py. It is decoded with its keep flags by the
product library and by the diagnostics build, and every chunk is checked three ways: the indices equal the ids the
case was built from (0 at null slots), the dictionary equals the entries it was built from, and materialize() of the
result equals the CPU oracle's decode of the same chunk bit for bit. A chunk the rule does not keep must come back
expanded and equal the oracle's arrays. Under the diagnostics build pf_debug_ids_counts = {blocks on the fast path,
pages on the slow path} must be what the rule in dict_cases predicts. A page with an id outside the dictionary must
give the status and the error of the expanding decode of the same file."""
import ctypes as C
import os

import numpy as np
import pytest

import dict_cases as DC
import pagekit as K
from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

TOTAL = [0, 0]   # fast blocks, slow pages seen by the cases of this module


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _ids_counts():
    """(blocks on the fast path, pages on the slow path) since the last call; diagnostics build only."""
    from pfloor import _native
    f = _native.lib().pf_debug_ids_counts
    f.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    buf = (C.c_ulonglong * 2)()
    assert f(buf, 1) == 0
    return int(buf[0]), int(buf[1])


def _decode(path, dec, keep, raw_null_keep=False):
    """Every chunk of row group 0 in one batch with the given keep flags (None: pf_decode_row_group;
    raw_null_keep: pf_decode_row_group_dict with keep == NULL). {(0, col): arrays, "_status", "_error", "_batch_bytes"}."""
    from pfloor import _native
    from pfloor.decoder import ParquetFile
    with ParquetFile(path) as pf:
        cols = list(range(pf.num_columns))
        items, total = pf.plan([0], cols)
        buf = dec.staging(total)
        descs = []
        for rg, col, s, n, off in items:
            if n:
                pf.read_into(s, n, buf.ptr.value + off)
            descs.append(pf.chunk_desc(rg, col, off))
        if raw_null_keep:
            arr = (_native.ChunkDesc * max(1, len(descs)))(*descs)
            _native.check(_native.lib().pf_decode_row_group_dict(dec.h, arr, len(descs), None, C.c_void_p(buf.ptr.value), max(total, 1), 0),
                          dec.h, "pf_decode_row_group_dict")
            dec.n_chunks = len(descs)
        else:
            dec.decode(descs, buf.ptr.value, max(total, 1), keep=keep)
        rc = dec.wait()
        out = {"_status": rc, "_error": dec.error() if rc else "", "_types": []}
        for i, col in enumerate(cols):
            c = pf.columns[col]
            out[(0, col)] = dec.fetch(i, c.physical_type, c.max_def, c.max_rep)
            out["_types"].append((c.physical_type, c.max_def, c.max_rep))
        n = C.c_size_t()
        _native.check(_native.lib().pf_batch_bytes(dec.h, C.byref(n)), dec.h, "pf_batch_bytes")
        out["_batch_bytes"] = n.value
        return out


def _same_arrays(a, b, where):
    assert set(a) == set(b), (where, sorted(a), sorted(b))
    for k, v in a.items():
        if k == "dictionary":
            _same_arrays(v, b[k], where + " dictionary")
        elif isinstance(v, np.ndarray):
            assert v.dtype == b[k].dtype and np.array_equal(v, b[k]), (where, k)
        else:
            assert v == b[k], (where, k, v, b[k])


def _check_chunk(g, spec, exp, where):
    from pfloor.decoder import INDEX_DTYPES, materialize
    assert g["status"] == 0, f"{where}: status {g['status']}"
    assert ("indices" in g) == spec.kept, f"{where}: kept {('indices' in g)}, by the rule {spec.kept}"
    if not spec.kept:
        assert_chunk_equal(g, exp, where)
        return
    iw = DC.index_width(spec.n_dict)
    want = spec.expected_indices()
    assert g["width"] == iw and g["indices"].dtype == INDEX_DTYPES[iw], f"{where}: index width {g['width']}"
    assert g["num_chars"] == 0 and "offsets" not in g and "chars" not in g and "values" not in g, where
    assert len(g["indices"]) == len(want), f"{where}: {len(g['indices'])} indices for {len(want)} slots"
    if not np.array_equal(g["indices"].astype(np.int64), want):
        bad = np.flatnonzero(g["indices"].astype(np.int64) != want)
        raise AssertionError(f"{where}: indices differ at slots {bad[:10]} (n={len(bad)}): {g['indices'][bad[:10]]} != {want[bad[:10]]}")
    d, ed = g["dictionary"], spec.expected_dictionary()
    assert d["n_entries"] == ed["n_entries"] and d["width"] == ed["width"], f"{where}: dictionary {d['n_entries']} x {d['width']}"
    for k in ("values", "offsets", "chars"):
        assert (k in d) == (k in ed), (where, k)
        if k in ed:
            assert d[k].dtype == ed[k].dtype and np.array_equal(d[k], ed[k]), f"{where}: dictionary {k} differs"
    assert_chunk_equal(materialize(g, spec.ptype), exp, where + " materialized")


def _write(case, oracle, tmp_path):
    specs = case.build(oracle.snappy_compress)
    chunks = [s.chunk for s in specs]
    data, _info = K.build_file(chunks, max(ch.num_entries for ch in chunks))
    path = os.path.join(str(tmp_path), "dict.parquet")
    with open(path, "wb") as fh:
        fh.write(data)
    with oracle.open(data=data) as of:
        exp = [of.decode(0, c) for c in range(len(chunks))]
    return specs, path, exp


@pytest.mark.parametrize("name", [n for n, c in DC.CASES.items() if not c.bad])
def test_keep_case(name, oracle, decoder, switches, tmp_path):
    from pfloor.decoder import GpuDecoder
    case = DC.CASES[name]
    specs, path, exp = _write(case, oracle, tmp_path)
    for c, s in enumerate(specs):   # the assembler's own expectation agrees with the oracle
        assert exp[c]["status"] == 0, (name, c, exp[c]["error"])
        assert_chunk_equal(exp[c], s.chunk.expected(), f"{name}: oracle against the construction, chunk {c}")
    keep = [s.keep for s in specs]
    got = _decode(path, decoder, keep)
    assert got["_status"] == 0, (name, got["_error"])
    for c, s in enumerate(specs):
        _check_chunk(got[(0, c)], s, exp[c], f"{name} [product library] chunk {c} ({s.chunk.name})")
    # the batch copy gives the same arrays
    batch = decoder.fetch_batch(got["_types"])
    for c in range(len(specs)):
        _same_arrays(got[(0, c)], batch[c], f"{name} fetch_batch chunk {c}")
    with switches(), GpuDecoder(0) as d:
        _ids_counts()
        dg = _decode(path, d, keep)
        counts = _ids_counts()
    want = (sum(s.counts()[0] for s in specs), sum(s.counts()[1] for s in specs))
    print(f"{name} [diagnostics build]: fast blocks {counts[0]}, slow pages {counts[1]}; by the rule {want}")
    assert dg["_status"] == 0, (name, dg["_error"])
    for c, s in enumerate(specs):
        _check_chunk(dg[(0, c)], s, exp[c], f"{name} [diagnostics build] chunk {c} ({s.chunk.name})")
    assert counts == want, f"{name}: fast blocks, slow pages {counts}, by the rule {want}"
    TOTAL[0] += counts[0]
    TOTAL[1] += counts[1]


@pytest.mark.parametrize("name", [n for n, c in DC.CASES.items() if c.bad])
def test_bad_id(name, oracle, decoder, switches, tmp_path):
    """An id equal to n_entries: status, error page and error text of the expanding decode; the good chunks intact."""
    from pfloor.decoder import GpuDecoder
    case = DC.CASES[name]
    specs, path, exp = _write(case, oracle, tmp_path)
    for c, s in enumerate(specs):
        assert (exp[c]["status"] != 0) == s.is_bad, f"{name}: the oracle on chunk {c}: {exp[c]['status']}"
    plain = _decode(path, decoder, None)
    kept = _decode(path, decoder, [True] * len(specs))
    with switches(), GpuDecoder(0) as d:
        diag = _decode(path, d, [True] * len(specs))
    for tag, got in (("product library", kept), ("diagnostics build", diag)):
        print(f"{name} [{tag}]: {got['_status']} {got['_error']!r}; expanding: {plain['_status']} {plain['_error']!r}")
        assert (got["_status"], got["_error"]) == (plain["_status"], plain["_error"]) and got["_status"] != 0, (name, tag)
        for c, s in enumerate(specs):
            assert got[(0, c)]["status"] == plain[(0, c)]["status"], (name, tag, c)
            if s.is_bad:
                assert got[(0, c)]["status"] == -2, (name, tag, c, got[(0, c)]["status"])
            else:
                _check_chunk(got[(0, c)], s, exp[c], f"{name} [{tag}] good chunk {c}")


def test_keep_null_and_all_zero_are_the_expanding_decode(oracle, decoder, tmp_path):
    """keep == NULL (pf_decode_row_group_dict itself) and keep all zero against pf_decode_row_group, array for array."""
    specs, path, exp = _write(DC.CASES["mixed-batch"], oracle, tmp_path)
    base = _decode(path, decoder, None)
    assert base["_status"] == 0, base["_error"]
    for tag, got in (("keep == NULL", _decode(path, decoder, None, raw_null_keep=True)),
                     ("keep all zero", _decode(path, decoder, [False] * len(specs)))):
        assert got["_status"] == 0 and got["_batch_bytes"] == base["_batch_bytes"], tag
        for c in range(len(specs)):
            _same_arrays(base[(0, c)], got[(0, c)], f"{tag} chunk {c}")
            assert_chunk_equal(got[(0, c)], exp[c], f"{tag} chunk {c}")
            assert decoder.dict_info(c).kept == 0
    kept = _decode(path, decoder, [s.keep for s in specs])
    print(f"mixed batch: {kept['_batch_bytes']} bytes kept, {base['_batch_bytes']} expanded")
    assert kept["_batch_bytes"] < base["_batch_bytes"]


def test_copy_rules(oracle, decoder, tmp_path):
    """pf_copy_column leaves offsets / chars buffers of a kept chunk alone; pf_copy_dictionary refuses a chunk that was
    not kept (PF_ERR_STATE) and a buffer that is too small (PF_ERR_CAPACITY, nothing copied); keep= takes no windows."""
    from pfloor import _native
    specs, path, _exp = _write(DC.CASES["mixed-batch"], oracle, tmp_path)
    _decode(path, decoder, [s.keep for s in specs])
    L = _native.lib()
    kept_str = next(c for c, s in enumerate(specs) if s.kept and s.ptype == K.BYTE_ARRAY)
    unkept = next(c for c, s in enumerate(specs) if not s.kept)
    ci, di = decoder.info(kept_str), decoder.dict_info(kept_str)
    assert di.kept == 1 and di.width == 0 and not ci.d_offsets and not ci.d_chars and ci.num_chars == 0
    o = _native.ColumnOut()
    vals = np.zeros(ci.num_slots * ci.width, np.uint8)
    offs, chars = np.full(8, 0x5a5a5a5a, np.int32), np.full(8, 0x5a, np.uint8)
    o.values, o.values_cap = vals.ctypes.data, vals.nbytes
    o.offsets, o.offsets_cap, o.chars, o.chars_cap = offs.ctypes.data, offs.nbytes, chars.ctypes.data, chars.nbytes
    assert L.pf_copy_column(decoder.h, kept_str, C.byref(o)) == 0
    assert (offs == 0x5a5a5a5a).all() and (chars == 0x5a).all() and np.array_equal(vals.astype(np.int64), specs[kept_str].expected_indices())
    do = _native.ColumnOut()
    small = np.full(di.n_entries, 0x5a5a5a5a, np.int32)           # one offset short
    dch = np.full(di.num_chars, 0x5a, np.uint8)
    do.offsets, do.offsets_cap, do.chars, do.chars_cap = small.ctypes.data, small.nbytes, dch.ctypes.data, dch.nbytes
    assert L.pf_copy_dictionary(decoder.h, kept_str, C.byref(do)) == -6
    assert (small == 0x5a5a5a5a).all() and (dch == 0x5a).all()
    assert L.pf_copy_dictionary(decoder.h, unkept, C.byref(do)) == -9
    assert decoder.dict_info(unkept).kept == 0 and decoder.dict_info(unkept).index_width == 0
    with pytest.raises(ValueError):
        decoder.decode([], 0, 1, windows=[], keep=[])
    with pytest.raises(ValueError):
        decoder.decode([], 0, 1, predicates=[], keep=[])


def test_dictionary_chars_overflow_reruns_the_batch(oracle, tmp_path):
    """The dictionary's chars count towards the chars arena's need. A fresh context sizes the arena from the page
    sizes: 16 MiB + twice the hint (the expanding chunk's data pages and the kept chunk's dictionary page, 12 MB), plus
    a quarter, about 51 MB. The expanding chunk's 44 MB of chars fit it, the kept chunk's 12 MB dictionary then does
    not: k_dict_offsets reports PF_ERR_CAPACITY, pf_wait runs the batch once more with 44 + 12 MB (+ 1 MiB) and both
    chunks come out right. Were the dictionary's chars left out of the need, the arena would not grow and the second
    run would fail the same way. (2000-byte entries: k_dict_pack copies each with the whole workgroup.)"""
    from pfloor.decoder import GpuDecoder
    rng = np.random.default_rng(101)
    big = DC.Spec("big", "binary", [bytes([65 + i]) * 400 for i in range(4)])
    for _ in range(5):
        big.page(rng.integers(0, 4, 22000), seed=1)
    big.keep = False
    entries = rng.integers(0, 256, (6000, 2000)).astype(np.uint8)
    kept = DC.Spec("kept", "binary", [entries[i].tobytes() for i in range(6000)])
    ids = rng.integers(0, 6000, 4097)
    ids[0], ids[-1] = 5999, 0
    kept.page(ids)
    specs = [big, kept]
    data, _info = K.build_file([s.chunk for s in specs], 110000)
    path = os.path.join(str(tmp_path), "overflow.parquet")
    with open(path, "wb") as fh:
        fh.write(data)
    with oracle.open(data=data) as of:
        exp = [of.decode(0, c) for c in range(2)]
    with GpuDecoder(0) as dec:
        got = _decode(path, dec, [s.keep for s in specs])
        reruns = dec.chars_reruns()
    print(f"chars overflow: status {got['_status']} {got['_error']!r}, reruns {reruns}")
    assert got["_status"] == 0, got["_error"]
    assert reruns == 1, reruns
    for c, s in enumerate(specs):
        _check_chunk(got[(0, c)], s, exp[c], f"chars overflow chunk {c}")
    assert got[(0, 1)]["dictionary"]["chars"].size == 12000000


def test_list_golden_is_not_kept(oracle, decoder):
    """tests/golden/list_prim.parquet: its list chunks (max_rep = 1) are decoded as ever, whatever is asked, with arrays
    equal to the oracle's expanded ones; the flat chunks beside them expand to the oracle's too."""
    from conftest import GOLDEN
    from pfloor.decoder import ParquetFile, decode_file, materialize
    path = os.path.join(GOLDEN, "list_prim.parquet")
    got = decode_file(path, decoder=decoder, dictionaries=True)
    assert got["_status"] == 0, got["_error"]
    nested = 0
    with oracle.open(path) as of, ParquetFile(path) as pf:
        for key, g in got.items():
            if not isinstance(key, tuple):
                continue
            col = pf.columns[key[1]]
            if col.max_rep > 0:
                nested += 1
                assert "indices" not in g, key
                assert_chunk_equal(g, of.decode(*key), f"list_prim {key}")
            else:
                assert_chunk_equal(materialize(g, col.physical_type), of.decode(*key), f"list_prim {key}")
    assert nested > 0


def test_both_paths_ran(oracle, switches, tmp_path):
    """Over the module both counters are non-zero (run alone, this test decodes one case of each path itself)."""
    from pfloor.decoder import GpuDecoder
    if not (TOTAL[0] and TOTAL[1]):
        for name in ("counts-int32", "more-runs-than-the-table"):
            specs, path, _exp = _write(DC.CASES[name], oracle, tmp_path)
            with switches(), GpuDecoder(0) as d:
                _ids_counts()
                assert _decode(path, d, [s.keep for s in specs])["_status"] == 0
                counts = _ids_counts()
            TOTAL[0] += counts[0]
            TOTAL[1] += counts[1]
    print(f"k_flat_ids over the module: fast blocks {TOTAL[0]}, slow pages {TOTAL[1]}")
    assert TOTAL[0] > 0 and TOTAL[1] > 0, TOTAL
