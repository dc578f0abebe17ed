"""Windows and predicates over kept dictionaries on the GPU (pf_decode_row_group_dict_filter; k_sel_dict and
k_sel_mask_dict: csrc/pf_filter_dict.hip; the kept form in k_win_copy, k_sel_prep and k_sel_gather).

Every batch of tests/dict_filter_cases.py is a file assembled by tests/pagekit.py and run through the C ABI under the
product library and under the diagnostics build. Every query is checked three ways: indices, validity and counts
against the numpy expectation, bit exact, padding bits included; the dictionary against the unfiltered kept decode of
the same file; materialize() of the result and selection() against what pf_decode_row_group_filter (no keep flags)
returns for the same call, which is itself checked against the numpy reference over the oracle's arrays. Every chunk
the rule keeps must report kept = 1, and under the diagnostics build pf_debug_sel_dict_counts = {predicates resolved
through a dictionary, dictionary entries evaluated} must be the number of RANGE predicates on kept chunks and the sum
of their dictionaries' sizes: nothing fell back to expanding."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import dict_cases as DC
import dict_filter_cases as FD
import filter_cases as FC
import pagekit as K
import window_cases as WC

pytestmark = pytest.mark.gpu

INVALID_ARG, CORRUPT, UNSUPPORTED_TYPE, STATE = -1, -2, -7, -9


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _counts():
    """(predicates resolved through a dictionary, entries evaluated) since the last call; diagnostics build only."""
    from pfloor import _native
    f = _native.lib().pf_debug_sel_dict_counts
    f.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    buf = (C.c_ulonglong * 2)()
    assert f(buf, 1) == 0
    return int(buf[0]), int(buf[1])


class _File:
    """A batch written to a file, its chunks read into a decoder's staging buffer once per decoder."""

    def __init__(self, specs, tmp_path, oracle=None, name="dictfilter.parquet"):
        self.specs = specs
        chunks = [s.chunk for s in specs]
        data, _info = K.build_file(chunks, max(ch.num_entries for ch in chunks))
        self.path = os.path.join(str(tmp_path), name)
        with open(self.path, "wb") as fh:
            fh.write(data)
        self.exp = None
        if oracle is not None:
            with oracle.open(data=data) as of:
                self.exp = [of.decode(0, c) for c in range(len(chunks))]

    def run(self, dec, how, keep=None, windows=None, preds=None):
        """how: "kept" pf_decode_row_group_dict_filter (GpuDecoder.decode_kept) | "plain" the entry points without keep
        flags (GpuDecoder.decode). preds: [(chunk, op, lo, hi)] with Python values."""
        from pfloor.decoder import ParquetFile
        with ParquetFile(self.path) as pf:
            cols = list(range(pf.num_columns))
            items, total = pf.plan([0], cols)
            buf = dec.staging(total)
            descs = []
            for rg, col, s, n, off in items:
                if n:
                    pf.read_into(s, n, buf.ptr.value + off)
                descs.append(pf.chunk_desc(rg, col, off))
            bound = None
            if preds:
                bound = [(c, op, FD.bound_bytes(self.specs[c].ptype, lo), FD.bound_bytes(self.specs[c].ptype, hi))
                         for c, op, lo, hi in preds]
            if how == "kept":
                dec.decode_kept(descs, buf.ptr.value, max(total, 1), keep=keep, windows=windows, predicates=bound)
            else:
                extra = {}
                if windows is not None:
                    extra["windows"] = windows
                if bound:
                    extra["predicates"] = bound
                dec.decode(descs, buf.ptr.value, max(total, 1), **extra)
            rc = dec.wait()
            out = {"_status": rc, "_error": dec.error() if rc else "", "_types": [], "_kept": []}
            for i, col in enumerate(cols):
                c = pf.columns[col]
                out[i] = dec.fetch(i, c.physical_type, c.max_def, c.max_rep)
                out["_types"].append((c.physical_type, c.max_def, c.max_rep))
                out["_kept"].append(dec.dict_info(i).kept)
            if preds:
                out["_selection"] = dec.selection()
            return out


def _same_dictionary(d, e, where):
    assert set(d) == set(e), (where, sorted(d), sorted(e))
    for k, v in e.items():
        if isinstance(v, np.ndarray):
            assert d[k].dtype == v.dtype and np.array_equal(d[k], v), f"{where}: dictionary {k} differs"
        else:
            assert d[k] == v, (where, k, d[k], v)


def _check_query(f, got, plain, base, ref, where):
    """got: the kept run; plain: the same call without keep flags; base: the unfiltered kept decode; ref: FD.reference."""
    from pfloor.decoder import INDEX_DTYPES, materialize
    rows_in, idx, expanded, kept = ref
    if idx is not None:
        for tag, g in (("no keep", plain), ("kept", got)):
            gin, grows = g["_selection"]
            assert gin == rows_in and grows.dtype == np.int32 and np.array_equal(grows, idx), f"{where} [{tag}]: selection"
    for c, s in enumerate(f.specs):
        w = f"{where} chunk {c} ({s.chunk.name})"
        assert got["_kept"][c] == int(s.kept), f"{w}: kept {got['_kept'][c]}, by the rule {int(s.kept)}"
        if expanded[c] is None:   # the window does not fit this chunk
            assert got[c]["status"] == plain[c]["status"] == INVALID_ARG, (w, got[c]["status"], plain[c]["status"])
            continue
        assert plain[c]["status"] == 0 and got[c]["status"] == 0, (w, plain[c]["status"], got[c]["status"], got["_error"])
        WC.assert_window_equal(plain[c], expanded[c], w + " [no keep] against the reference")
        g = got[c]
        if not s.kept:
            assert "indices" not in g, w
            WC.assert_window_equal(g, plain[c], w + " [expanded beside kept chunks]")
            for k in WC.ARRAYS:
                assert (k in g) == (k in plain[c]), (w, k)
            continue
        e = kept[c]
        iw = DC.index_width(s.n_dict)
        assert g["width"] == iw and g["indices"].dtype == INDEX_DTYPES[iw], f"{w}: index width {g['width']}"
        assert g["num_chars"] == 0 and "offsets" not in g and "chars" not in g and "values" not in g, w
        for k in ("num_entries", "num_slots", "num_values", "num_rows"):
            assert g[k] == e[k], f"{w}: {k} {g[k]} != {e[k]}"
        if not np.array_equal(g["indices"].astype(np.int64), e["indices"]):
            bad = np.flatnonzero(g["indices"].astype(np.int64) != e["indices"])
            raise AssertionError(f"{w}: indices differ at slots {bad[:10]} (n={len(bad)}): {g['indices'][bad[:10]]} != {e['indices'][bad[:10]]}")
        assert ("validity" in g) == ("validity" in e), w
        if "validity" in e:
            assert np.array_equal(g["validity"], e["validity"]), f"{w}: validity (padding bits included)"
        _same_dictionary(g["dictionary"], base[c]["dictionary"], w)
        m = materialize(g, s.ptype)
        WC.assert_window_equal(m, plain[c], w + " materialized against the filter without keep")
        assert m["num_chars"] == plain[c]["num_chars"] and m["width"] == plain[c]["width"], w


def _expected_counts(specs, preds):
    on_kept = [c for c, op, _lo, _hi in preds if op == FD.RANGE and specs[c].kept]
    return len(on_kept), sum(specs[c].n_dict for c in on_kept)


@pytest.mark.parametrize("name", list(FD.BATCHES))
def test_batch(name, oracle, decoder, switches, tmp_path):
    from pfloor.decoder import GpuDecoder
    specs, windows, queries = FD.BATCHES[name].build(oracle.snappy_compress)
    f = _File(specs, tmp_path, oracle)
    exp = []
    for c, s in enumerate(specs):   # the assembler's own expectation agrees with the oracle
        assert f.exp[c]["status"] == 0, (name, c, f.exp[c]["error"])
        WC.assert_window_equal(f.exp[c], s.chunk.expected(), f"{name}: oracle against the construction, chunk {c}")
        exp.append(FD.canon(s, f.exp[c]))
    keep = [s.keep for s in specs]
    base = _base(f, decoder, keep)   # the unfiltered kept decode: the dictionaries every query must return
    refs = [FD.reference(specs, exp, windows, preds) for _l, preds in queries]
    for (label, preds), ref in zip(queries, refs):
        plain = f.run(decoder, "plain", windows=windows, preds=preds)
        got = f.run(decoder, "kept", keep=keep, windows=windows, preds=preds)
        _check_query(f, got, plain, base, ref, f"{name} / {label} [product library]")
    total = [0, 0]
    with switches(), GpuDecoder(0) as d:
        dbase = _base(f, d, keep)
        for (label, preds), ref in zip(queries, refs):
            plain = f.run(d, "plain", windows=windows, preds=preds)
            _counts()
            got = f.run(d, "kept", keep=keep, windows=windows, preds=preds)
            counts = _counts()
            _check_query(f, got, plain, dbase, ref, f"{name} / {label} [diagnostics build]")
            want = _expected_counts(specs, preds)
            assert counts == want, f"{name} / {label}: resolved through a dictionary, entries evaluated {counts}, expected {want}"
            total[0] += counts[0]
            total[1] += counts[1]
    print(f"{name}: {len(queries)} queries, {total[0]} predicates resolved through a dictionary, {total[1]} entries evaluated")


def _base(f, dec, keep):
    """The unfiltered kept decode (pf_decode_row_group_dict) of the file."""
    from pfloor.decoder import ParquetFile
    with ParquetFile(f.path) as pf:
        cols = list(range(pf.num_columns))
        items, total = pf.plan([0], cols)
        buf = dec.staging(total)
        descs = []
        for rg, col, s, n, off in items:
            if n:
                pf.read_into(s, n, buf.ptr.value + off)
            descs.append(pf.chunk_desc(rg, col, off))
        dec.decode(descs, buf.ptr.value, max(total, 1), keep=keep)
        rc = dec.wait()
        assert rc == 0, dec.error()
        return [dec.fetch(i, pf.columns[c].physical_type, pf.columns[c].max_def, pf.columns[c].max_rep) for i, c in enumerate(cols)]


def _same_arrays(a, b, where):
    assert set(a) == set(b), (where, sorted(a), sorted(b))
    for k, v in a.items():
        if k == "dictionary":
            _same_dictionary(v, b[k], where)
        elif isinstance(v, np.ndarray):
            assert v.dtype == b[k].dtype and np.array_equal(v, b[k]), (where, k)
        else:
            assert v == b[k], (where, k, v, b[k])


def test_equivalences(oracle, decoder, tmp_path):
    """keep == NULL is pf_decode_row_group_filter; no windows and no predicates is pf_decode_row_group_dict, the batch
    copies included. Array for array."""
    from pfloor import _native
    specs, windows, queries = FD.BATCHES["windows-and-predicates"].build(oracle.snappy_compress)
    f = _File(specs, tmp_path)
    keep = [s.keep for s in specs]
    for label, preds in queries:
        a = f.run(decoder, "plain", windows=windows, preds=preds)
        b = f.run(decoder, "kept", keep=None, windows=windows, preds=preds)
        assert a["_status"] == b["_status"] == 0 and b["_kept"] == [0] * len(specs), label
        assert a["_selection"][0] == b["_selection"][0] and np.array_equal(a["_selection"][1], b["_selection"][1]), label
        for c in range(len(specs)):
            _same_arrays(a[c], b[c], f"keep == NULL / {label} chunk {c}")
    base = _base(f, decoder, keep)
    n0 = C.c_size_t()
    _native.check(_native.lib().pf_batch_bytes(decoder.h, C.byref(n0)), decoder.h, "pf_batch_bytes")
    got = f.run(decoder, "kept", keep=keep)
    n1 = C.c_size_t()
    _native.check(_native.lib().pf_batch_bytes(decoder.h, C.byref(n1)), decoder.h, "pf_batch_bytes")
    assert got["_status"] == 0 and n0.value == n1.value and got["_kept"] == [int(s.kept) for s in specs]
    batch = decoder.fetch_batch(got["_types"])
    for c in range(len(specs)):
        _same_arrays(base[c], got[c], f"no windows, no predicates chunk {c}")
        _same_arrays(got[c], batch[c], f"fetch_batch chunk {c}")
    ident = f.run(decoder, "kept", keep=keep, windows=[(0, -1)] * len(specs))     # identity windows: still that decode
    _native.check(_native.lib().pf_batch_bytes(decoder.h, C.byref(n1)), decoder.h, "pf_batch_bytes")
    assert n1.value == n0.value
    for c in range(len(specs)):
        _same_arrays(base[c], ident[c], f"identity windows chunk {c}")


@pytest.mark.parametrize("name", ["bad-id-packed-middle-block", "bad-id-rle-first-block", "bad-id-packed-last-block"])
def test_bad_id(name, oracle, decoder, switches, tmp_path):
    """An id equal to n_entries. In a predicate chunk: every chunk fails with the status, page and text of the expanding
    filter. In a payload chunk: only that chunk fails. After either the batch copies are PF_ERR_STATE."""
    from pfloor import _native
    from pfloor.decoder import GpuDecoder
    specs = DC.CASES[name].build(oracle.snappy_compress)
    f = _File(specs, tmp_path, oracle)
    keep = [True] * len(specs)
    bad = [c for c, s in enumerate(specs) if s.is_bad]
    good = [c for c, s in enumerate(specs) if not s.is_bad]
    L = _native.lib()

    def both(dec, preds, tag):
        plain = f.run(dec, "plain", preds=preds)
        got = f.run(dec, "kept", keep=keep, preds=preds)
        print(f"{name} [{tag}]: kept {got['_status']} {got['_error']!r}; expanding {plain['_status']} {plain['_error']!r}")
        assert (got["_status"], got["_error"]) == (plain["_status"], plain["_error"]) and got["_status"] == CORRUPT, tag
        for c in range(len(specs)):
            assert got[c]["status"] == plain[c]["status"], (tag, c, got[c]["status"], plain[c]["status"])
        n = C.c_size_t()
        assert L.pf_batch_bytes(dec.h, C.byref(n)) == STATE
        assert L.pf_copy_batch_async(dec.h, None, 0) == STATE
        ci, di, host = _native.ColumnInfo(), _native.DictInfo(), (C.c_uint8 * 8)()
        assert L.pf_column_info_host(dec.h, 0, host, C.byref(ci)) == STATE and L.pf_dict_info_host(dec.h, 0, host, C.byref(di)) == STATE
        return got, plain

    def run(dec, tag):
        for c in bad:      # the predicate chunk is the bad one: every chunk takes its status
            ptype = specs[c].ptype
            got, _plain = both(dec, [(c, FD.RANGE, b"" if ptype == K.BYTE_ARRAY else -2 ** 62, None)], f"{tag}, predicate on bad chunk {c}")
            assert all(got[k]["status"] == CORRUPT for k in range(len(specs))), tag
        c0 = good[1]       # a payload chunk is bad: only it fails
        lo = np.ascontiguousarray(specs[c0].dvals).view(np.int64).ravel()[3].item()
        preds = [(c0, FD.RANGE, lo, None)]
        got, plain = both(dec, preds, f"{tag}, predicate on good chunk {c0}")
        exp = [FD.canon(s, e) if e["status"] == 0 else None for s, e in zip(specs, f.exp)]
        mask = FC.eval_predicates([(exp[c0], specs[c0].ptype)], [(0, FD.RANGE, lo, None)])
        idx = np.flatnonzero(mask)
        assert np.array_equal(got["_selection"][1], idx) and 0 < len(idx) < len(mask)
        for c, s in enumerate(specs):
            assert got[c]["status"] == (CORRUPT if s.is_bad else 0), (tag, c)
            if not s.is_bad:
                from pfloor.decoder import materialize
                assert got["_kept"][c] == 1
                WC.assert_window_equal(materialize(got[c], s.ptype), FC.take_rows(exp[c], idx), f"{name} [{tag}] good chunk {c}")
                assert np.array_equal(got[c]["indices"].astype(np.int64), s.expected_indices()[idx])
    run(decoder, "product library")
    with switches(), GpuDecoder(0) as d:
        run(d, "diagnostics build")


def test_call_errors_and_async_copies(oracle, decoder, tmp_path):
    """PF_PRED_RANGE on a kept INT96 / FIXED_LEN_BYTE_ARRAY chunk stays PF_ERR_UNSUPPORTED_TYPE, the call errors of
    pf_decode_row_group_filter come out with keep flags set, and pf_copy_columns_async works after a kept filter."""
    from pfloor import _native
    specs, _w, _q = FD.BATCHES["nulls-int96-flba"].build(oracle.snappy_compress)
    f = _File(specs, tmp_path)
    keep = [True] * len(specs)
    L = _native.lib()
    for c, s in enumerate(specs):
        if s.ptype in (K.INT96, K.FLBA):
            with pytest.raises(Exception):
                f.run(decoder, "kept", keep=keep, preds=[(c, FD.RANGE, None, None)])
            assert "INT96" in decoder.error(), decoder.error()
            assert L.pf_wait(decoder.h) == STATE   # (nothing was enqueued)
    with pytest.raises(Exception):
        f.run(decoder, "kept", keep=keep, preds=[(len(specs), FD.IS_NULL, None, None)])
    with pytest.raises(Exception):
        f.run(decoder, "kept", keep=keep, windows=[(-1, 5)] * len(specs))
    with pytest.raises(Exception):
        f.run(decoder, "kept", keep=keep, preds=[(0, FD.IS_NULL, None, None)] * 9)
    c0 = 1
    preds = [(c0, FD.RANGE, FD._mid(specs[c0]), None)]
    got = f.run(decoder, "kept", keep=keep, preds=preds)
    assert got["_status"] == 0 and got["_kept"] == [1] * len(specs)
    n = len(specs)
    outs = (_native.ColumnOut * n)()
    arrs = []
    for c in range(n):
        ci = decoder.info(c)
        v = np.full(ci.num_slots * ci.width, 0xa5, np.uint8)
        b = np.full((ci.num_slots + 7) // 8, 0xa5, np.uint8)
        outs[c].values, outs[c].values_cap = (v.ctypes.data if v.size else None), v.nbytes
        outs[c].validity, outs[c].validity_cap = (b.ctypes.data if b.size else None), b.nbytes
        arrs.append((v, b))
    idx = (C.c_int * n)(*range(n))
    _native.check(L.pf_copy_columns_async(decoder.h, n, idx, outs), decoder.h, "pf_copy_columns_async")
    _native.check(L.pf_sync(decoder.h), decoder.h, "pf_sync")
    for c in range(n):
        assert arrs[c][0].tobytes() == got[c]["indices"].tobytes(), c
        assert np.array_equal(arrs[c][1], got[c]["validity"]), c


def test_dictionary_chars_overflow_reruns_the_filter(tmp_path):
    """A kept string predicate chunk whose dictionary chars overflow the chars arena on the first pass: the sizes of
    test_gpu_dict_keep's overflow test (the arena's floor is 16 MiB plus twice the page bytes, so small data never
    overflows it), with the kept chunk as long as the expanding one so that both can be filtered together. On the first
    pass k_dict_offsets reports PF_ERR_CAPACITY and k_sel_dict leaves; pf_wait runs the batch once more, window and
    filter stages included, and the filtered result must be right. The expectation comes from the construction: an entry
    matches or not (Python bytes), a row matches when its id's entry does."""
    from pfloor.decoder import GpuDecoder, materialize
    t0 = time.time()
    rng = np.random.default_rng(101)
    rows = 110000
    big = DC.Spec("big", "binary", [bytes([65 + i]) * 400 for i in range(4)])
    kept = DC.Spec("kept", "binary", [rng.integers(0, 256, 2000, dtype=np.uint8).tobytes() for _ in range(6000)])
    ids = rng.integers(0, 6000, rows)
    ids[0], ids[-1] = 5999, 0
    for p in range(5):
        big.page(rng.integers(0, 4, 22000), seed=1)
        kept.page(ids[p * 22000:(p + 1) * 22000], seed=p)
    big.keep = False
    specs = [big, kept]
    f = _File(specs, tmp_path, name="overflow.parquet")
    lo, hi = sorted(kept.dvals)[100], sorted(kept.dvals)[102]
    match = np.array([lo <= e <= hi for e in kept.dvals], bool)
    idx = np.flatnonzero(match[ids])
    assert match.sum() == 3 and 0 < len(idx) < 200
    with GpuDecoder(0) as dec:
        got = f.run(dec, "kept", keep=[False, True], windows=[(0, -1), (0, rows)], preds=[(1, FD.RANGE, lo, hi)])
        reruns = dec.chars_reruns()
    print(f"chars overflow under a filter: status {got['_status']} {got['_error']!r}, reruns {reruns}, {len(idx)} rows, "
          f"{time.time() - t0:.1f} s")
    assert got["_status"] == 0, got["_error"]
    assert reruns == 1, reruns
    assert got["_selection"][0] == rows and np.array_equal(got["_selection"][1], idx)
    assert got["_kept"] == [0, 1] and np.array_equal(got[1]["indices"].astype(np.int64), ids[idx])
    assert got[1]["dictionary"]["chars"].size == 12000000
    m = materialize(got[1], K.BYTE_ARRAY)
    assert m["chars"].tobytes() == b"".join(kept.dvals[i] for i in ids[idx])
    WC.assert_window_equal(got[0], FC.take_rows(FD.canon(big, big.chunk.expected()), idx), "chars overflow, the expanding chunk")
