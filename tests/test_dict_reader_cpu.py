"""Kept dictionaries on the host, without a GPU: pfloor.decoder.materialize expands fabricated kept arrays ("indices"
+ "dictionary", as GpuDecoder.fetch returns them for a kept chunk) into the canonical layout of include/pfloor.h, and
a reader._ColumnCursor over kept arrays yields what a cursor over their materialization yields.

The expectation is built here slot by slot from the same inputs (values[s] = dictionary[indices[s]] where the slot is
valid, zero bytes or a zero-length string where it is not), never by calling the code under test."""
import types

import numpy as np
import pytest

from pfloor.decoder import INDEX_DTYPES, materialize
from pfloor.reader import _ColumnCursor

WIDTHS = {1: 4, 2: 8, 3: 12, 4: 4, 5: 8}      # INT32, INT64, INT96, FLOAT, DOUBLE
TYPES = [(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (7, 5), (7, 16), (6, 0)]


def _entries(ptype, type_length, n, rng):
    """n dictionary entries as bytes objects; BYTE_ARRAY entries include the empty string and a 33-byte value."""
    if ptype == 6:
        out = [bytes(rng.integers(97, 123, int(rng.integers(1, 12))).astype(np.uint8)) for _ in range(n)]
        if n > 1:
            out[1] = b""
        if n > 2:
            out[2] = b"x" * 33
        return out
    w = type_length if ptype == 7 else WIDTHS[ptype]
    return [bytes(rng.integers(0, 256, w).astype(np.uint8)) for _ in range(n)]


def _kept(ptype, type_length, entries, idx, valid, index_width, optional=True):
    """(kept arrays, expected canonical arrays) of a chunk whose slot s holds entries[idx[s]] where valid[s]."""
    ns = len(idx)
    w = 0 if ptype == 6 else (type_length if ptype == 7 else WIDTHS[ptype])
    d = {"n_entries": len(entries), "width": w}
    if ptype == 6:
        offs = np.zeros(len(entries) + 1, np.int32)
        np.cumsum([len(e) for e in entries], out=offs[1:])
        d["offsets"], d["chars"] = offs, np.frombuffer(b"".join(entries), np.uint8)
    else:
        d["values"] = np.frombuffer(b"".join(entries), np.uint8)
    stored = np.where(valid, idx, 0).astype(INDEX_DTYPES[index_width])   # a null slot holds 0
    kept = {"status": 0, "num_entries": ns, "num_slots": ns, "num_values": int(valid.sum()), "num_rows": ns, "num_chars": 0,
            "width": index_width, "indices": stored, "dictionary": d}
    exp = {"num_entries": ns, "num_slots": ns, "num_values": int(valid.sum()), "num_rows": ns}
    if optional:
        kept["validity"] = exp["validity"] = np.packbits(valid, bitorder="little")
    slots = [entries[int(idx[s])] if valid[s] else (b"" if ptype == 6 else bytes(w)) for s in range(ns)]
    if ptype == 6:
        eo = np.zeros(ns + 1, np.int32)
        np.cumsum([len(x) for x in slots], out=eo[1:])
        exp["offsets"], exp["chars"] = eo, np.frombuffer(b"".join(slots), np.uint8)
    else:
        exp["values"] = np.frombuffer(b"".join(slots), np.uint8)
    return kept, exp


def _assert_canonical(got, exp, ptype, where):
    for k in ("num_entries", "num_slots", "num_values", "num_rows"):
        assert got[k] == exp[k], (where, k)
    assert "indices" not in got and "dictionary" not in got, where
    for k in ("values", "offsets", "chars", "validity"):
        assert (k in got) == (k in exp), (where, k)
        if k in exp:
            assert np.asarray(got[k]).dtype == np.asarray(exp[k]).dtype, (where, k, np.asarray(got[k]).dtype)
            assert np.array_equal(got[k], exp[k]), (where, k)
    if ptype == 6:
        assert got["num_chars"] == len(exp["chars"]) and got["width"] == 0, where


@pytest.mark.parametrize("ptype,type_length", TYPES)
@pytest.mark.parametrize("index_width,n_entries", [(1, 1), (1, 7), (1, 256), (2, 257), (2, 4000), (4, 65537)])
def test_materialize(ptype, type_length, index_width, n_entries):
    rng = np.random.default_rng(1000 * ptype + n_entries)
    entries = _entries(ptype, type_length, n_entries, rng)
    ns = 1000
    idx = rng.integers(0, n_entries, ns)
    idx[5], idx[6] = n_entries - 1, 0           # the last and the first entry are used
    if ptype == 6 and n_entries > 2:
        idx[7], idx[8] = 1, 2                    # the empty string and the 33-byte value
    for name, valid in (("all present", np.ones(ns, bool)),
                        ("first null", np.arange(ns) != 0),
                        ("last null", np.arange(ns) != ns - 1),
                        ("first and last null", (np.arange(ns) != 0) & (np.arange(ns) != ns - 1)),
                        ("random", rng.random(ns) < 0.8),
                        ("all null", np.zeros(ns, bool))):
        kept, exp = _kept(ptype, type_length, entries, idx, valid, index_width)
        _assert_canonical(materialize(kept, ptype), exp, ptype, f"{name}, type {ptype}, {n_entries} entries")
    kept, exp = _kept(ptype, type_length, entries, idx, np.ones(ns, bool), index_width, optional=False)   # REQUIRED
    _assert_canonical(materialize(kept, ptype), exp, ptype, f"required, type {ptype}")


@pytest.mark.parametrize("ptype,type_length", TYPES)
def test_materialize_empty_dictionary_all_null(ptype, type_length):
    for ns in (0, 1, 9):
        kept, exp = _kept(ptype, type_length, [], np.zeros(ns, np.int64), np.zeros(ns, bool), 1)
        _assert_canonical(materialize(kept, ptype), exp, ptype, f"empty dictionary, {ns} slots")


def test_materialize_refuses_an_index_outside_the_dictionary():
    kept, _ = _kept(1, 0, _entries(1, 0, 3, np.random.default_rng(0)), np.array([0, 1, 2]), np.ones(3, bool), 1)
    kept["indices"] = np.array([0, 3, 1], np.uint8)
    with pytest.raises(ValueError):
        materialize(kept, 1)
    kept["validity"] = np.packbits(np.array([True, False, True]), bitorder="little")   # ... unless its slot is null
    assert materialize(kept, 1)["values"].size == 12


def test_materialize_leaves_expanded_arrays_alone():
    arrays = {"status": 0, "num_slots": 2, "values": np.arange(8, dtype=np.uint8), "width": 4}
    assert materialize(arrays, 1) is arrays


def _col(ptype, type_length=0, converted=-1, logical=0, scale=0, optional=True):
    return types.SimpleNamespace(physical_type=ptype, type_length=type_length, max_def=int(optional), max_rep=0, repeated_def=0,
                                 converted_type=converted, logical_type=logical, scale=scale, precision=9, path=["c"])


CURSOR_COLUMNS = {
    "utf8": (_col(6, converted=0), 6, 0),
    "decimal": (_col(7, 5, converted=5, scale=2), 7, 5),
    "decimal_binary": (_col(6, converted=5, scale=3), 6, 0),   # (the empty entry stringifies as "<INVALID>")
    "int96": (_col(3), 3, 0),
    "double": (_col(5), 5, 0),
    "double_required": (_col(5, optional=False), 5, 0),
}


@pytest.mark.parametrize("name", list(CURSOR_COLUMNS))
@pytest.mark.parametrize("index_width,n_entries", [(1, 5), (2, 300)])
def test_cursor_over_kept_arrays(name, index_width, n_entries):
    col, ptype, tl = CURSOR_COLUMNS[name]
    rng = np.random.default_rng(n_entries)
    entries = _entries(ptype, tl, n_entries, rng)
    ns = 700
    idx = rng.integers(0, n_entries, ns)
    valid = rng.random(ns) < 0.7 if col.max_def else np.ones(ns, bool)
    if col.max_def:
        valid[0], valid[-1] = False, False
    kept, _ = _kept(ptype, tl, entries, idx, valid, index_width, optional=bool(col.max_def))
    a, b = _ColumnCursor(col, kept), _ColumnCursor(col, materialize(kept, ptype))
    calls = []
    convert = a._convert
    a._convert = lambda raw: (calls.append(raw), convert(raw))[1]
    nulls = 0
    for s in range(ns):
        assert a.definition_level() == b.definition_level(), (name, s)
        va, vb = a.read_value(), b.read_value()
        assert type(va) is type(vb) and (va == vb or (va != va and vb != vb)), (name, s, va, vb)   # (NaN equals NaN here)
        nulls += va is None
        a.consume()
        b.consume()
        assert a.repetition_level() == b.repetition_level() == 0
    assert nulls == int((~valid).sum())
    assert len(calls) == len(set(int(i) for i in idx[valid])), "every used dictionary entry is converted once"
