"""Reference side of the row-window tests: plain numpy, never the code under test.

`slice_chunk` cuts a whole decoded chunk (the oracle's decode, or the arrays a file was written from) in the canonical
layout of include/pfloor.h down to rows [skip, skip + take), as pf_decode_row_group_rows must return it: values from the
window's first slot, validity bits from bit 0 with zero padding, offsets rebased to 0, only the window's chars and
levels. `canonical_*` build that layout from Python values (the pyarrow comparison, the GPU-written files)."""
import os

import numpy as np

from conftest import GOLDEN

ROWWINDOW = os.path.join(GOLDEN, "rowwindow")
FIXTURES = ("rw_snappy", "rw_none")
ARRAYS = ("values", "validity", "offsets", "chars", "list_offsets", "list_validity", "def_levels", "rep_levels")
COUNTS = ("num_entries", "num_slots", "num_values", "num_rows", "num_chars")

# k_win_copy's tile (csrc/pf_internal.h WIN_TILE): output bytes of one array one workgroup writes per round
WIN_TILE = 4096


def fixture_path(name):
    return os.path.join(ROWWINDOW, name + ".parquet")


def _bits(b, n):
    return np.unpackbits(np.asarray(b, np.uint8), bitorder="little")[:n]


def _pack(bits):
    return np.packbits(np.asarray(bits, np.uint8), bitorder="little")


def slice_chunk(a, skip, take):
    """Rows [skip, skip + take) of the whole chunk `a` (take -1: to the end)."""
    rows = int(a["num_rows"])
    if take < 0:
        take = rows - skip
    assert 0 <= skip and skip + take <= rows
    nested = "rep_levels" in a
    if nested:
        starts = np.append(np.flatnonzero(np.asarray(a["rep_levels"]) == 0), int(a["num_entries"]))
        assert len(starts) == rows + 1
        e0, e1 = int(starts[skip]), int(starts[skip + take])
        lo = np.asarray(a["list_offsets"], np.int64)
        s0, s1 = int(lo[skip]), int(lo[skip + take])
    else:
        e0 = s0 = skip
        e1 = s1 = skip + take
    w = int(a.get("width", 0))
    out = {"num_entries": e1 - e0, "num_slots": s1 - s0, "num_rows": take, "num_values": s1 - s0, "num_chars": 0, "width": w}
    if "values" in a:
        out["values"] = np.asarray(a["values"]).view(np.uint8)[s0 * w:s1 * w].copy()
    if "validity" in a:
        v = _bits(a["validity"], int(a["num_slots"]))[s0:s1]
        out["validity"] = _pack(v)
        out["num_values"] = int(v.sum())
    if "offsets" in a:
        off = np.asarray(a["offsets"], np.int32)
        out["offsets"] = (off[s0:s1 + 1] - off[s0]).astype(np.int32)
        out["chars"] = np.asarray(a["chars"], np.uint8)[off[s0]:off[s1]].copy()
        out["num_chars"] = int(off[s1] - off[s0])
    if nested:
        lo32 = np.asarray(a["list_offsets"], np.int32)
        out["list_offsets"] = (lo32[skip:skip + take + 1] - lo32[skip]).astype(np.int32)
        out["list_validity"] = _pack(_bits(a["list_validity"], rows)[skip:skip + take])
        out["def_levels"] = np.asarray(a["def_levels"], np.uint8)[e0:e1].copy()
        out["rep_levels"] = np.asarray(a["rep_levels"], np.uint8)[e0:e1].copy()
    return out


def assert_window_equal(got, exp, label=""):
    """Bit-exact, padding bits included: every count and every array byte."""
    for k in COUNTS:
        if k in exp:
            assert int(got[k]) == int(exp[k]), f"{label}: {k} {got[k]} != {exp[k]}"
    for a in ARRAYS:
        if a not in exp:
            continue
        assert a in got, f"{label}: missing {a}"
        g = np.ascontiguousarray(got[a]).view(np.uint8).ravel()
        e = np.ascontiguousarray(exp[a]).view(np.uint8).ravel()
        assert g.shape == e.shape, f"{label}: {a} has {g.size} bytes, expected {e.size}"
        if not np.array_equal(g, e):
            bad = np.flatnonzero(g != e)
            raise AssertionError(f"{label}: {a} differs at bytes {bad[:8]} ({len(bad)} in all): "
                                 f"got {g[bad[:8]]}, expected {e[bad[:8]]}")


# ---- canonical arrays from Python values ---------------------------------------------------------------------------

def canonical_fixed(values, dtype, nullable):
    """values: a list with None for nulls (null slots hold zero bytes)."""
    n = len(values)
    present = np.array([v is not None for v in values], bool)
    arr = np.array([0 if v is None else v for v in values], dtype)
    out = {"num_entries": n, "num_slots": n, "num_rows": n, "num_values": int(present.sum()), "num_chars": 0,
           "width": arr.dtype.itemsize, "values": arr.view(np.uint8).copy()}
    if nullable:
        out["validity"] = _pack(present)
    return out


def canonical_strings(values, nullable):
    """values: a list of bytes / str / None (null slots are zero-length)."""
    raw = [b"" if v is None else (v.encode() if isinstance(v, str) else bytes(v)) for v in values]
    n = len(raw)
    off = np.zeros(n + 1, np.int32)
    np.cumsum([len(x) for x in raw], out=off[1:])
    out = {"num_entries": n, "num_slots": n, "num_rows": n, "num_values": sum(v is not None for v in values),
           "num_chars": int(off[-1]), "width": 0, "offsets": off, "chars": np.frombuffer(b"".join(raw), np.uint8).copy()}
    if nullable:
        out["validity"] = _pack([v is not None for v in values])
    return out


def canonical_list_int32(lists):
    """lists: per row None | [] | [int or None, ...] under the three-level LIST schema of pyarrow
    (optional group (LIST) { repeated group list { optional int32 element } }): max_def 3, repeated_def 2,
    list_null_def 1."""
    defs, reps, vals, valid, lo, lv = [], [], [], [], [0], []
    for row in lists:
        lv.append(row is not None)
        if row is None or len(row) == 0:
            defs.append(0 if row is None else 1)
            reps.append(0)
        else:
            for i, x in enumerate(row):
                defs.append(2 if x is None else 3)
                reps.append(0 if i == 0 else 1)
                vals.append(0 if x is None else x)
                valid.append(x is not None)
        lo.append(len(vals))
    return {"num_entries": len(defs), "num_slots": len(vals), "num_rows": len(lists), "num_values": int(sum(valid)),
            "num_chars": 0, "width": 4, "values": np.array(vals, np.int32).view(np.uint8).copy(), "validity": _pack(valid),
            "list_offsets": np.array(lo, np.int32), "list_validity": _pack(lv),
            "def_levels": np.array(defs, np.uint8), "rep_levels": np.array(reps, np.uint8)}


def page_rows(first_rows, n_rows):
    """[(row_lo, row_hi)] of the pages whose first rows are given."""
    ends = list(first_rows[1:]) + [n_rows]
    return list(zip(first_rows, ends))


def select_pages(first_rows, n_rows, lo, hi):
    """The issue's rule, restated: data pages p with first[p] < hi and first[p + 1] > lo; none for an empty range."""
    if lo == hi:
        return []
    return [p for p, (a, b) in enumerate(page_rows(first_rows, n_rows)) if a < hi and b > lo]
