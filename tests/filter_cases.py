"""Reference side of the row-filter tests: plain numpy and Python, never the code under test.

`eval_predicates` evaluates a conjunction over whole decoded flat chunks (the canonical layout of include/pfloor.h)
under the rules of pf_decode_row_group_filter: a null row matches only IS_NULL; INT32 / INT64 / BOOLEAN compare as
signed integers; FLOAT / DOUBLE by IEEE lo <= v && v <= hi (numpy's comparisons: NaN matches no bound, -0.0 == +0.0);
BYTE_ARRAY as Python bytes (unsigned bytewise, a proper prefix first). `take_rows` compacts a chunk to given rows as
the filter must return it, next to window_cases.slice_chunk."""
import numpy as np

from window_cases import _bits, _pack

BOOLEAN, INT32, INT64, INT96, FLOAT, DOUBLE, BYTE_ARRAY, FLBA = range(8)
RANGE, IS_NULL, NOT_NULL = 0, 1, 2
SEL_TILE = 1024   # rows per workgroup round of the k_sel_* kernels (csrc/pf_internal.h)
_DTYPE = {BOOLEAN: np.uint8, INT32: np.int32, INT64: np.int64, FLOAT: np.float32, DOUBLE: np.float64}


def present_of(chunk):
    n = int(chunk["num_slots"])
    return _bits(chunk["validity"], n).astype(bool) if "validity" in chunk else np.ones(n, bool)


def values_of(chunk, ptype):
    """The chunk's slots as typed values: a numpy array, or a list of bytes for BYTE_ARRAY (null slots: zero / b"")."""
    if ptype == BYTE_ARRAY:
        off = np.asarray(chunk["offsets"], np.int64)
        raw = np.asarray(chunk["chars"], np.uint8).tobytes()
        return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return np.ascontiguousarray(chunk["values"]).view(np.uint8).view(_DTYPE[ptype])


def eval_predicates(columns, preds):
    """columns: [(chunk, physical type)]; preds: [(column, op, lo, hi)] with lo / hi Python values of the column's
    type or None. Returns the bool mask over the rows."""
    n = int(columns[0][0]["num_rows"])
    mask = np.ones(n, bool)
    for col, op, lo, hi in preds:
        chunk, ptype = columns[col]
        assert int(chunk["num_rows"]) == n and "rep_levels" not in chunk
        present = present_of(chunk)
        if op == IS_NULL:
            mask &= ~present
            continue
        if op == NOT_NULL:
            mask &= present
            continue
        assert op == RANGE
        v = values_of(chunk, ptype)
        if ptype == BYTE_ARRAY:
            m = np.array([(lo is None or bytes(lo) <= x) and (hi is None or x <= bytes(hi)) for x in v], bool).reshape(n)
        else:
            dt = _DTYPE[ptype]
            m = np.ones(n, bool)
            with np.errstate(invalid="ignore"):
                if lo is not None:
                    m &= dt(lo) <= v
                if hi is not None:
                    m &= v <= dt(hi)
        mask &= m & present
    return mask


def take_rows(chunk, idx):
    """The flat chunk compacted to rows idx (ascending), in the canonical layout."""
    idx = np.asarray(idx, np.int64)
    assert "rep_levels" not in chunk
    k = len(idx)
    w = int(chunk.get("width", 0))
    out = {"num_entries": k, "num_slots": k, "num_rows": k, "num_values": k, "num_chars": 0, "width": w}
    if "values" in chunk:
        out["values"] = np.ascontiguousarray(chunk["values"]).view(np.uint8).reshape(-1, w)[idx].ravel().copy()
    if "validity" in chunk:
        v = _bits(chunk["validity"], int(chunk["num_slots"]))[idx]
        out["validity"] = _pack(v)
        out["num_values"] = int(v.sum())
    if "offsets" in chunk:
        off = np.asarray(chunk["offsets"], np.int64)
        lens = off[idx + 1] - off[idx]
        noff = np.zeros(k + 1, np.int32)
        np.cumsum(lens, out=noff[1:])
        chars = np.asarray(chunk["chars"], np.uint8)
        parts = [chars[off[i]:off[i + 1]] for i in idx]
        out["offsets"] = noff
        out["chars"] = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        out["num_chars"] = int(noff[-1])
    return out
