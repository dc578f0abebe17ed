"""Case generator of the DELTA_BINARY_PACKED / DELTA_BYTE_ARRAY write tests (TEST INFRASTRUCTURE ONLY;
pure Python + numpy, no product code). Shared by test_write_delta_cpu.py (the expected streams, read
by the oracle and pyarrow) and test_gpu_write_delta.py (the GPU encoder against those streams).

A case is one column: its present (dense) values, the rows they sit in and the page size it is
written with. The cases are grouped into files of equal row count:

  n<count>   every integer family as INT32 and INT64, REQUIRED, `count` values in one page: the edges
             of miniblock (32), block (128 deltas = values 2..129) and stream header (0, 1, 2)
  pages      every integer and string family at LAYOUT_ROWS rows as REQUIRED, with 30 % nulls, and
             with all-null pages between all-present ones, at 64 and 136 rows per page (page starts
             reset the first value and the prefix)
  big        20,001 rows at the default page size: a 20,000-value page (the read path's block-parallel
             DELTA_BINARY_PACKED route) and a page of one value
"""
import numpy as np

import pagekit as K

INT_COUNTS = (0, 1, 2, 32, 33, 34, 64, 65, 128, 129, 130, 161, 257, 1025)
PAGE_ROWS = (64, 136)
LAYOUT_ROWS = 408          # 3 pages of 136, 6 pages of 64 and one of 24
DEFAULT_PAGE_ROWS = 20000
INT_FAMILIES = ("constant", "ascending", "steps", "uniform", "minmax", "outlier", "flatmini")
STRING_FAMILIES = ("sorted", "text", "empty", "runs", "prefixes", "long", "bytes")
MODES = ("req", "nulls", "nullpage")


def _rng(*key):
    return np.random.default_rng(sum(ord(c) * (i + 7) for i, c in enumerate("/".join(map(str, key)))))


def _from_deltas(first, deltas, bits):
    """first, first + d0, first + d0 + d1, ... wrapped to `bits`."""
    v = np.concatenate([[0], np.cumsum(np.asarray(deltas, np.int64))]) + np.int64(first)
    return v.astype(np.int32) if bits == 32 else v


def int_values(family, bits, n):
    """n values of an integer family as int32 / int64."""
    dt = np.int32 if bits == 32 else np.int64
    lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
    rng = _rng(family, bits, n)
    if n == 0:
        return np.zeros(0, dt)
    nd = n - 1
    blk, pos = np.arange(nd) // 128, np.arange(nd) % 128
    if family == "constant":                     # all deltas 0: every width 0
        return np.full(n, -7, dt)
    if family == "ascending":
        return (np.arange(n) - 5).astype(dt)
    if family == "steps":                        # small signed steps
        return _from_deltas(1000, rng.integers(-3, 4, nd), bits)
    if family == "uniform":                      # the whole range: wrapping deltas, width 32 / 64
        return rng.integers(lo, hi, n, dtype=dt, endpoint=True)
    if family == "minmax":                       # deltas of +-(2^bits - 1), which wrap to +-1
        return np.where(np.arange(n) % 2 == 0, lo, hi).astype(dt)
    if family == "outlier":                      # noise of 1..4 bits by miniblock, one 2^20 outlier per block
        d = rng.integers(0, 1 << 30, nd) % (2 << (pos // 32))
        d[pos == (37 * blk + 3) % 128] = 1 << 20
        return _from_deltas(-12345, d, bits)
    if family == "flatmini":                     # first miniblock of every block all-min (width 0)
        d = np.where(pos < 32, -2, rng.integers(-2, 50, nd))
        return _from_deltas(0, d, bits)
    raise KeyError(family)


def string_values(family, n):
    """n values of a string family as a list of bytes."""
    rng = _rng(family, n)
    if family == "sorted":                       # sorted keys with long shared prefixes
        keys = np.sort(rng.integers(0, 10**7, n))
        return [b"customer/region-%02d/account-%010d" % (k // 10**6, k) for k in keys]
    if family == "text":
        return [(rng.integers(0, 26, int(m)) + 97).astype(np.uint8).tobytes() for m in rng.integers(0, 40, n)]
    if family == "empty":
        return [b""] * n
    if family == "runs":                         # runs of identical values: suffix empty
        return [b"value-%04d" % (i // 5) for i in range(n)]
    if family == "prefixes":                     # each value a proper prefix of the previous, then the reverse
        base = (rng.integers(0, 26, 30) + 97).astype(np.uint8).tobytes()
        lens = [30 - k if k < 30 else k - 29 for k in (i % 60 for i in range(n))]
        return [base[:m] for m in lens]
    if family == "long":                         # 400 bytes that share 399
        base = (rng.integers(0, 26, 399) + 97).astype(np.uint8).tobytes()
        return [base + bytes([65 + i % 26]) for i in range(n)]
    if family == "bytes":                        # uniform random bytes
        return [rng.integers(0, 256, int(m), dtype=np.uint8).tobytes() for m in rng.integers(0, 21, n)]
    raise KeyError(family)


def present_rows(mode, rows, page_rows):
    """None (REQUIRED) or the bool mask of present rows."""
    if mode == "req":
        return None
    if mode == "nulls":
        return _rng("present", rows, page_rows).random(rows) >= 0.3
    assert mode == "nullpage"                    # page 0 present, page 1 null, ...
    return (np.arange(rows) // page_rows) % 2 == 0


class Case:
    def __init__(self, name, ptype, family, rows, mode="req", page_rows=DEFAULT_PAGE_ROWS):
        self.name, self.ptype, self.rows, self.page_rows = name, ptype, rows, page_rows
        self.present = present_rows(mode, rows, page_rows)
        m = rows if self.present is None else int(self.present.sum())
        if ptype == K.BYTE_ARRAY:
            self.dense = string_values(family, m)
        else:
            self.dense = int_values(family, 32 if ptype == K.INT32 else 64, m)

    @property
    def optional(self):
        return self.present is not None

    @property
    def encoding(self):
        return K.DELTA_BYTE_ARRAY if self.ptype == K.BYTE_ARRAY else K.DELTA_BINARY_PACKED

    def mask(self):
        return np.ones(self.rows, bool) if self.present is None else self.present

    def pages(self):
        """[(present mask of the page's rows or None, its present values)]; a chunk of 0 rows is one empty page."""
        out, d = [], 0
        mask = self.mask()
        for r0 in range(0, max(self.rows, 1), self.page_rows):
            pm = mask[r0:r0 + self.page_rows]
            cnt = int(pm.sum())
            out.append((pm if self.optional else None, self.dense[d:d + cnt]))
            d += cnt
        return out

    def stream(self, vals):
        """The values section of a page holding `vals`, in parquet-mr's layout."""
        if self.ptype == K.BYTE_ARRAY:
            return K.delta_byte_array(list(vals))
        return K.dbp([int(v) for v in vals], bits=32 if self.ptype == K.INT32 else 64)

    def pagekit_vals(self, vals):
        if self.ptype == K.BYTE_ARRAY:
            return list(vals)
        return np.ascontiguousarray(vals).view(np.uint8).reshape(len(vals), K.width_of(self.ptype))

    def row_arrays(self):
        """The column as the encoder takes it: (values | (offsets, chars), validity or None); null rows 0 / empty."""
        mask = self.mask()
        validity = np.packbits(mask, bitorder="little") if self.optional else None
        if self.ptype == K.BYTE_ARRAY:
            lens = np.zeros(self.rows, np.int64)
            lens[mask] = [len(x) for x in self.dense]
            offs = np.zeros(self.rows + 1, np.int32)
            np.cumsum(lens, out=offs[1:])
            return (offs, np.frombuffer(b"".join(self.dense), np.uint8)), validity
        v = np.zeros(self.rows, self.dense.dtype)
        v[mask] = self.dense
        return v, validity

    def expected(self):
        """The decoded chunk in the canonical layout of include/pfloor.h (what golden_util compares)."""
        mask = self.mask()
        out = {"num_entries": self.rows, "num_slots": self.rows, "num_values": int(mask.sum()), "num_rows": self.rows}
        data, validity = self.row_arrays()
        if self.ptype == K.BYTE_ARRAY:
            out["offsets"], out["chars"] = data
        else:
            out["values"] = data.view(np.uint8)
        if self.optional:
            out["validity"] = validity
        return out

    def pylist(self):
        """Rows as Python values, None = null (what pyarrow's to_pylist gives; BYTE_ARRAY as bytes)."""
        it = iter(self.dense if self.ptype == K.BYTE_ARRAY else self.dense.tolist())
        return [next(it) if p else None for p in self.mask()]


def _count_cases(n):
    return [Case(f"{fam}_{bits}", pt, fam, n) for fam in INT_FAMILIES for pt, bits in ((K.INT32, 32), (K.INT64, 64))]


def _layout_cases():
    out = []
    for pr in PAGE_ROWS:
        for mode in MODES:
            for fam in INT_FAMILIES:
                for pt, bits in ((K.INT32, 32), (K.INT64, 64)):
                    out.append(Case(f"{fam}_{bits}_{mode}_{pr}", pt, fam, LAYOUT_ROWS, mode, pr))
            for fam in STRING_FAMILIES:
                out.append(Case(f"s_{fam}_{mode}_{pr}", K.BYTE_ARRAY, fam, LAYOUT_ROWS, mode, pr))
    return out


def _big_cases():
    return [Case("steps_64", K.INT64, "steps", 20001), Case("uniform_32", K.INT32, "uniform", 20001),
            Case("s_sorted", K.BYTE_ARRAY, "sorted", 20001)]


FILE_IDS = tuple(f"n{n}" for n in INT_COUNTS) + ("pages", "big")
_CACHE = {}


def file_cases(fid):
    """(rows, cases) of a file; built once and shared (callers must not modify the arrays)."""
    if fid not in _CACHE:
        if fid == "pages":
            _CACHE[fid] = (LAYOUT_ROWS, _layout_cases())
        elif fid == "big":
            _CACHE[fid] = (20001, _big_cases())
        else:
            _CACHE[fid] = (int(fid[1:]), _count_cases(int(fid[1:])))
    return _CACHE[fid]
