"""Reference encoder and case generator of the RLE / bit-packed hybrid write tests (TEST INFRASTRUCTURE
ONLY; pure Python + numpy, no product code). Shared by test_write_hybrid_cpu.py (the expected streams,
read back by the oracle, pyarrow and the decoder below) and test_gpu_write_hybrid.py (the GPU encoder
against those streams).

`encode` is parquet-mr's RunLengthBitPackingHybridEncoder as a value-by-value state machine: previous
value, repeat count, a buffer of 8 values, the count of groups under the open bit-packed header, that
header's position, and the tail rule of toBytes(). It is deliberately not the closed form the kernels
use (a chain of positions over run lengths), so the tests do not restate the code under test.

A case is one column: its present (dense) values, the rows they sit in and the page size it is written
with. INT32 cases are dictionary-encoded, so their id stream is the values renumbered in first-occurrence
order; BOOLEAN cases are RLE-encoded. Cases of equal row count share a file (`file_cases`).
"""
import numpy as np

import pagekit as K

DEFAULT_PAGE_ROWS = 20000


# ---------------------------------------------------------------- reference encoder / decoder
def _uvarint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _pack8(vals, bw):
    acc = 0
    for k, x in enumerate(vals):
        acc |= int(x) << (k * bw)
    return acc.to_bytes(bw, "little")


class _Encoder:
    def __init__(self, bw):
        self.bw = bw
        self.out = bytearray()
        self.prev = 0               # previousValue
        self.repeat = 0             # repeatCount
        self.buf = []               # bufferedValues[0 .. numBufferedValues)
        self.groups = 0             # bitPackedGroupCount
        self.header = -1            # bitPackedRunHeaderPointer

    def write(self, v):
        if v == self.prev:
            self.repeat += 1
            if self.repeat >= 8:    # the run goes on: nothing is buffered any more
                return
        else:
            if self.repeat >= 8:
                self._rle_run()
            self.repeat = 1
            self.prev = v
        self.buf.append(v)
        if len(self.buf) == 8:
            self._packed_group()

    def _packed_group(self):
        if self.groups >= 63:
            self._end_packed()
        if self.header == -1:
            self.header = len(self.out)
            self.out.append(0)
        self.out += _pack8(self.buf, self.bw)
        self.buf = []
        self.repeat = 0             # what the group ate no longer counts towards a run
        self.groups += 1

    def _end_packed(self):
        if self.header == -1:
            return
        self.out[self.header] = (self.groups << 1) | 1
        self.header = -1
        self.groups = 0

    def _rle_run(self):
        self._end_packed()
        self.out += _uvarint(self.repeat << 1) + int(self.prev).to_bytes((self.bw + 7) // 8, "little")
        self.repeat = 0
        self.buf = []

    def finish(self):
        if self.repeat >= 8:
            self._rle_run()
        elif self.buf:
            self.buf += [0] * (8 - len(self.buf))
            self._packed_group()
            self._end_packed()
        else:
            self._end_packed()
        return bytes(self.out)


def encode(values, bw):
    """The hybrid stream of `values` at width `bw` (no width byte, no length prefix)."""
    e = _Encoder(bw)
    for v in np.asarray(values).tolist():
        e.write(int(v))
    return e.finish()


def decode(stream, bw, n):
    """The first n values of a hybrid stream; the whole stream must be consumed by them."""
    out, pos, nb = [], 0, (bw + 7) // 8
    while len(out) < n:
        h, shift = 0, 0
        while True:
            b = stream[pos]
            pos += 1
            h |= (b & 0x7f) << shift
            shift += 7
            if not b & 0x80:
                break
        if h & 1:
            groups = h >> 1
            acc = int.from_bytes(stream[pos:pos + groups * bw], "little")
            assert pos + groups * bw <= len(stream)
            pos += groups * bw
            out += [(acc >> (k * bw)) & ((1 << bw) - 1) for k in range(groups * 8)]
        else:
            v = int.from_bytes(stream[pos:pos + nb], "little")
            pos += nb
            out += [v] * (h >> 1)
    assert pos == len(stream), (pos, len(stream))
    assert all(v == 0 for v in out[n:]), "padding of the last group is not zero"
    return out[:n]


def id_width(d):
    """parquet-mr's BytesUtils.getWidthFromMaxInt(d - 1): a one-entry dictionary has width 0."""
    return int(max(d - 1, 0)).bit_length()


def first_occurrence_ids(values):
    """(ids, dictionary): values renumbered in the order they first occur."""
    values = np.asarray(values)
    if len(values) == 0:
        return np.zeros(0, np.int64), values
    uniq, first, inv = np.unique(values, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")         # unique index -> rank of its first occurrence
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    return rank[inv.ravel()], uniq[order]


# ---------------------------------------------------------------- cases
def _rng(*key):
    return np.random.default_rng(sum(ord(c) * (i + 7) for i, c in enumerate("/".join(map(str, key)))))


def _noise(n, a=101, b=102):
    """n values without two equal neighbours."""
    return [a if i % 2 == 0 else b for i in range(n)]


class Case:
    def __init__(self, name, ptype, dense, present=None, page_rows=DEFAULT_PAGE_ROWS):
        self.name, self.ptype, self.page_rows = name, ptype, page_rows
        self.present = None if present is None else np.asarray(present, bool)
        self.dense = np.asarray(dense, np.uint8 if ptype == K.BOOLEAN else np.int32)
        self.rows = len(self.dense) if self.present is None else len(self.present)
        assert len(self.dense) == (self.rows if self.present is None else int(self.present.sum())), name
        if ptype == K.BOOLEAN:
            self.ids, self.dictionary = self.dense, None
        else:
            self.ids, self.dictionary = first_occurrence_ids(self.dense)

    @property
    def optional(self):
        return self.present is not None

    @property
    def encoding(self):
        if self.ptype == K.BOOLEAN:
            return K.RLE
        return K.RLE_DICTIONARY if len(self.dense) else K.PLAIN   # a chunk without a value has no dictionary

    @property
    def bw(self):
        return 1 if self.ptype == K.BOOLEAN else id_width(len(self.dictionary))

    def mask(self):
        return np.ones(self.rows, bool) if self.present is None else self.present

    def pages(self):
        """[(present mask of the page's rows or None, its present values, their ids)]; 0 rows: one empty page."""
        out, d = [], 0
        mask = self.mask()
        for r0 in range(0, max(self.rows, 1), self.page_rows):
            pm = mask[r0:r0 + self.page_rows]
            cnt = int(pm.sum())
            out.append((pm if self.optional else None, self.dense[d:d + cnt], self.ids[d:d + cnt]))
            d += cnt
        return out

    def levels_stream(self, pm):
        return encode(np.asarray(pm, np.uint8), 1) if self.optional else b""

    def values_stream(self, ids):
        """The values section of a page: width byte + id stream, or 4-byte length + BOOLEAN stream."""
        if self.encoding == K.PLAIN:
            return b""
        s = encode(ids, self.bw)
        if self.ptype == K.BOOLEAN:
            return len(s).to_bytes(4, "little") + s
        return bytes([self.bw]) + s

    def pagekit_vals(self, vals):
        a = np.ascontiguousarray(vals)
        return a.view(np.uint8).reshape(len(a), K.width_of(self.ptype))

    def row_arrays(self):
        """The column as the encoder takes it: (values, validity or None); null rows 0."""
        mask = self.mask()
        validity = np.packbits(mask, bitorder="little") if self.optional else None
        v = np.zeros(self.rows, self.dense.dtype)
        v[mask] = self.dense
        return v, validity

    def expected(self):
        """The decoded chunk in the canonical layout of include/pfloor.h (what golden_util compares)."""
        mask = self.mask()
        out = {"num_entries": self.rows, "num_slots": self.rows, "num_values": int(mask.sum()), "num_rows": self.rows}
        data, validity = self.row_arrays()
        out["values"] = data.view(np.uint8)
        if self.optional:
            out["validity"] = validity
        return out

    def pylist(self):
        it = iter(self.dense.astype(bool).tolist() if self.ptype == K.BOOLEAN else self.dense.tolist())
        return [next(it) if p else None for p in self.mask()]


def _int(name, dense, **kw):
    return Case(name, K.INT32, dense, **kw)


def _dict_values(d, n, key):
    """n INT32 values of exactly d distinct ones: each once (shuffled ids are not needed: first-occurrence
    order numbers them anyway), then random picks with runs of 1..20 mixed in."""
    rng = _rng("dict", d, n, key)
    vals = (np.arange(d, dtype=np.int64) * 2654435761 % (1 << 31)).astype(np.int32)   # distinct: odd multiplier mod 2^31
    rest = n - d
    assert rest >= 0
    picks = rng.integers(0, d, rest)
    runs = rng.choice([1, 1, 1, 2, 7, 8, 9, 20], rest)
    ids = np.repeat(picks, runs)[:rest]
    return np.concatenate([vals, vals[ids]])


def _null_stretches(rows, key):
    """Present mask with null stretches of 100..3000 rows between present stretches of 1..2500."""
    rng = _rng("stretch", rows, key)
    m, r, on = np.ones(rows, bool), 0, True
    while r < rows:
        k = int(rng.integers(1, 2500)) if on else int(rng.integers(100, 3001))
        m[r:r + k] = on
        r, on = r + k, not on
    return m


def _bool_family(fam, n, key):
    rng = _rng("bool", fam, n, key)
    if fam == "constant":
        return np.ones(n, np.uint8)
    if fam == "alternating":
        return (np.arange(n) % 2).astype(np.uint8)
    if fam == "random":
        return (rng.random(n) < 0.5).astype(np.uint8)
    assert fam == "longruns"
    runs = rng.choice([1, 3, 7, 8, 9, 40, 700], n)
    return np.repeat(np.arange(n) % 2, runs)[:n].astype(np.uint8)


def _small_cases():
    out = []
    # a repeat of L values starting o entries after a group boundary, between values that do not repeat
    for L in (7, 8, 9, 15, 16, 17):
        for o in range(9):
            out.append(_int(f"rep{L}_at{o}", _noise(o) + [7] * L + _noise(48 - o - L, 103, 104)))
    out.append(_int("eaten_head", [0] + [1] * 10))
    # two short repeats back to back whose sum passes 8
    out.append(_int("two_5_5", [1] * 5 + [2] * 5 + _noise(6)))
    out.append(_int("two_4_7_at3", _noise(3) + [1] * 4 + [2] * 7 + _noise(2)))
    out.append(_int("two_7_7", [1] * 7 + [2] * 7 + [3] * 2))
    # packed stretches of 62 .. 127 groups, and each plus one value; ids cycle 0 1 2 (no repeats), or are random
    for g in (62, 63, 64, 126, 127):
        for extra in (0, 1):
            n = 8 * g + extra
            out.append(_int(f"packed{g}_{extra}", np.arange(n) % 3))
            out.append(_int(f"packed{g}_{extra}_rnd", _rng("packed", n).integers(0, 1 << 20, n) * 2 + np.arange(n) % 2))
    # a packed stretch, a run, a packed stretch of more than 63 groups: the header count restarts after the run
    out.append(_int("packed_run_packed", list(np.arange(520) % 3) + [9] * 30 + list(np.arange(1030) % 3)))
    # RLE counts at the varint edges; one value (width 0), and one value followed by another (width 1)
    for c in (63, 64, 8191, 8192, 20000):
        out.append(_int(f"rle{c}_w0", [5] * c))
        out.append(_int(f"rle{c}_w1", [5] * c + [6]))
    # stream lengths
    for n in (0, 1, 7, 8, 9):
        out.append(_int(f"len{n}", _rng("len", n).integers(0, 5, n)))
    # the stream ends inside a repeat of 7 (padded group) / of 8 (RLE run)
    out.append(_int("end_in_7", _noise(8) + [3] * 7))
    out.append(_int("end_in_7_mid", _noise(5) + [3] * 7))
    out.append(_int("end_in_8", _noise(8) + [3] * 8))
    # widths 0, 1, 2, 7, 8, 9 through dictionaries of 1 .. 257 values
    for d in (1, 2, 3, 100, 256, 257):
        out.append(_int(f"dict{d}", _dict_values(d, 1000, "w")))
        present = _rng("dictnull", d).random(1000) >= 0.3
        out.append(_int(f"dict{d}_nulls_136", _dict_values(d, int(present.sum()), "n"), present=present, page_rows=136))
    return out


def _level_cases():
    out = []
    for pr, rows in ((64, 6000), (136, 6000), (DEFAULT_PAGE_ROWS, 45000)):
        masks = {"allpresent": np.ones(rows, bool), "allnull": np.zeros(rows, bool), "alternating": np.arange(rows) % 2 == 0,
                 "nulls30": _rng("nulls30", rows, pr).random(rows) >= 0.3, "stretches": _null_stretches(rows, pr)}
        for name, m in masks.items():
            dense = _rng("lv", name, pr).integers(0, 50, int(m.sum()))
            out.append(_int(f"lv_{name}_{pr}", dense, present=m, page_rows=pr))
    # one page larger than any tile of the kernel, with long and short stretches
    m = _null_stretches(45000, "onepage")
    out.append(_int("lv_stretches_onepage", _rng("lv1").integers(0, 3, int(m.sum())), present=m, page_rows=45000))
    return out


def _boolean_cases():
    out = []
    for fam in ("constant", "alternating", "random", "longruns"):
        for pr, rows in ((136, 1000), (DEFAULT_PAGE_ROWS, 45000)):
            out.append(Case(f"b_{fam}_req_{pr}", K.BOOLEAN, _bool_family(fam, rows, "req"), page_rows=pr))
            m = _rng("bnull", fam, pr).random(rows) >= 0.3
            out.append(Case(f"b_{fam}_nulls_{pr}", K.BOOLEAN, _bool_family(fam, int(m.sum()), "nulls"), present=m, page_rows=pr))
            m = (np.arange(rows) // pr) % 2 == 0          # an all-null page next to a full one
            out.append(Case(f"b_{fam}_nullpage_{pr}", K.BOOLEAN, _bool_family(fam, int(m.sum()), "np"), present=m, page_rows=pr))
    return out


def _large_dict_cases():
    """Widths 16 and 17: dictionaries of 65,536 and 65,537 values, one 70,000-row chunk each."""
    return [_int(f"dict{d}", _dict_values(d, 70000, "large")) for d in (65536, 65537)]


_CACHE = {}


def _all():
    if "files" not in _CACHE:
        files = {}
        for c in _small_cases() + _level_cases() + _boolean_cases() + _large_dict_cases():
            files.setdefault(f"r{c.rows}", []).append(c)
        for fid, cases in files.items():
            assert len({c.name for c in cases}) == len(cases), fid
        _CACHE["files"] = files
    return _CACHE["files"]


def file_cases(fid):
    """(rows, cases) of a file; built once and shared (callers must not modify the arrays)."""
    return int(fid[1:]), _all()[fid]


FILE_IDS = tuple(sorted(_all(), key=lambda f: int(f[1:])))
