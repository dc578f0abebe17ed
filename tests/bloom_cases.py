"""Reference of the split-block Bloom filter tests (test-only; no product code is imported here).

The format's rules (parquet-format BloomFilter.md), restated from the values alone:
  * every present value is hashed with XXH64, seed 0, over its PLAIN bytes (BYTE_ARRAY: without the length prefix;
    FLOAT / DOUBLE: the bits);
  * a filter of `nbytes` is nbytes / 32 blocks of eight uint32 words; a hash h picks block ((h >> 32) * blocks) >> 32
    and sets bit ((uint32)h * SALT[i]) >> 27 of word i, for i in 0..7;
  * it is stored as a Thrift compact BloomFilterHeader {1 numBytes, 2 {1 BLOCK}, 3 {1 XXHASH}, 4 {1 UNCOMPRESSED}}
    followed by the words, little-endian.
test_write_bloom_cpu.py pins all of it to the bytes pyarrow writes."""
import math
import struct

import numpy as np

import pagekit as K

M64 = (1 << 64) - 1
P1, P2, P3, P4, P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                      0x27D4EB2F165667C5)
SALT = (0x47b6137b, 0x44974d91, 0x8824ad5b, 0xa2b7289d, 0x705495c7, 0x2df1424b, 0x9efc4947, 0x5c6bfb31)
MIN_BYTES, MAX_BYTES = 32, 128 << 20


# ---------------------------------------------------------------- XXH64, pure Python
def _rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & M64


def _round(acc, lane):
    return (_rotl((acc + lane * P2) & M64, 31) * P1) & M64


def _merge(h, v):
    return ((h ^ _round(0, v)) * P1 + P4) & M64


def xxh64(data, seed=0):
    data = bytes(data)
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M64, (seed + P2) & M64, seed & M64, (seed - P1) & M64]
        while n - p >= 32:
            lanes = struct.unpack_from("<4Q", data, p)
            v = [_round(v[i], lanes[i]) for i in range(4)]
            p += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M64
        for x in v:
            h = _merge(h, x)
    else:
        h = (seed + P5) & M64
    h = (h + n) & M64
    while n - p >= 8:
        h ^= _round(0, struct.unpack_from("<Q", data, p)[0])
        h = (_rotl(h, 27) * P1 + P4) & M64
        p += 8
    if n - p >= 4:
        h ^= (struct.unpack_from("<I", data, p)[0] * P1) & M64
        h = (_rotl(h, 23) * P2 + P3) & M64
        p += 4
    while p < n:
        h ^= (data[p] * P5) & M64
        h = (_rotl(h, 11) * P1) & M64
        p += 1
    h ^= h >> 33
    h = (h * P2) & M64
    h ^= h >> 29
    h = (h * P3) & M64
    return h ^ (h >> 32)


assert xxh64(b"") == 0xEF46DB3751D8E999 and xxh64(b"abc") == 0x44BC2CF5AD770999
try:   # the published implementation, where it is installed
    import xxhash as _xxhash
except ImportError:
    _xxhash = None
if _xxhash is not None:
    _probe = bytes((i * 37 + 11) & 0xff for i in range(300))
    for _n in list(range(0, 101)) + [255, 256, 257, 300]:
        for _seed in (0, 0x9E3779B97F4A7C15):
            assert xxh64(_probe[:_n], _seed) == _xxhash.xxh64(_probe[:_n], seed=_seed).intdigest(), (_n, _seed)


def hashes_fixed(arr):
    """XXH64, seed 0, of every item of a 4- or 8-byte numpy array (its bits), vectorised: the function above for an
    input of exactly one 4-byte or one 8-byte step."""
    a = np.ascontiguousarray(arr)
    u = np.uint64
    with np.errstate(over="ignore"):
        def rotl(v, r):
            return (v << u(r)) | (v >> u(64 - r))
        if a.dtype.itemsize == 4:
            k = a.view(np.uint32).astype(u)
            h = u((P5 + 4) & M64) ^ (k * u(P1))
            h = rotl(h, 23) * u(P2) + u(P3)
        else:
            assert a.dtype.itemsize == 8
            k = a.view(u)
            h = u((P5 + 8) & M64) ^ (rotl(k * u(P2), 31) * u(P1))
            h = rotl(h, 27) * u(P1) + u(P4)
        h = h ^ (h >> u(33))
        h = h * u(P2)
        h = h ^ (h >> u(29))
        h = h * u(P3)
        return h ^ (h >> u(32))


for _v in (np.array([0, 1, -1, 123456789], np.int32), np.array([0, 1, -1, 1 << 62], np.int64),
           np.array([0.0, -0.0, float("nan"), 1.5], np.float32), np.array([0.0, -0.0, float("inf"), 2.5], np.float64)):
    assert [int(x) for x in hashes_fixed(_v)] == [xxh64(_v[i:i + 1].tobytes()) for i in range(len(_v))]


def hashes_bytes(values):
    return np.array([xxh64(v) for v in values], np.uint64)


# ---------------------------------------------------------------- the filter
def build_filter(hashes, nbytes):
    """The bitset (nbytes bytes) that holds `hashes` (uint64 array)."""
    assert nbytes >= MIN_BYTES and nbytes & (nbytes - 1) == 0
    nb = nbytes // 32
    h = np.asarray(hashes, np.uint64)
    words = np.zeros((nb, 8), np.uint32)
    blk = (((h >> np.uint64(32)) * np.uint64(nb)) >> np.uint64(32)).astype(np.int64)
    lo = (h & np.uint64(0xffffffff)).astype(np.uint32)
    with np.errstate(over="ignore"):
        for i in range(8):
            bit = (lo * np.uint32(SALT[i])) >> np.uint32(27)
            np.bitwise_or.at(words[:, i], blk, np.uint32(1) << bit)
    return words.astype("<u4").tobytes()


def might_contain(bitset, h):
    nb = len(bitset) // 32
    blk = (((h >> 32) * nb) >> 32) * 32
    for i in range(8):
        word = struct.unpack_from("<I", bitset, blk + 4 * i)[0]
        if not word >> ((((h & 0xffffffff) * SALT[i]) & 0xffffffff) >> 27) & 1:
            return False
    return True


def header(nbytes):
    """BloomFilterHeader, Thrift compact: field 1 i32 numBytes (zigzag varint), fields 2..4 a struct holding the empty
    struct 1 (BLOCK, XXHASH, UNCOMPRESSED), stop."""
    v, out = nbytes << 1, bytearray([0x15])
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out) + b"\x1c\x1c\x00\x00" * 3 + b"\x00"


assert header(4096) == bytes.fromhex("1580401c1c00001c1c00001c1c000000")


def optimal_bytes(ndv, fpp, max_bytes=MAX_BYTES):
    """bits = -8 ndv / ln(1 - fpp^(1/8)); bytes rounded up to a power of two in [32, max_bytes]."""
    bits = int(-8.0 * ndv / math.log(1.0 - fpp ** 0.125))
    nbytes = MIN_BYTES
    while nbytes * 8 < bits:
        nbytes *= 2
    return min(nbytes, max_bytes)


# ---------------------------------------------------------------- cases
_NP = {K.INT32: np.int32, K.INT64: np.int64, K.FLOAT: np.float32, K.DOUBLE: np.float64}
_ARROW = {K.INT32: "int32", K.INT64: "int64", K.FLOAT: "float32", K.DOUBLE: "float64", K.BYTE_ARRAY: "binary"}


class Case:
    """One column: fixed-width `values` (numpy array, row-indexed) or a list of bytes, and `present` (bool per row,
    None: REQUIRED). Null rows hold a value that must never reach the filter."""

    def __init__(self, name, ptype, values, present=None, page_rows=0, char_pad=0):
        self.name, self.ptype, self.page_rows, self.char_pad = name, ptype, page_rows, char_pad
        self.optional = present is not None
        self.rows = len(values)
        self.present = None if present is None else np.asarray(present, bool)
        self.values = values if ptype == K.BYTE_ARRAY else np.asarray(values, _NP[ptype])
        self._hashes = None

    def present_values(self):
        if self.present is None:
            return self.values
        if self.ptype == K.BYTE_ARRAY:
            return [v for v, p in zip(self.values, self.present) if p]
        return self.values[self.present]

    def hashes(self):
        if self._hashes is None:
            pv = self.present_values()
            if self.ptype == K.BYTE_ARRAY:
                self._hashes = hashes_bytes(pv)
            else:
                self._hashes = hashes_fixed(pv) if len(pv) else np.zeros(0, np.uint64)
            self._hashes.setflags(write=False)
        return self._hashes

    def filter(self, nbytes):
        return build_filter(self.hashes(), nbytes)

    def distinct(self):
        return len(np.unique(self.hashes()))

    def pyarrow_bytes(self, ndv, fpp):
        """The size pyarrow 25 gives this column's filter under {"ndv": ndv, "fpp": fpp}: it sizes for the distinct
        values it saw when they are fewer than ndv (measured: 600 distinct values in 5,000 rows with ndv = 10^6,
        fpp = 0.01 get the 1,024 bytes of ndv = 600; so do 600 with ndv = 5,000)."""
        return optimal_bytes(min(ndv, self.distinct()), fpp)

    def row_arrays(self):
        """(values | (offsets, chars), validity or None) as pf_encode_chunk takes them. Strings: `char_pad` unused
        bytes in front of the first value, so that values start at odd addresses; null rows are empty."""
        validity = None if self.present is None else np.packbits(self.present, bitorder="little")
        if self.ptype != K.BYTE_ARRAY:
            return self.values, validity
        keep = [v if (self.present is None or self.present[i]) else b"" for i, v in enumerate(self.values)]
        offsets = np.zeros(self.rows + 1, np.int64)
        if self.rows:
            np.cumsum([len(v) for v in keep], out=offsets[1:])
        offsets += self.char_pad
        chars = np.frombuffer(b"\xa5" * self.char_pad + b"".join(keep), np.uint8)
        return (offsets.astype(np.int32), chars), validity

    def arrow(self):
        import pyarrow as pa
        mask = None if self.present is None else ~self.present
        if self.ptype == K.BYTE_ARRAY:
            return pa.array([v if (mask is None or not mask[i]) else None for i, v in enumerate(self.values)], pa.binary())
        return pa.array(self.values, _ARROW[self.ptype], mask=mask)


def _nulls(rng, n, frac=0.3):
    return rng.random(n) >= frac


def _fixed(ptype, rng, n, distinct=None):
    """n values of the type; `distinct`: drawn from that many."""
    pool_n = distinct or n
    if ptype == K.INT32:
        pool = rng.integers(-(1 << 31), 1 << 31, pool_n, dtype=np.int64).astype(np.int32)
    elif ptype == K.INT64:
        pool = rng.integers(-(1 << 63), (1 << 63) - 1, pool_n, dtype=np.int64)
    elif ptype == K.FLOAT:
        pool = (rng.standard_normal(pool_n) * 1e3).astype(np.float32)
    else:
        pool = rng.standard_normal(pool_n) * 1e6
    return pool[rng.integers(0, pool_n, n)] if distinct else pool


def _words(rng, n, distinct=None):
    pool_n = distinct or n
    pool = [b"k%d-" % i + bytes(rng.integers(0x61, 0x7b, int(rng.integers(0, 24))).astype(np.uint8)) for i in range(pool_n)]
    return [pool[i] for i in rng.integers(0, pool_n, n)] if distinct else pool


TYPES = {"int32": K.INT32, "int64": K.INT64, "float": K.FLOAT, "double": K.DOUBLE, "binary": K.BYTE_ARRAY}
# dictionary bits of pf_encode_column besides the filter, by route
ROUTES = {"plain": dict(dictionary=False),
          "dictionary": dict(dictionary=True),
          "dict_over_limit": dict(dictionary=True, dict_page_limit=1),   # fallback 1
          "delta_fallback": dict(dictionary=False, delta_fallback=True),
          "all_bits": dict(dictionary=True, delta_fallback=True, hybrid_runs=True, statistics=True, page_checksums=True)}
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 4097, 70000)
SIZES = (32, 64, 1024, 1 << 20)

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def typed(tname, nulls=False):
    """5,000 rows drawn from 600 values (a dictionary that fits), two pages; with 30 % nulls on request."""
    def make():
        rng = np.random.default_rng(1000 + len(tname) + 7 * nulls + sum(tname.encode()))
        t = TYPES[tname]
        vals = _words(rng, 5000, 600) if t == K.BYTE_ARRAY else _fixed(t, rng, 5000, 600)
        return Case(f"{tname}{'_n' if nulls else ''}", t, vals, _nulls(rng, 5000) if nulls else None, page_rows=3000)
    return _once(("typed", tname, nulls), make)


def counted(n, nulls):
    """n rows of distinct INT64 values (pages of 20,000 rows: 70,000 rows are four pages and 274 workgroups)."""
    def make():
        rng = np.random.default_rng(2000 + n + nulls)
        return Case(f"i64_{n}{'_n' if nulls else ''}", K.INT64, _fixed(K.INT64, rng, n), _nulls(rng, n) if nulls else None)
    return _once(("counted", n, nulls), make)


def counted_strings(n, nulls):
    def make():
        rng = np.random.default_rng(3000 + n + nulls)
        return Case(f"ba_{n}{'_n' if nulls else ''}", K.BYTE_ARRAY, _words(rng, n), _nulls(rng, n) if nulls else None)
    return _once(("counted_strings", n, nulls), make)


def all_null(tname):
    t = TYPES[tname]
    vals = [b"never"] * 500 if t == K.BYTE_ARRAY else np.full(500, 7, _NP[t])
    return Case(f"{tname}_all_null", t, vals, np.zeros(500, bool))


def three_values(tname):
    """3 distinct values x 20,000: a D = 3 dictionary over 60,000 rows."""
    t = TYPES[tname]
    base = [b"", b"x", b"a-longer-value-of-37-bytes-0123456789"] if t == K.BYTE_ARRAY else np.array([0, 1, -5], _NP[t])
    idx = np.arange(60000) % 3
    return Case(f"{tname}_three", t, [base[i] for i in idx] if t == K.BYTE_ARRAY else base[idx])


def float_specials(tname):
    """NaNs of both signs with payloads, +-0.0, +-inf, subnormals, as raw bits; repeated so that pages and a dictionary form."""
    if tname == "float":
        bits = np.array([0x7fc00000, 0xffc00000, 0x7fc00001, 0x7f800001, 0xffbfffff, 0x00000000, 0x80000000, 0x7f800000,
                         0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x3f800000], np.uint32)
        vals = np.tile(bits, 40).view(np.float32)
    else:
        bits = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000001, 0x7ff0000000000001,
                         0xfff7ffffffffffff, 0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000,
                         0xfff0000000000000, 0x0000000000000001, 0x8000000000000001, 0x000fffffffffffff,
                         0x3ff0000000000000], np.uint64)
        vals = np.tile(bits, 40).view(np.float64)
    present = np.ones(len(vals), bool)
    present[::7] = False
    return Case(f"{tname}_specials", TYPES[tname], vals, present, page_rows=200)


def string_cases():
    """name -> Case: the tail branches and loop boundaries of XXH64, long values, arbitrary bytes, odd addresses,
    empty strings present and null."""
    def make():
        rng = np.random.default_rng(4000)
        raw = bytes(rng.integers(0, 256, 8192).astype(np.uint8))
        out = {}
        # every length 0..70 (tails of 8, 4 and 1 bytes; the 32-byte loop at 31 / 32 / 33 / 63 / 64 / 65), arbitrary
        # bytes; one pad byte in front, so that with the lengths 0, 1, 2, ... the values start at every alignment
        out["lengths_0_70"] = Case("lengths_0_70", K.BYTE_ARRAY, [raw[7 * n:7 * n + n] for n in range(71)], char_pad=1)
        long_ = [raw[:255], raw[1:257], raw[3:1003], raw[5:4102]]
        mix = []
        for i in range(300):
            mix.append(long_[(i // 60) % 4] if i % 60 == 17 else b"s%d" % i)
        out["long_among_short"] = Case("long_among_short", K.BYTE_ARRAY, mix, char_pad=3)
        out["bytes_00_ff"] = Case("bytes_00_ff", K.BYTE_ARRAY,
                                  [b"\x00", b"\xff", b"\x00\x00", b"\xff\x00\xff", b"\x00" * 33, b"\xff" * 64, b"a\x00b", b"\x80\x7f"] * 20,
                                  char_pad=1)
        present = np.array([(i % 3) != 1 for i in range(90)])
        out["empty_present_and_null"] = Case("empty_present_and_null", K.BYTE_ARRAY,
                                             [b"" if i % 2 == 0 else b"v%d" % i for i in range(90)], present)
        out["only_empty"] = Case("only_empty", K.BYTE_ARRAY, [b""] * 10)
        return out
    return _once("strings", make)


def pyarrow_options(nbytes, distinct):
    """bloom_filter_options for which pyarrow writes a filter of `nbytes` over a chunk of `distinct` distinct values
    (Case.pyarrow_bytes: ndv above that count is of no effect, so search ndv <= distinct and the fpp)."""
    for fpp in (0.01, 0.05, 0.001, 0.2, 1e-5, 1e-6, 1e-7, 1e-8):
        for ndv in sorted({max(1, distinct >> s) for s in range(24)} | {max(1, distinct * k // 16) for k in range(1, 17)}, reverse=True):
            if optimal_bytes(ndv, fpp) == nbytes:
                return {"ndv": ndv, "fpp": fpp}
    raise ValueError(f"no pyarrow options give {nbytes} bytes over {distinct} distinct values")
