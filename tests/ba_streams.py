"""PLAIN BYTE_ARRAY value streams that stress the guess-and-verify value walk (TEST INFRASTRUCTURE ONLY).

The walk (k_ba_tile or k_ba_cand / k_ba_link / k_ba_count, k_ba_scan, k_ba_emit, k_ba_verify,
k_ba_fallback with ba_relink_wg and binary_walk_wg, pf_ba.hip) guesses the <len><bytes> chain from
the positions whose 4-byte length fits the stream and verifies the guess. Text never produces a
fitting length away from a true prefix, so a suite of text never challenges the verification. The
cases here are binary payloads full of fitting lengths, and text streams whose one interesting prefix
or value end lands on a chosen byte of the tile geometry. Pure Python / numpy over pagekit: nothing is
imported from the product, and the expected values are the constructed ones.

corpus() returns {file id: [Case]}: the cases of one id are the chunks of one file (one decode call).
"""
import numpy as np

import pagekit as K

# The walk's own constants, restated (never imported).
BA_TILE = 8192       # BA_TILE, pf_internal.h    stream bytes per k_ba_* tile
BA_SHORT = 48        # BA_SHORT, pf_internal.h   page bytes per value up to which a batch takes the fused k_ba_tile
BA_HALO = 128        # BA_HALO, pf_ba.hip        k_ba_tile links a successor at most this far from its prefix
BA_MAX_LINKED = 124  # k_ba_tile, pf_ba.hip      sv - q <= BA_HALO with sv = q + 4 + len: the longest value linked in a tile
BA_STAGE_END = 176   # BA_FSTAGE, pf_ba.hip      3 * 128 + 8192 + 48 staged from t0 - 256: the stage ends at t1 + 176
BW_TILE = 1024       # BW_TILE, pf_ba.hip        binary_walk_wg: stream bytes per tile
BW_LOOK = 64         # BW_LOOK, pf_ba.hip        binary_walk_wg: staged lookahead
BW_CAP = 256         # BW_CAP, pf_ba.hip         binary_walk_wg: candidates per tile
MAX_STREAM = 3 * BA_TILE

T1 = BA_TILE         # the first tile's end: where the geometry cases aim

FAMILIES = ("text", "zeros", "empty", "low", "u32", "stream_in_value", "phase", "random")
# Binary pages the filters do get right, with false positions around the chain they accept: uniform bytes
# 1-255 (no zero byte, so none of the one-byte values that "random" loses to the adjacency rule), and the
# same with a few values past the halo (re-linked on the fused route).
EXTRA = ("random_nz", "random_nz_long")


class Case:
    """One stream and where it sits. `vals` is what a reader must return (for a damaged stream the
    reference reads: its clean values; for one it rejects they are placeholders), `stream` the value
    section, `present` the null mask of a flat OPTIONAL page (None: REQUIRED), `where` "data" or
    "dict" (the PLAIN dictionary page of a dictionary chunk whose data page holds 300 random ids),
    `filler` the byte length of the one value of a page put ahead of the page under test (None: no
    such page), `damage` a short name for damaged streams, `land` {label: stream position} of the
    positions the geometry builder aimed at (asserted there)."""

    def __init__(self, name, payload, vals, stream=None, present=None, where="data", layout="a", nested=False,
                 geometry="", filler=None, damage=None, land=None):
        self.name, self.payload, self.vals = name, payload, list(vals)
        self.stream = K.plain(K.BYTE_ARRAY, self.vals) if stream is None else stream
        self.present, self.where, self.layout, self.nested = present, where, layout, nested
        self.geometry, self.filler, self.damage, self.land = geometry, filler, damage, dict(land or {})

    @property
    def count(self):
        return len(self.vals)

    def page_bytes_per_value(self):
        """What plan_ba_walks (pf_plan.cpp:269) compares with BA_SHORT, at most: the page body
        (a v1 page's levels included, bounded here: a bit per flat entry, three bits for each of the about 1.5
        entries per value of a LIST leaf, and the run headers) over its value count; the CPU test checks
        the assembled pages themselves."""
        levels = self.count + 16 if self.nested else 0 if self.present is None else len(self.present) // 4 + 16
        return (len(self.stream) + levels) / max(1, self.count)

    def short(self):
        return self.page_bytes_per_value() <= BA_SHORT

    def describe(self):
        return (f"{self.name}: payload={self.payload} geometry={self.geometry or '-'} where={self.where} "
                f"layout={self.layout} nested={self.nested} nulls={self.present is not None} "
                f"n={len(self.stream)} count={self.count}" + (f" damage={self.damage}" if self.damage else ""))

    def but(self, name, **kw):
        """The same stream somewhere else."""
        d = dict(payload=self.payload, vals=self.vals, stream=self.stream, present=self.present, where=self.where,
                 layout=self.layout, nested=self.nested, geometry=self.geometry, filler=self.filler,
                 damage=self.damage, land=self.land)
        d.update(kw)
        return Case(name, **d)


def _rng(*key):
    return np.random.default_rng(sum(ord(c) * (i + 7) for i, c in enumerate("/".join(map(str, key)))))


# ---------------------------------------------------------------- payloads
def _bytes(rng, kind, n):
    if kind == "text":
        return (rng.integers(0, 26, n) + 97).astype(np.uint8).tobytes()
    if kind == "zeros":
        return bytes(n)
    if kind == "low":
        # bytes 0-3, zero a little over half the time: a window reads as a fitting length when its two
        # high bytes are zero (0.3 of the positions; 1 / 16 with a uniform draw, which leaves too few
        # positions whose successor fits as well for the two-false-positions-per-value condition)
        return rng.choice(np.arange(4, dtype=np.uint8), n, p=(0.55, 0.15, 0.15, 0.15)).tobytes()
    assert kind in ("random", "random_nz"), kind
    return rng.integers(kind == "random_nz", 256, n).astype(np.uint8).tobytes()


def _cut(blob, lens):
    ends = np.cumsum(lens)
    return [blob[int(e - ln):int(e)] for e, ln in zip(ends, lens)]


def _fit(vals, limit=MAX_STREAM):
    """Drop values from the end until the stream is at most `limit` bytes."""
    total = sum(4 + len(v) for v in vals)
    while total > limit:
        total -= 4 + len(vals.pop())
    return vals


def family(kind, seed=1):
    """The values of payload family `kind` (FAMILIES), at most three tiles of stream and at most
    BA_SHORT bytes of page per value."""
    rng = _rng("family", kind, seed)
    if kind in ("text", "zeros", "random"):
        lens = rng.integers(0, 40, 1000)
        vals = _cut(_bytes(rng, kind, int(lens.sum())), lens)
    elif kind in EXTRA:
        lens = rng.integers(0, 40, 900)
        if kind == "random_nz_long":
            lens[50::100] = rng.integers(125, 400, len(lens[50::100]))
        vals = _cut(_bytes(rng, "random_nz", int(lens.sum())), lens)
    elif kind == "empty":        # every position is a fitting length
        vals = [b""] * 5000
    elif kind == "low":
        lens = rng.integers(0, 60, 700)
        vals = _cut(_bytes(rng, "low", int(lens.sum())), lens)
    elif kind == "u32":          # 0-11 packed little-endian integers below 50 per value
        vals = [rng.integers(0, 50, int(k)).astype("<u4").tobytes() for k in rng.integers(0, 12, 900)]
    elif kind == "stream_in_value":
        # a value is itself a PLAIN stream of 0-8 text values: every inner chain is self-consistent and
        # ends where the next true prefix starts, so inner values from the third on have both links
        vals = []
        for k in rng.integers(0, 9, 560):
            lens = rng.integers(0, 12, int(k))
            vals.append(K.plain(K.BYTE_ARRAY, _cut(_bytes(rng, "text", int(lens.sum())), lens)))
    elif kind == "phase":
        # <text 8-30> <1-3 zero bytes> <empty> x 4: after the short value's length byte come 19 + k zero
        # bytes, so q + 1, q + 2 and q + 3 of its prefix q each read 0, 0, 0, ... : three or more links
        # of a chain 1, 2 or 3 bytes out of phase with the true one (which also runs through the zeros)
        vals = []
        for i, ln in enumerate(rng.integers(8, 31, 500)):
            vals += [_bytes(rng, "text", int(ln)), bytes(1 + i % 3), b"", b"", b"", b""]
    else:
        raise AssertionError(kind)
    return _fit(vals)


# ---------------------------------------------------------------- the counting rule of the CPU check
def fitting(stream):
    """fit[q]: the little-endian length at q fits the stream (q + 4 + len <= n), for q in [0, n - 4]."""
    b = np.frombuffer(stream, np.uint8).astype(np.int64)
    n = len(b)
    if n < 4:
        return np.zeros(0, bool), np.zeros(0, np.int64)
    ln = b[:n - 3] | (b[1:n - 2] << 8) | (b[2:n - 1] << 16) | (b[3:] << 24)
    q = np.arange(n - 3)
    return ln <= n - q - 4, q + 4 + ln


def false_positions(stream, vals):
    """(false positions, those of them at the end of a three-link chain of false positions). A false
    position is not a true prefix, its length fits, and the position after its value is the stream end
    or again a fitting length (the format's own statement of the walk's candidate test)."""
    n = len(stream)
    fit, succ = fitting(stream)
    if len(fit) == 0:
        return 0, 0
    s = np.where(fit, succ, 0)
    nxt_ok = (s == n) | ((s + 4 <= n) & fit[np.minimum(s, len(fit) - 1)])
    false = fit & nxt_ok
    true = np.cumsum([0] + [4 + len(v) for v in vals])[:-1]
    false[true[true < len(false)]] = False
    link1 = np.zeros(len(false), bool)
    src = np.flatnonzero(false & (s < len(false)))
    link1[s[src]] = True
    link1 &= false
    link2 = np.zeros(len(false), bool)
    src = np.flatnonzero(link1 & (s < len(false)))
    link2[s[src]] = True
    link2 &= false
    return int(false.sum()), int(link2.sum())


# ---------------------------------------------------------------- geometry builders
class _Stream:
    """Values appended one by one, with the stream position known."""

    def __init__(self, key, pad="text"):
        self.rng, self.vals, self.pos, self.pad, self.land = _rng("geometry", key), [], 0, pad, {}

    def add(self, v):
        self.vals.append(v)
        self.pos += 4 + len(v)
        return self

    def pad_to(self, target):
        """8-byte text values and one of adjusted length: the next prefix starts at `target`."""
        d = target - self.pos
        assert d == 0 or d >= 4, (self.pos, target)
        while d >= 16:
            self.add(_bytes(self.rng, self.pad, 8))
            d -= 12
        if d:
            self.add(_bytes(self.rng, self.pad, d - 4))
        assert self.pos == target, (self.pos, target)
        return self

    def at(self, label, target, v):
        """Value v with its prefix at `target`."""
        self.pad_to(target)
        self.land[label] = self.pos
        return self.add(v)

    def some(self, k, lo=8, hi=31):
        for ln in self.rng.integers(lo, hi, k):
            self.add(_bytes(self.rng, self.pad, int(ln)))
        return self

    def case(self, name, payload, geometry, **kw):
        true = np.cumsum([0] + [4 + len(v) for v in self.vals])
        for label, p in self.land.items():   # every landing position is a true prefix (or the stream end)
            assert p in true, (name, label, p)
        return Case(name, payload, self.vals, geometry=geometry, land=self.land, **kw)


def _text(s, n):
    return _bytes(s.rng, "text", n)


def straddle_cases():
    """A prefix k bytes before the end of a tile: the 4-byte length straddles the boundary by 0-3 bytes
    (k = 4, 5: the last whole prefix and one earlier). At the 8 KiB tile of the k_ba_* kernels, and at
    the 1 KiB tile of binary_walk_wg, where one complete extra record after the page's last value
    (which a reader ignores) makes the count check fail, so the page is walked there."""
    out = []
    for k in range(6):
        s = _Stream(f"straddle{k}")
        s.at("prefix", T1 - k, _text(s, 20)).some(12)
        out.append(s.case(f"straddle_t1-{k}", "text", f"prefix at t1-{k}"))
    for k in range(6):
        s = _Stream(f"bwstraddle{k}")
        s.at("prefix", BW_TILE - k, _text(s, 20)).at("prefix2", 3 * BW_TILE - k, _text(s, 5)).some(12)
        c = s.case(f"bw_straddle_1k-{k}", "text", f"prefix at 1024-{k} and 3072-{k}, extra record", damage="extra_record")
        c.stream += K.plain(K.BYTE_ARRAY, [b"extra"])
        out.append(c)
    return out


def value_end_cases():
    """A value ending exactly at t1, t1 + 127 and t1 + 128 (the end of k_ba_tile's window), and a
    successor prefix at t1 + 172 / 173 / 176 (the last staged length, the first one not staged, the
    stage end: r + 4 > BA_FSTAGE in k_ba_tile, pf_ba.hip)."""
    out = []
    for end in (0, 127, 128):
        s = _Stream(f"end{end}")
        s.at("prefix", T1 + end - 4 - 100, _text(s, 100))
        assert s.pos == T1 + end
        s.land["end"] = s.pos
        s.some(12)
        out.append(s.case(f"value_end_t1+{end}", "text", f"100-byte value ends at t1+{end}"))
    for nxt in (BA_STAGE_END - 4, BA_STAGE_END - 3, BA_STAGE_END):
        s = _Stream(f"succ{nxt}")
        s.at("prefix", T1 + nxt - 4 - 100, _text(s, 100))   # a candidate inside the window (< t1 + 128)
        assert s.land["prefix"] < T1 + BA_HALO and s.pos == T1 + nxt
        s.land["successor"] = s.pos
        s.some(12)
        out.append(s.case(f"successor_t1+{nxt}", "text", f"successor prefix at t1+{nxt}"))
    return out


HALO_LENGTHS = (123, 124, 125, 128)
HALO_PLACES = ("mid", "t1-1", "t1-128", "t1-129", "first", "last")


def halo_case(length, place):
    """One value of `length` bytes among 8-30-byte text values."""
    s = _Stream(f"halo{length}{place}")
    v = _text(s, length)
    if place == "first":
        s.at("prefix", 0, v).some(40)
    elif place == "last":
        s.some(40).at("prefix", s.pos, v)
    else:
        s.some(20)
        s.at("prefix", {"mid": 4000, "t1-1": T1 - 1, "t1-128": T1 - 128, "t1-129": T1 - 129}[place], v).some(20)
    return s.case(f"halo_{length}_{place}", "text", f"{length}-byte value, {place}")


LONG_LENGTHS = (8188, 8192, 8193, 16384 + 5, 20000)


def long_case(length, payload, among):
    """One long value, alone in its page or among enough 8-byte values (12 bytes of stream each) that the
    page stays at BA_SHORT bytes per value, so the batch keeps the fused walk."""
    s = _Stream(f"long{length}{payload}{among}", pad=payload)
    v = _bytes(s.rng, payload, length)
    if among:
        k = (length + 4) // 30 + 8   # (length + 4 + 12 k) / (k + 1) < 43
        s.some(k // 2, 8, 9).at("prefix", s.pos, v).some(k - k // 2, 8, 9)
    else:
        s.at("prefix", 0, v)
    return s.case(f"long_{length}_{payload}_{'among' if among else 'alone'}", payload,
                  f"{length}-byte value {'among 8-byte values' if among else 'alone'}")


STREAM_SIZES = (4, 5, 8191, 8192, 8193, 8196, 16384, 3 * BA_TILE)


def size_cases():
    """Streams of exactly n bytes (the tile count, t0 >= n for a planned tile past the value section
    of a nullable v1 page), and pages of 1, 2 and 3 values (values 0 and 1 reach link level 2 only
    through the position-0 rule)."""
    out = []
    for n in STREAM_SIZES:
        s = _Stream(f"size{n}")
        s.pad_to(n)
        s.land["end"] = s.pos
        assert len(K.plain(K.BYTE_ARRAY, s.vals)) == n
        c = s.case(f"size_{n}", "text", f"stream of {n} bytes")
        out += [c, c.but(f"size_{n}_opt", present=_present(c.count, n))]
    for k in (1, 2, 3):
        s = _Stream(f"count{k}").some(k, 10, 11)
        c = s.case(f"count_{k}", "text", f"page of {k} values")
        out += [c, c.but(f"count_{k}_opt", present=_present(k, k)), c.but(f"count_{k}_dict", where="dict")]
    return out


def residue_cases(payload):
    """The page under test behind a filler page of one r-byte value, r = 0..15: the value section's
    offset inside its chunk takes every residue mod 16 (the decoder places chunks at 256-byte
    multiples, so for an uncompressed page that is the stream's device alignment). Layouts a and e
    decode in place; layout c is a Snappy page whose body goes to aligned scratch: one case."""
    rng = _rng("residue", payload)
    lens = rng.integers(0, 40, 360)
    vals = _cut(_bytes(rng, payload, int(lens.sum())), lens)
    assert BA_TILE < sum(4 + len(v) for v in vals) < BA_TILE + 1500
    out = [Case(f"residue_{payload}_{lay}_{r}", payload, vals, layout=lay, filler=r, geometry=f"filler page of {r} bytes")
           for lay in ("a", "e") for r in range(16)]
    out.append(Case(f"residue_{payload}_c", payload, vals, layout="c", filler=3, geometry="Snappy page"))
    return out


def _present(count, seed):
    """A null mask with `count` values and 25 % nulls."""
    p = np.ones(count + count // 3 + (count < 3), bool)
    p[count:] = False
    _rng("present", count, seed).shuffle(p)
    return p


# ---------------------------------------------------------------- damaged streams
def damaged_cases():
    """Streams a reader must reject, and streams with bytes after the last value that it reads as if
    they were not there. The expected verdict is the reference reader's (the oracle's), taken by the
    tests; `vals` holds the clean values for the streams it accepts."""
    base = family("text")[:300]
    clean = K.plain(K.BYTE_ARRAY, base)
    starts = np.cumsum([0] + [4 + len(v) for v in base])

    def patch(pos, value):
        b = bytearray(clean)
        b[pos:pos + 4] = int(value).to_bytes(4, "little")
        return bytes(b)

    mid = 150
    five = np.ones(5, bool)
    out = [
        Case("trail_junk3", "text", base, stream=clean + b"\x07\xff\x01", damage="trail_junk3"),
        Case("trail_record", "text", base, stream=clean + K.plain(K.BYTE_ARRAY, [b"one more"]), damage="extra_record"),
        Case("trail_junk3_zeros", "zeros", family("zeros")[:300],
             stream=K.plain(K.BYTE_ARRAY, family("zeros")[:300]) + b"\x07\xff\x01", damage="trail_junk3"),
        Case("last_overrun", "text", base, stream=patch(int(starts[-2]), len(base[-1]) + 1), damage="last_overrun"),
        Case("mid_ffffffff", "text", base, stream=patch(int(starts[mid]), 0xFFFFFFFF), damage="mid_ffffffff"),
        # value `mid` swallows its successor: the chain is back on a true prefix, one value short
        Case("mid_resync", "text", base, stream=patch(int(starts[mid]), len(base[mid]) + 4 + len(base[mid + 1])),
             damage="mid_resync"),
        Case("empty_section", "text", [b""] * 5, stream=b"", present=five, damage="empty_section"),
        Case("three_bytes", "text", [b""] * 5, stream=b"\x00\x00\x00", present=five, damage="three_bytes"),
    ]
    out += [out[0].but("trail_junk3_dict", where="dict"), out[1].but("trail_record_dict", where="dict"),
            out[0].but("trail_junk3_v2", layout="e"), out[3].but("last_overrun_v2", layout="e")]
    return out


# ---------------------------------------------------------------- the corpus
def family_cases(where):
    """Every family as a REQUIRED data page ("req"), with 25 % nulls ("opt") or as the dictionary
    page ("dict"), v1 (layout a) and v2 (layout e)."""
    out = []
    for kind in FAMILIES + EXTRA:
        vals = family(kind)
        for lay in ("a", "e"):
            present = _present(len(vals), kind) if where == "opt" else None
            out.append(Case(f"{kind}_{where}_{lay}", kind, vals, present=present, layout=lay,
                            where="dict" if where == "dict" else "data"))
    return out


_CORPUS = None


def corpus():
    """{file id: [Case]}. The files "long-alone" and "dict-long" hold a page above BA_SHORT bytes per
    value (data pages / dictionary pages), which sends that batch's walks to the multi-kernel route in
    the product library; every other file stays at or under it, so all its walks are fused."""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    fam = {k: family(k) for k in FAMILIES}
    adversarial = [Case(f"{k}_req_a", k, fam[k]) for k in FAMILIES[1:7]]
    long_among = [long_case(n, p, True) for p in ("text", "low") for n in LONG_LENGTHS]
    long_alone = [long_case(n, p, False) for p in ("text", "low") for n in LONG_LENGTHS]
    files = {
        "families-req": family_cases("req"),
        "families-opt-list": family_cases("opt") + [Case(f"{k}_list", k, fam[k], nested=True) for k in ("zeros", "low", "stream_in_value")]
        + [long_case(20000, "low", True).but("long_20000_low_list", nested=True)],
        "families-dict": family_cases("dict"),
        "straddle-ends": straddle_cases() + value_end_cases(),
        "halo": [halo_case(n, p) for n in HALO_LENGTHS for p in HALO_PLACES],
        "long-among": long_among + [long_among[4].but("long_20000_text_opt", present=_present(long_among[4].count, 7)),
                                    long_among[9].but("long_20000_low_opt", present=_present(long_among[9].count, 8))],
        "sizes": size_cases(),
        "long-alone": long_alone + adversarial + [long_alone[1].but("long_8192_text_opt", present=_present(1, 9))],
        "dict-long": [long_alone[0].but("dict_long_8188_text", where="dict"),
                      long_case(20000, "low", False).but("dict_long_20000_low", where="dict")] + adversarial,
        "residue": residue_cases("zeros") + residue_cases("text"),
        "damaged": damaged_cases() + [Case("clean_text", "text", fam["text"]), Case("clean_zeros", "zeros", fam["zeros"]),
                                      Case("clean_dict", "text", fam["text"], where="dict")],
    }
    for fid, cases in files.items():
        names = [c.name for c in cases]
        assert len(set(names)) == len(names), (fid, names)
        for c in cases:
            long_point = c.name.startswith(("long_", "dict_long_"))
            assert len(c.stream) <= MAX_STREAM + 16 or long_point, c.describe()
            if fid not in ("long-alone", "dict-long"):
                assert c.short(), (fid, c.describe(), c.page_bytes_per_value())
    assert not all(c.short() for c in files["long-alone"] if c.where == "data")
    assert not all(c.short() for c in files["dict-long"] if c.where == "dict")
    assert all(c.short() for c in files["dict-long"] if c.where == "data")
    _CORPUS = files
    return files


# ---------------------------------------------------------------- chunks and files
def _list_structure(rng, n_values):
    """defs / reps of a LIST leaf page holding n_values values: null and empty lists, 1-4 elements, null elements."""
    defs, reps, left = [], [], n_values
    while left:
        r = rng.random()
        if r < 0.1:
            defs.append(0); reps.append(0)
        elif r < 0.2:
            defs.append(1); reps.append(0)
        else:
            k = int(rng.integers(1, 5))
            for j in range(k):
                d = 2 if (rng.random() < 0.15 or not left) else 3
                left -= d == 3
                defs.append(d); reps.append(int(j > 0))
    return np.array(defs, np.uint8), np.array(reps, np.uint8)


def chunk_of(case, compress):
    """The column chunk of a case (pagekit.Chunk, with its expected arrays)."""
    rng = _rng("chunk", case.name)
    lay = K.LAYOUTS[case.layout]
    if case.where == "dict":
        ch = K.Chunk(case.name, K.BYTE_ARRAY, layout=lay, compress=compress)
        body = ch._z(case.stream)   # (set_dictionary encodes the values itself; a damaged stream is given)
        hdr = K.dict_page_header(case.count, K.PLAIN, len(case.stream), len(body))
        ch.dict = hdr + body
        ch.usize += len(hdr) + len(case.stream)
        ch.encodings.add(K.PLAIN)
        ids = rng.integers(0, case.count, 300)
        bw = int(case.count - 1).bit_length()
        ch.add_page(K.RLE_DICTIONARY, K.dict_indices(ids, bw), vals=[case.vals[int(i)] for i in ids])
        return ch
    ch = K.Chunk(case.name, K.BYTE_ARRAY, optional=case.present is not None, nested=case.nested, layout=lay, compress=compress)
    if case.filler is not None:
        v = [_bytes(rng, "text", case.filler)]
        ch.add_page(K.PLAIN, K.plain(K.BYTE_ARRAY, v), vals=v)
    if case.nested:
        defs, reps = _list_structure(rng, case.count)
        ch.add_page(K.PLAIN, case.stream, defs=defs, reps=reps, vals=case.vals)
    else:
        ch.add_page(K.PLAIN, case.stream, present=case.present, vals=case.vals)
    return ch


def build(cases, compress):
    """(file bytes, info, chunks, expected arrays) of the cases as the chunks of one file."""
    chunks = [chunk_of(c, compress) for c in cases]
    data, info = K.build_file(chunks, max(ch.num_entries for ch in chunks))
    return data, info, chunks, [ch.expected() for ch in chunks]


def stream_residue(info_c):
    """The last page's value-section offset inside its chunk, mod 16."""
    return (info_c["values"][-1][0] - info_c["offset"]) % 16


# ---------------------------------------------------------------- the walk's acceptance rules, restated
# What the filters of pf_ba.hip decide for one walk job (stream, value count), from their stated
# rules and in plain numpy: which of the three outcomes a job takes on each route. The GPU tests hold the
# route counters of every file to these. (The values never depend on the outcome: only the route does.)
def _links_verify(cand, succ, n, count):
    """k_ba_link x 2, k_ba_count / k_ba_scan, k_ba_verify (and ba_relink_wg, which restates them) over a
    candidate bitmap: True when the accepted set is `count` positions that chain exactly from 0."""
    if n == 0 or count <= 0:
        return False
    c = np.flatnonzero(cand)
    link1 = np.zeros(len(cand), bool)
    s = succ[c]
    s = s[s < n]
    link1[s[cand[s]]] = True
    link1[0] = True
    c1 = np.flatnonzero(cand & link1)
    link2 = np.zeros(len(cand), bool)
    s = succ[c1]
    s = s[s < n]
    link2[s[cand[s]]] = True
    link2[0] = True
    acc = np.flatnonzero(cand & link2)
    if len(acc) != count or acc[0] != 0:
        return False
    return bool(np.all(succ[acc[:-1]] == acc[1:]))


def _padded(stream):
    """fit and succ over every position 0 .. n + BA_TILE (False past n - 4), so windows can overhang."""
    n = len(stream)
    fit, succ = fitting(stream)
    f = np.zeros(n + 2 * BA_TILE, bool)
    s = np.zeros(n + 2 * BA_TILE, np.int64)
    f[:len(fit)] = fit
    s[:len(succ)] = succ
    return f, s


def multi_kernel_outcome(stream, count):
    """k_ba_cand's rule: q is plausible if its length fits and the position after its value is the
    stream end or again a fitting length; a plausible position followed by another is dropped."""
    n = len(stream)
    fit, succ = _padded(stream)
    sv = np.where(fit, succ, 0)
    m = fit & ((sv == n) | ((sv + 4 <= n) & fit[sv]))
    cand = m & ~np.roll(m, -1)
    return "accepted" if _links_verify(cand, succ, n, count) else "walked"


def fused_outcome(stream, count):
    """k_ba_tile per tile (candidates over [t0 - 256, t1 + 128] with a successor past the stage taken as
    plausible unread, links at most BA_HALO far, the local chain check), k_ba_scan's count, then
    ba_relink_wg over the tiles' own candidate words."""
    n = len(stream)
    if count <= 0:
        return "accepted"
    fit, succ = _padded(stream)
    sv_all = np.where(fit, succ, 0)
    cand_job = np.zeros(len(fit), bool)
    total, bad = 0, False
    for t0 in range(0, max(n, 1), BA_TILE):
        if t0 >= n:
            break
        t1, sb = t0 + BA_TILE, t0 - 2 * BA_HALO
        wend = t1 + BA_HALO
        lo = max(sb, 0)
        q = np.arange(lo, wend + 1)
        sv = sv_all[q]
        unread = sv - sb + 4 > BA_TILE + 3 * BA_HALO + 48
        m = fit[q] & ((sv == n) | ((sv + 4 <= n) & (unread | fit[np.minimum(sv, len(fit) - 1)])))
        C = np.zeros(len(fit), bool)
        C[q[:-1]] = m[:-1] & ~m[1:]
        L1 = np.zeros(len(fit), bool)
        for p in np.flatnonzero(C):
            s = succ[p]
            if s - p <= BA_HALO and s >= t0 - BA_HALO and s < wend and s < n:
                L1[s] = True
        if t0 == 0:
            L1[0] = True
        L2 = np.zeros(len(fit), bool)
        for p in np.flatnonzero(C & L1):
            s = succ[p]
            if p >= t0 - BA_HALO and s - p <= BA_HALO and s >= t0 and s < wend and s < n:
                L2[s] = True
        if t0 == 0:
            L2[0] = True
        acc = C & L2
        cand_job[t0:t1] = C[t0:t1]
        own = np.flatnonzero(acc[t0:t1]) + t0
        total += len(own)
        if t0 == 0 and not acc[0]:
            bad = True
        for p in own:
            s = succ[p]
            if s != n and s - p > BA_HALO:
                bad = True
                break
            if acc[p + 1:min(s, wend)].any() or (s < wend and s < n and not acc[s]):
                bad = True
                break
    if not bad and total == count:
        return "accepted"
    return "re-linked" if _links_verify(cand_job, succ, n, count) else "walked"


def expected_counts(cases, route):
    """(re-linked, walked) jobs of a file of these cases on `route` ("fused" / "multi"): one job per
    PLAIN BYTE_ARRAY page, the filler pages (one text value: accepted) included."""
    out = {"accepted": 0, "re-linked": 0, "walked": 0}
    for c in cases:
        out[(fused_outcome if route == "fused" else multi_kernel_outcome)(c.stream, c.count)] += 1
    return out["re-linked"], out["walked"]
