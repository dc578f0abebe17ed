"""k_flat_fixed's eight-a-thread body (flat_fixed8, pf_flat.hip; the id unpack is csrc/pf_fix_ids.h): fixed-width
dictionary pages whose levels are all present, eight consecutive entries a thread from one run lookup and one load.

Every case is a file of chunks assembled by tests/pagekit.py. It is decoded three times: by the product library, by the
diagnostics build with its defaults, and by the diagnostics build with PF_FIX8=0 (flat_present_fixed decodes every
block, as before this body). Each chunk must equal the CPU oracle's bit for bit every time. pf_debug_fix8_counts gives
{blocks the body decoded, groups of 8 it decoded entry by entry, blocks of dictionary pages k_flat_fixed gave to
flat_present_fixed}, and the counters must say what the case was built for:
  blocks   by the body's rule (4- or 8-byte values, a dictionary aligned to them, a run table of at most RUN_CAP runs that
           covers the page, ids of at most 16 bits) every page is either the body's, block by block, or the old body's.
           A Snappy chunk's dictionary is decompressed to an aligned address. An uncompressed chunk's lies where the
           file has it: a chunk's bytes start on a 256-byte boundary of the input buffer, so it is aligned exactly when
           the dictionary page's header is a multiple of the value width long. Dictionaries of 64 to 1023 values have a
           16-byte header; the uncompressed cases use those, and the plan knows the others for the old body's;
  groups   a group is decoded entry by entry when its entries lie in more than one run or it is the page's last,
           partial group in a packed run. The test parses the case's own id streams and counts those. Beside them only
           the packed groups at the two ends of a page's id section can be slow (their words would reach outside it:
           at most 2 + 20 // width a page), so the count must lie between the two.
A page with an id outside the dictionary must give the status and the error of the PF_FIX8=0 run."""
import ctypes as C
import os

import numpy as np
import pytest

import pagekit as K
from golden_util import assert_chunk_equal

pytestmark = pytest.mark.gpu

RUN_CAP = 256
COUNTS = (1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 2 * 8192 + 1)
PTYPES = {"int32": K.INT32, "float": K.FLOAT, "int64": K.INT64, "double": K.DOUBLE}
V1S = K.Layout("v1s", False, K.SNAPPY)


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _fix8_counts():
    """(blocks of the new body, slow groups, blocks of the old body) since the last call; diagnostics build only."""
    from pfloor import _native
    f = _native.lib().pf_debug_fix8_counts
    f.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    buf = (C.c_ulonglong * 3)()
    assert f(buf, 1) == 0
    return int(buf[0]), int(buf[1]), int(buf[2])


def _bw(n):
    return max(n - 1, 0).bit_length()


def _dict(ptype, n, seed):
    """n distinct dictionary values as rows of bytes."""
    w = K.width_of(ptype)
    rng = np.random.default_rng(seed)
    v = np.zeros((n, w), np.uint8)
    v[:, :4] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)     # distinct
    v[:, w - 2:] ^= rng.integers(0, 256, (n, 2), dtype=np.uint8)
    return v


# ---------------------------------------------------------------- what a stream asks of the body
def _runs(stream, bw, n):
    """[(first, count, packed)] of a hybrid stream up to n values (as k_runs walks it)."""
    out, pos, first, nb = [], 0, 0, (bw + 7) // 8
    while first < n and pos < len(stream):
        h, sh = 0, 0
        while True:
            b = stream[pos]
            pos += 1
            h |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                break
        if h & 1:
            c = (h >> 1) * 8
            pos += (h >> 1) * bw
        else:
            c = h >> 1
            pos += nb
        if c:
            out.append((first, min(c, n - first), bool(h & 1)))
            first += c
    return out


def _designed_slow(stream, bw, n):
    """Groups of 8 (from entry 0) that lie in more than one run, or are partial in a packed run of width > 0."""
    runs = _runs(stream, bw, n)
    run_of = np.zeros(n, np.int64)
    packed = np.zeros(len(runs), bool)
    for i, (f, c, p) in enumerate(runs):
        run_of[f:f + c] = i
        packed[i] = p
    slow = 0
    for e0 in range(0, n, 8):
        m = min(8, n - e0)
        if run_of[e0] != run_of[e0 + m - 1] or (m < 8 and packed[run_of[e0]] and bw > 0):
            slow += 1
    return slow, len(runs)


class Case:
    def __init__(self, name, build, bad=False, env=None):
        self.name, self.build, self.bad, self.env = name, build, bad, env or {}


class Plan:
    """What the counters must show for one built file (filled by add_page below)."""

    def __init__(self, bsz=8192):
        self.bsz, self.new, self.old, self.slow_lo, self.slow_hi = bsz, 0, 0, 0, 0


def add_page(plan, ch, dvals, ids, bw, style="mr", rng=None, stream=None, present=None, encoding=K.RLE_DICTIONARY):
    """One dictionary data page of ch (ids index dvals) and what it adds to the plan."""
    ids = np.asarray(ids, np.uint64)
    if stream is None:
        stream = K.hybrid(ids, bw, style, rng)
    n = len(ids)
    vals = dvals[np.minimum(ids, len(dvals) - 1).astype(np.int64)]
    ch.add_page(encoding, bytes([bw]) + stream, present=present, vals=vals)
    blocks = max(1, (n + plan.bsz - 1) // plan.bsz)
    slow, nruns = _designed_slow(stream, bw, n)
    # the dictionary's address: decompressed to aligned scratch, or the header's length into the chunk's aligned bytes
    aligned = ch.layout.codec == K.SNAPPY or (len(ch.dict) - dvals.size) % ch.width == 0
    if nruns > RUN_CAP or bw > 16 or not aligned:
        plan.old += blocks
    else:
        plan.new += blocks
        plan.slow_lo += slow
        plan.slow_hi += slow + 2 + 20 // max(bw, 1)


def _alternating(n, dn, bw, rle_len, rng):
    """RLE runs of rle_len values and one-group bit-packed runs in turn: (ids, stream). Odd RLE runs leave the packed runs
    off the 8-entry grid, so nearly every group straddles."""
    ids, out, nb = [], bytearray(), (bw + 7) // 8
    while len(ids) < n:
        v, c = int(rng.integers(dn)), min(rle_len, n - len(ids))
        out += K._uvarint(c << 1) + v.to_bytes(nb, "little")
        ids += [v] * c
        if len(ids) < n:
            g = rng.integers(0, dn, 8)
            out += b"\x03" + K._pack_le(g, bw)
            ids += [int(x) for x in g[:min(8, n - len(ids))]]
    return np.asarray(ids, np.uint64), bytes(out)


def _no_repeats(ids, dn):
    """No run of 8 equal ids by chance, so parquet-mr style streams are bit-packed throughout."""
    return (ids + np.arange(len(ids), dtype=np.uint64) % 2 * (dn // 2)) % dn if dn > 1 else ids


def _counts_case(pname, dsizes, layout=V1S, optional=False, counts=COUNTS):
    ptype = PTYPES[pname]

    def build(compress, plan):
        rng = np.random.default_rng(len(pname) + sum(dsizes))
        chunks = []
        for dn in dsizes:
            dvals = _dict(ptype, dn, dn)
            for n in counts:
                ch = K.Chunk(f"{pname}_{dn}_{n}", ptype, optional=optional, layout=layout, compress=compress)
                ch.set_dictionary(dvals)
                add_page(plan, ch, dvals, rng.integers(0, dn, n), _bw(dn), rng=rng,
                         present=np.ones(n, bool) if optional else None)
                chunks.append(ch)
        return chunks
    return build


def _cases():
    out = []
    # entry counts at group, tile and block edges; dictionaries of 1 (width 0), 2, 7 and 50 values
    for pname in PTYPES:
        out.append(Case(f"counts-{pname}", _counts_case(pname, (1, 2, 7, 50))))
    # a dictionary that fits LDS with no room for a block's ids behind it, and one that does not fit (global gather)
    out.append(Case("counts-int32-dict2526", _counts_case("int32", (2526,))))
    out.append(Case("counts-int64-dict10000", _counts_case("int64", (10000,))))
    # uncompressed chunks: the dictionary and the id sections lie where the file has them (v1 and v2 pages)
    out.append(Case("counts-uncompressed-int32-v1", _counts_case("int32", (100,), layout=K.LAYOUTS["a"])))
    out.append(Case("counts-uncompressed-int64-v2", _counts_case("int64", (1000,), layout=K.LAYOUTS["e"])))
    out.append(Case("counts-uncompressed-unaligned", _counts_case("int32", (50,), layout=K.LAYOUTS["a"], counts=(9, 8193))))
    # an OPTIONAL column whose v2 page headers say no value is null
    # (from 8 entries on the assembler writes the levels as one RLE run, which is what "all present" reads)
    out.append(Case("optional-all-present-v2", _counts_case("int64", (7,), layout=K.LAYOUTS["c"], optional=True,
                                                            counts=[n for n in COUNTS if n >= 8])))

    def widths(ws, ptype):
        def build(compress, plan):
            chunks = []
            for bw in ws:
                rng = np.random.default_rng(100 + bw)
                dn = min(1 << bw, 1 << 17)   # (every bit of an id up to 17 bits wide is used)
                dvals = _dict(ptype, dn, bw)
                ch = K.Chunk(f"w{bw}", ptype, layout=V1S, compress=compress)
                ch.set_dictionary(dvals)
                add_page(plan, ch, dvals, _no_repeats(rng.integers(0, dn, 8193).astype(np.uint64), dn), bw, rng=rng)
                chunks.append(ch)
            return chunks
        return build
    out.append(Case("widths-1-16-int32", widths(range(1, 17), K.INT32)))
    out.append(Case("widths-1-16-double", widths(range(1, 17), K.DOUBLE)))
    out.append(Case("widths-17-24-32", widths((17, 24, 32), K.INT32)))

    # run layouts
    def all_rle(compress, plan):
        rng = np.random.default_rng(5)
        chunks = []
        for pname in ("int32", "int64"):
            dvals = _dict(PTYPES[pname], 50, 3)
            ids = np.repeat(rng.integers(0, 50, 300), rng.integers(40, 80, 300))[:8193].astype(np.uint64)   # <= 205 runs
            ch = K.Chunk(f"rle_{pname}", PTYPES[pname], layout=V1S, compress=compress)
            ch.set_dictionary(dvals)
            add_page(plan, ch, dvals, ids, 6, style="rle")
            chunks.append(ch)
        return chunks
    out.append(Case("all-rle", all_rle))

    def alternating(compress, plan):
        rng = np.random.default_rng(6)
        chunks = []
        for pname, dn, rle_len, n in (("int32", 7, 1, 1100), ("int64", 50, 3, 1400), ("float", 50, 8, 2000),
                                      ("double", 2526, 13, 2600), ("int32", 1, 3, 1400)):
            dvals = _dict(PTYPES[pname], dn, dn)
            bw = _bw(dn)
            ids, stream = _alternating(n, dn, bw, rle_len, rng)
            ch = K.Chunk(f"alt_{pname}_{rle_len}", PTYPES[pname], layout=V1S, compress=compress)
            ch.set_dictionary(dvals)
            add_page(plan, ch, dvals, ids, bw, stream=stream)
            chunks.append(ch)
        return chunks
    out.append(Case("alternating-rle-packed", alternating))

    def too_many_runs(compress, plan):
        rng = np.random.default_rng(8)
        dvals = _dict(K.INT32, 7, 1)
        ch = K.Chunk("mixed", K.INT32, layout=V1S, compress=compress)
        ch.set_dictionary(dvals)
        add_page(plan, ch, dvals, rng.integers(0, 7, 4097), 3, style="mixed", rng=rng)   # > 1000 runs
        return [ch]
    out.append(Case("more-runs-than-the-table", too_many_runs))

    # pages after a page of odd length: slot_base odd, for both widths, v1 / v2, Snappy / uncompressed
    def pages(compress, plan):
        rng = np.random.default_rng(9)
        chunks = []
        for lname, lay in (("a", K.LAYOUTS["a"]), ("c", K.LAYOUTS["c"]), ("e", K.LAYOUTS["e"]), ("v1s", V1S)):
            for pname in ("int32", "int64"):
                dvals = _dict(PTYPES[pname], 100, 4)   # (a 16-byte dictionary page header: aligned when uncompressed too)
                ch = K.Chunk(f"pages_{lname}_{pname}", PTYPES[pname], layout=lay, compress=compress)
                ch.set_dictionary(dvals)
                for n in (5001, 17, 4098, 1, 9003):
                    add_page(plan, ch, dvals, _no_repeats(rng.integers(0, 100, n).astype(np.uint64), 100), 7, rng=rng)
                chunks.append(ch)
        return chunks
    out.append(Case("several-pages-odd-offsets", pages))

    # the last bit-packed run cut short (parquet-mr reads the missing bits as zero), in a full and in a partial group
    def truncated(compress, plan):
        rng = np.random.default_rng(12)
        chunks = []
        for n, pname in ((8200, "int32"), (8197, "int64")):
            dvals = _dict(PTYPES[pname], 30, 5)
            ids = _no_repeats(rng.integers(0, 30, n).astype(np.uint64), 30)
            ids[8192:] = 0
            ids[8192:8194] = (3, 1)
            stream = K.hybrid(ids, 5, "mr", rng)
            ch = K.Chunk(f"trunc_{n}", PTYPES[pname], layout=V1S, compress=compress)
            ch.set_dictionary(dvals)
            add_page(plan, ch, dvals, ids, 5, stream=stream[:-3])   # the group's last three bytes are zero: dropped
            chunks.append(ch)
        return chunks
    out.append(Case("truncated-last-run", truncated))

    # errors: an id equal to dict_n in the first group, the last group and a group that straddles two runs
    for where in ("first", "last", "straddling"):
        def bad(compress, plan, where=where):
            rng = np.random.default_rng(10)
            dvals = _dict(K.INT64, 7, 2)
            n = 2 * 8192 + 1
            if where == "straddling":
                ids, _ = _alternating(1400, 7, 3, 3, rng)
                pos = 9     # entries 8..15: the end of a packed run, an RLE run, the start of the next packed run
            else:
                ids = _no_repeats(rng.integers(0, 7, n).astype(np.uint64), 7)
                pos = 3 if where == "first" else n - 1
            good = K.Chunk("good", K.INT64, layout=V1S, compress=compress)
            good.set_dictionary(dvals)
            ch = K.Chunk("bad", K.INT64, layout=V1S, compress=compress)
            ch.set_dictionary(dvals)
            for c, v in ((good, ids.copy()), (ch, ids.copy())):
                if c is ch:
                    v[pos] = 7
                if where == "straddling":   # the same runs, the id changed inside its packed group
                    stream, e, b = bytearray(), 0, 0
                    while e < len(v):
                        k = min(3, len(v) - e)
                        stream += K._uvarint(k << 1) + int(v[e]).to_bytes(1, "little")
                        e += k
                        if e < len(v):
                            g = np.zeros(8, np.uint64)
                            m = min(8, len(v) - e)
                            g[:m] = v[e:e + m]
                            stream += b"\x03" + K._pack_le(g, 3)
                            e += m
                    add_page(plan, c, dvals, v, 3, stream=bytes(stream))
                else:
                    add_page(plan, c, dvals, v, 3, rng=rng)
            return [good, ch]
        out.append(Case(f"bad-id-{where}-group", bad, bad=True))

    # block widths
    for blk in (4096, 8192, 16384):
        def blocks(compress, plan):
            rng = np.random.default_rng(13)
            chunks = []
            for pname, dn in (("int32", 2526), ("int64", 50)):
                dvals = _dict(PTYPES[pname], dn, 6)
                ch = K.Chunk(f"blk_{pname}", PTYPES[pname], layout=V1S, compress=compress)
                ch.set_dictionary(dvals)
                add_page(plan, ch, dvals, rng.integers(0, dn, 2 * 8192 + 1), _bw(dn), rng=rng)
                chunks.append(ch)
            return chunks
        out.append(Case(f"block-width-{blk}", blocks, env={"PF_FIX_BLK": blk}))
    return out


CASES = {c.name: c for c in _cases()}


def _compare(got, exp, case, tag):
    for c, e in enumerate(exp):
        g = got[(0, c)]
        where = f"{case.name} [{tag}] chunk {c}"
        if e["status"] != 0:
            assert case.bad and g["status"] != 0, f"{where}: the oracle rejects it ({e['error']}), the GPU reports {g['status']}"
            continue
        assert g["status"] == 0, f"{where}: status {g['status']} ({got['_error']})"
        assert_chunk_equal(g, e, where)
    if not case.bad:
        assert got["_status"] == 0, (case.name, tag, got["_error"])


@pytest.mark.parametrize("name", list(CASES))
def test_fix8_case(name, oracle, decoder, switches, tmp_path):
    from pfloor.decoder import GpuDecoder, decode_file
    case = CASES[name]
    plan = Plan(int(case.env.get("PF_FIX_BLK", 8192)))
    chunks = case.build(oracle.snappy_compress, plan)
    data, _info = K.build_file(chunks, max(ch.num_entries for ch in chunks))
    path = os.path.join(str(tmp_path), "fix8.parquet")
    with open(path, "wb") as fh:
        fh.write(data)
    with oracle.open(data=data) as of:
        exp = [of.decode(0, c) for c in range(len(chunks))]
    if not case.bad:   # the assembler's own expectation agrees with the oracle
        for c, ch in enumerate(chunks):
            assert_chunk_equal(exp[c], ch.expected(), f"{name}: oracle against the construction, chunk {c}")
    _compare(decode_file(path, decoder=decoder), exp, case, "product library")
    seen = {}
    for env, tag in ((dict(case.env), "diagnostics build"), (dict(case.env, PF_FIX8=0), "diagnostics build PF_FIX8=0")):
        with switches(**env), GpuDecoder(0) as d:
            _fix8_counts()
            got = decode_file(path, decoder=d)
            new, slow, old = _fix8_counts()
        print(f"{name} [{tag}]: blocks of the new body {new} (plan {plan.new}), slow groups {slow} (plan {plan.slow_lo} to "
              f"{plan.slow_hi}), blocks of the old body {old} (plan {plan.old})")
        _compare(got, exp, case, tag)
        seen[tag] = ([got[(0, c)]["status"] for c in range(len(chunks))], got["_status"], got["_error"])
        if case.bad:     # a failed chunk's later blocks are not decoded at all: the body that met the id
            if "PF_FIX8" in env:
                assert new == 0 and old >= 1, f"{name} [{tag}]: blocks new, old {(new, old)}"
            else:
                assert new >= 1 and old == 0, f"{name} [{tag}]: blocks new, old {(new, old)}"
            continue
        if "PF_FIX8" in env:
            assert (new, slow) == (0, 0), f"{name} [{tag}]: the new body ran ({new}, {slow})"
            total = plan.new + plan.old
            assert old == total, f"{name} [{tag}]: blocks of the old body {old}, by the rule {total}"
        else:
            assert (new, old) == (plan.new, plan.old), f"{name} [{tag}]: blocks new, old {(new, old)}, by the rule " \
                                                        f"{(plan.new, plan.old)}"
            assert plan.slow_lo <= slow <= plan.slow_hi, f"{name} [{tag}]: slow groups {slow}, by the rule " \
                                                         f"{plan.slow_lo} to {plan.slow_hi}"
    if case.bad:   # status and error as with the old body
        assert seen["diagnostics build"] == seen["diagnostics build PF_FIX8=0"], seen
