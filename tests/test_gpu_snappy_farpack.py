"""k_snappy_exec5's chunk-packed far-copy sources (pf_snappy_exec.hip: X5_FCH), on hand-assembled
streams (snappy_tokens.Stream). A far copy's source left the 4 KiB ring and is read from HBM: the producer
loads the nch = (fsh + ol + 15) >> 4 aligned 16-byte chunks that cover it (fsh: the source address's low four
bits) into the batch's chunk buffer, at the running sum of nch, and cuts the batch before the copy whose chunks
would pass X5_FCH = 64. The expected bytes are the assembler's own; every stream must come out bit-exact AND
report FB_OK: a whole-page redo or the serial kernel would decode a broken far path correctly and hide it.

How the streams pin a batch. A literal longer than 64 bytes is a batch of its own, and one longer than
XCHUNK = 1024 bytes also ends the input chunk, so the tokens behind a separator literal of SEP bytes open both a
fresh input chunk and a fresh batch: up to 128 tokens / 764 output bytes of them are one batch unless the far
limit under test cuts it. nch depends on the address, which is the output offset plus the arena's base; the
test does not know the base's low bits, so lengths whose nch does not depend on fsh are used where a chunk
count must be exact (1 byte: one chunk; 17 bytes: two), and every scenario is repeated with the sources shifted
by 0..15 bytes (a 64-byte copy takes five chunks at fifteen of the sixteen shifts, four at the other).

The frontier sweep. A source is far only when it starts more than XRING - X5_BATCH = 3332 bytes before its
batch, and in steady state the landed frontier LF trails the batch by at most 764 + 2 * 1024 bytes, so a far
source can be unlanded only behind a long literal: LF is then the 1 KiB slot floor F of that literal's start
(F - 1024 when the batch before the literal was an ordinary one). So a far source never ends within 400 bytes
of its own batch's start (it would be a ring copy); the sweep that reaches the landed-frontier test puts the
sources' ends 0..400 bytes below F and below F - 1024, behind a literal long enough to make them far, lengths
1, 16, 17 and 64. The sweep against the batch's own start is run as well (ring copies)."""
import numpy as np
import pytest

import snappy_tokens as T
from golden_util import assert_chunk_equal
from test_gpu_snappy_pages import (DIRECT_VALUES, FB_OK, FB_REDO, NV_OPT, _compressible, _data_page, _debug, _end,
                                   _levels, _write)

pytestmark = pytest.mark.gpu

X5_FCH = 64           # pf_snappy_exec.hip (today's value: a retune moves the cases with it)
PREFIX = 8192         # random literal bytes in front: the sources
SEP = 1100            # separator literal: > XCHUNK, so the next token opens an input chunk and a batch
FAR = 5000            # far offsets are FAR .. FAR + 15 (> XRING + X5_BATCH)
SWEEP_LENGTHS = (1, 16, 17, 64)


def _far(s, al, ln):
    """A far copy of ln bytes whose source's output offset is al mod 16."""
    off = FAR + (s.opos - FAR - al) % 16
    assert (s.opos - off) % 16 == al % 16 and s.opos - off >= 0
    return s.copy(2, off, ln)


def _stream(seed):
    s = T.Stream(seed)
    s.lit(s.rand(PREFIX))
    return s


def _alignment_grid():
    """Every length 1..64 at every source alignment 0..15, back to back (nch 1..5, lengths that end exactly on
    a chunk edge included); and the same with a one-byte literal between the copies."""
    out = []
    for gap in (0, 1):
        s = _stream(900 + gap)
        for al in range(16):
            for ln in range(1, 65):
                _far(s, al, ln)
                if gap:
                    s.lit(s.rand(1))
        assert s.opos < T.BLOCK
        out.append((f"grid_gap{gap}", s))
    return out


def _group(s, sh, plan):
    """One batch behind a separator: plan = [(count, length)], the sources shifted by sh."""
    s.lit(s.rand(SEP))
    i = 0
    for count, ln in plan:
        for _ in range(count):
            _far(s, sh + i, ln)
            i += 1


# scenario -> [(count, length)]; chunk totals by the lengths' fixed nch (1 byte: 1, 17 bytes: 2). Every scenario is
# at most 128 tokens and 764 bytes up to the copy under test, so nothing but the chunk limit cuts before it.
PLANS = {
    # more than 64 far copies back to back (with X5_FCH > 64: one batch, the second LDS-DMA instruction)
    "over64": [(100, 1)],
    "over64_len4": [(100, 4)],
    # 128 one-byte far copies: 128 tokens, 128 chunks
    "x128_one_byte": [(128, 1)],
    # exactly X5_FCH chunks from two-chunk and one-chunk copies, and more behind them
    "exact_fch": [(15, 17), (X5_FCH - 30, 1), (10, 17)],
    # one chunk under X5_FCH, then a copy that needs two
    "one_under_then_two": [(X5_FCH - 1, 1), (1, 17), (20, 1)],
    # X5_FCH - 4 chunks, then a 64-byte copy (five chunks at 15 shifts of 16) crosses X5_FCH
    "five_chunk_crosses": [(15, 17), (X5_FCH - 34, 1), (1, 64), (5, 17)],
    # X5_FCH - 5 chunks, then the 64-byte copy ends exactly at X5_FCH (or one under)
    "five_chunk_fits": [(15, 17), (X5_FCH - 35, 1), (1, 64), (5, 17)],
}
assert X5_FCH >= 36 and 15 + X5_FCH - 30 + 1 <= 128 and 15 * 17 + X5_FCH - 30 + 64 <= 764


def _scenarios():
    out = []
    for k, (name, plan) in enumerate(PLANS.items()):
        s = _stream(910 + k)
        for sh in range(16):
            _group(s, sh, plan)
        s.lit(s.rand(SEP))
        assert s.opos < T.BLOCK, name
        out.append((name, s))
    return out


def _sweep_tokens(s, ref, ds):
    """Copies of every sweep length whose source ends d bytes below output offset ref."""
    for d in ds:
        for ln in SWEEP_LENGTHS:
            a = ref - d - ln
            assert a >= 0
            s.copy(2, s.opos - a, ln)


def _frontier_sweeps():
    """Sources ending 0..400 bytes below the landed frontier behind a long literal (see the module docstring):
    `ordinary`: the batch before the literal is an ordinary one, LF = F - 1024; `long`: a 100-byte literal (a
    long one) stands before it, LF = F. 7 distances x 4 lengths = 28 tokens, 686 bytes: one batch."""
    out = []
    ds = list(range(401))
    groups = [ds[i:i + 7] for i in range(0, len(ds), 7)]
    for mode in ("ordinary", "long"):
        for part in range(0, len(groups), 13):
            s = _stream(930 + part + (500 if mode == "long" else 0))
            for g in groups[part:part + 13]:
                s.copy(2, 100, 30)                      # an ordinary batch
                if mode == "long":
                    s.lit(s.rand(100))
                F = s.opos & ~1023
                # long enough that a source ending at the frontier (<= the literal's start) is far: it starts more
                # than 3332 bytes before the batch
                s.lit(s.rand(3400))
                _sweep_tokens(s, F - 1024 if mode == "ordinary" else F, g)
            assert s.opos < T.BLOCK, (mode, part)
            out.append((f"frontier_{mode}_{part}", s))
    return out


def _batch_start_sweep():
    """Sources ending 0..400 bytes before their own batch's start (ring copies, see the module docstring), the
    d = 0 one first in its batch: its last byte is the last byte before the batch."""
    out = []
    ds = list(range(401))
    groups = [ds[i:i + 7] for i in range(0, len(ds), 7)]
    for part in range(0, len(groups), 30):
        s = _stream(960 + part)
        for g in groups[part:part + 30]:
            s.lit(s.rand(SEP))
            _sweep_tokens(s, s.opos, g)
        assert s.opos < T.BLOCK
        out.append((f"batch_start_{part}", s))
    return out


def _edges():
    out = []
    # a source at output byte 0 (the loads start at the arena's first chunk)
    s = T.Stream(980)
    s.lit(s.rand(5000))
    for ln in SWEEP_LENGTHS:
        s.copy(2, s.opos, ln).lit(s.rand(2))
    s.copy(2, s.opos - 1, 64)
    out.append(("source_byte0", s))
    # a source whose last byte is the last byte before the batch, first token of the batch
    s = _stream(981)
    for ln in SWEEP_LENGTHS:
        s.lit(s.rand(SEP)).copy(2, ln, ln)
        _far(s, 3, 20)
    out.append(("source_ends_at_batch", s))
    return out


CASES = {
    "alignment_grid": _alignment_grid,
    "scenarios": _scenarios,
    "frontier": _frontier_sweeps,
    "batch_start": _batch_start_sweep,
    "edges": _edges,
}


@pytest.fixture(scope="module")
def dec():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


@pytest.mark.parametrize("group", list(CASES))
def test_far_chunk_packing(dec, group):
    wrong = []
    for name, s in CASES[group]():
        stream, exp = s.finish()
        assert exp is not None and len(exp) >= 5000
        got, code = dec.snappy_decompress(stream, cap=len(exp))
        if got != exp:
            at = next((i for i, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp))) if isinstance(got, bytes) else got
            wrong.append(f"{name}: output differs (first at byte {at} of {len(exp)}; status / code {code})")
        elif code != T.FB_OK:
            wrong.append(f"{name}: pf_snappy_last_fallback {code}, expected FB_OK")
    assert not wrong, "\n".join(wrong)


def _direct_mix(s, head, total):
    """A page body for the direct split (values from od.dlo = len(head) on go straight into the column, the
    level bytes into the scratch body): far sources in the level section (a + ol <= dlo), from the first value
    byte on, the alignment grid, and batches at the chunk limit -- the column arena's alignment differs from
    the scratch body's by dlo."""
    dlo = len(head)
    s.lit(head + s.rand(PREFIX))
    for rep in range(3):
        s.lit(s.rand(SEP))
        for a in range(dlo):                       # below dlo: whole sources inside the level section
            for ln in range(1, dlo - a + 1):
                s.copy(2, s.opos - a, ln)
        for a in range(dlo, dlo + 16):             # at and just past dlo
            for ln in (1, 8, 17, 64):
                s.copy(2, s.opos - a, ln)
    for al in range(16):
        for ln in range(1, 65, 3):
            _far(s, al, ln)
    for sh in range(0, 16, 3):
        for name in ("over64", "exact_fch", "one_under_then_two", "five_chunk_crosses"):
            _group(s, sh, PLANS[name])
    assert s.opos < T.BLOCK - 400
    _end(s, total)


def test_direct_split_page(dec, oracle, tmp_path):
    """The same mix through a DIRECT_VALUES page (built as test_gpu_snappy_pages.py builds its pages), far
    sources on both sides of od.dlo: FB_OK; that file's straddling page beside it stays FB_REDO."""
    from pfloor.decoder import decode_file
    nv = NV_OPT
    head = _levels(nv)
    total = len(head) + 8 * nv
    table = [("farpack_mix", _direct_mix, FB_OK), ("far_copy_straddles_dlo", _compressible(straddle=True), FB_REDO)]
    body, values, unc = bytearray(), [], 0
    for i, (name, build, _fb) in enumerate(table):
        s = T.Stream(990 + i)
        build(s, head, total)
        stream, exp = s.finish()
        assert len(exp) == total and exp[:len(head)] == head, name
        values.append(np.frombuffer(exp[len(head):], dtype=np.int64))
        page = _data_page(stream, total, nv, statistics=True)
        body += page
        unc += len(page) - len(stream) + total
    path = str(tmp_path / "farpack_direct.parquet")
    _write(path, 2, True, body, nv * len(table), len(table), unc=unc)
    got = decode_file(path, decoder=dec)
    assert got["_status"] == 0, got["_error"]
    gv = np.frombuffer(got[(0, 0)]["values"].tobytes(), np.int64)
    jobs, direct = _debug(dec)
    for p, (name, _b, fb) in enumerate(table):
        ne = np.flatnonzero(gv[p * nv:(p + 1) * nv] != values[p])
        assert not len(ne), f"{name}: {len(ne)} values differ, first {ne[0]} (fallback {jobs[p][0]}, direct {direct[p]})"
    assert np.unpackbits(got[(0, 0)]["validity"], bitorder="little")[:nv * len(table)].all()
    with oracle.open(path) as of:
        ref = of.decode(0, 0)
        assert ref["status"] == 0, ref["error"]
        assert_chunk_equal(got[(0, 0)], ref, "far chunk packing, direct page")
    assert [(jobs[p][0], direct[p]) for p in range(len(table))] == [(fb, DIRECT_VALUES) for _n, _b, fb in table]
