"""tools/exec_cuts.py's batch model (the producer cuts of k_snappy_exec5) on three hand-made
token lists whose cuts are known by construction: the far limit of the fixed slots, the chunk limit of the
packed layout, and 128 tokens."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import exec_cuts as X  # noqa: E402


def _tokens(spec, pos=3):
    """[(kind, ol, off)] -> exec_cuts tokens (in_pos, kind, ol, off, tl): literals with their minimal header,
    copies as 3-byte copy-2 tokens, back to back from input position pos."""
    out = []
    for kind, ol, off in spec:
        tl = 3 if kind else ol + (1 if ol <= 60 else 2 if ol <= 256 else 3)
        out.append((pos, kind, ol, off, tl))
        pos += tl
    return out


def _shape(recs):
    return [(kind, reason, nt) for kind, reason, nt, _nb, _nf, _nc in recs]


# A 6000-byte literal is a batch of its own. The far copy behind it waits one empty batch: the frontier is the
# slot floor of the previous batch's start, 0 behind the literal; behind the empty batch (which starts at 6000)
# it is 5120, above every source here.
HEAD = [("long", "long", 1), ("nop", "frontier", 0)]


def test_far_limit():
    """60 far copies of 4 bytes from 16-byte aligned sources: 24 a batch in the fixed slots, one batch packed."""
    spec, o = [(0, 6000, 0)], 6000
    for i in range(60):
        spec.append((1, 4, o - 16 * i))
        o += 4
    toks = _tokens(spec)
    assert _shape(X.batches(toks, 0, o, False)) == HEAD + [("normal", "far", 24), ("normal", "far", 24), ("normal", "end", 12)]
    packed = X.batches(toks, 0, o, True)
    assert _shape(packed) == HEAD + [("normal", "end", 60)]
    assert packed[-1][4:] == (60, 60)          # 60 far copies, one chunk each


def test_chunk_limit():
    """2-byte far copies whose source starts at the last byte of a chunk take two chunks each: 32 of them fill
    X5_FCH = 64 chunks with 64 bytes and 32 tokens, so nothing but the chunk limit cuts. The fixed slots cut
    the same tokens at 24."""
    spec, o = [(0, 6000, 0)], 6000
    for i in range(100):
        spec.append((1, 2, o - (15 + 16 * i)))
        o += 2
    toks = _tokens(spec)
    assert X.X5_FCH == 64
    packed = X.batches(toks, 0, o, True)
    assert _shape(packed) == HEAD + [("normal", "chunks", 32)] * 3 + [("normal", "end", 4)]
    assert packed[2][4:] == (32, 64) and packed[-1][4:] == (4, 8)
    assert _shape(X.batches(toks, 0, o, True, fch=128)) == HEAD + [("normal", "chunks", 64), ("normal", "end", 36)]
    assert _shape(X.batches(toks, 0, o, True, fch=96)) == HEAD + [("normal", "chunks", 48), ("normal", "chunks", 48), ("normal", "end", 4)]
    assert _shape(X.batches(toks, 0, o, False)) == HEAD + [("normal", "far", 24)] * 4 + [("normal", "end", 4)]
    # a 64-byte source at byte 1 of a chunk takes five chunks, at byte 0 four; 17 bytes take two anywhere
    assert [X.nchunks(a, 64) for a in (0, 1, 15, 16)] == [4, 5, 5, 4]
    assert {X.nchunks(a, 17) for a in range(16)} == {2} and {X.nchunks(a, 1) for a in range(16)} == {1}


def test_token_limit():
    """One-byte ring copies: 128 tokens a batch in both layouts (300 tokens: 128, 128, 44)."""
    spec = [(0, 10, 0)] + [(1, 1, 1)] * 299
    toks = _tokens(spec)
    want = [("normal", "tokens", 128), ("normal", "tokens", 128), ("normal", "end", 44)]
    assert _shape(X.batches(toks, 0, 309, False)) == want
    assert _shape(X.batches(toks, 0, 309, True)) == want
