"""The argument k_snappy_index's successor record rests on (pf_snappy_parse.hip: succ_walk), on the CPU.

The chain pass wants, for a window starting at W and an entry e into it, the first position m of chain(e) that
lies on chain(W) (the window's own chain) and the difference of the two chains' output sums up to m. The index
pass used to read m off the window's token-start bitmap; it now finds it without the bitmap, with two pointers
p = e and q = W of which the one behind steps one token at a time until they are equal. This file checks, in
pure Python on snappy_tokens streams, that the two definitions agree for every entry in a window's first 200
bytes (true token starts or not: a chain may start at any byte), and that the kernel's limits (IDX_EXT staged
bytes past the window start, IDX_STEPS tokens) only ever turn an answer into "not resolved", never into another
answer."""
import numpy as np
import pytest

import snappy_tokens as T

WIN = 8192          # SNAP_WIN
IDX_EXT = 512       # pf_snappy_parse.hip (today's values)
IDX_STEPS = 384


def tok(b, p):
    """(input bytes, output bytes) of the token whose tag is b[p]; bytes past the end read as zero. A 4-byte
    literal length breaks the chain (None), as in the kernels."""
    tag = b[p]
    kind, hi = tag & 3, tag >> 2
    if kind == 1:
        return 2, 4 + (hi & 7)
    if kind == 2:
        return 3, hi + 1
    if kind == 3:
        return 5, hi + 1
    if hi < 60:
        return 2 + hi, hi + 1
    nb = hi - 59
    if nb == 4:
        return None
    ln = int.from_bytes((b[p + 1:p + 1 + nb] + bytes(4))[:nb], "little") + 1
    return 1 + nb + ln, ln


def chain(b, start):
    """{position: output bytes of the chain from `start` before it} for every token start the chain from `start`
    reaches (positions < len(b); the chain stops where a token would run past the end)."""
    n, p, acc, out = len(b), start, 0, {}
    while p < n:
        out[p] = acc
        t = tok(b, p)
        if t is None or p + t[0] > n:
            break
        acc += t[1]
        p += t[0]
    return out


def by_definition(b, e, W, own=None):
    """(m, output difference) from the two chains, or None if chain(e) never meets chain(W) (own: chain(b, W),
    when the caller has it)."""
    own = chain(b, W) if own is None else own
    for p, acc in chain(b, e).items():        # (in chain order)
        if p in own:
            return p, (acc - own[p]) & 0xFFFFFFFF
    return None


def two_pointer(b, e, W, ext=None, cap=None):
    """The kernel's walk. (m, difference), None when a chain ends before they meet, "slow" when the walk
    would need a byte at or past W + ext or more than `cap` steps."""
    n = len(b)
    lim = n if ext is None else min(W + ext, n)
    p, q, ap, aq, steps = e, W, 0, 0, 0
    while True:
        if p == q:
            return (p, (ap - aq) & 0xFFFFFFFF) if p < n else None
        lo = min(p, q)
        if lo >= lim:
            return "slow" if lim < n else None
        if cap is not None and steps == cap:
            return "slow"
        t = tok(b, lo)
        if t is None or lo + t[0] > n:
            return None
        if p < q:
            p, ap = p + t[0], ap + t[1]
        else:
            q, aq = q + t[0], aq + t[1]
        steps += 1


def _mixed(seed, nbytes):
    s = T.Stream(seed)
    T.mixed_block_tokens(s, nbytes)
    return s.finish()[0]


def _copy1_runs(seed, period):
    """Runs of 2-byte copy-1 tokens whose offset byte is itself a copy-1 tag (chains started one byte apart stay
    one byte apart), broken by a 3-byte token every `period` tokens (0: never): a window and a half of them behind the first."""
    s = T.Stream(seed)
    s.lit(s.rand(300))
    k = 0
    while len(s.body) < 2 * WIN + WIN // 2:
        k += 1
        if period and k % period == 0:
            s.copy(2, 40, 9)
        else:
            s.copy(1, 0x05, 4)       # tag 0x01, offset byte 0x05 = a copy-1 tag
    return s.finish()[0]


def _long_literals(seed):
    """Literals of 100..3000 bytes of random data: an entry inside one starts a chain of garbage tokens."""
    s = T.Stream(seed)
    while len(s.body) < 3 * WIN + 100:
        s.lit(s.rand(int(s.rng.integers(100, 3000))))
        s.copy(2, 50, 20)
    return s.finish()[0]


def _streams():
    out = [(f"mixed_{i}", _mixed(1000 + i, 60000)) for i in range(3)]
    out += [(f"copy1_runs_{p}", _copy1_runs(1010 + p, p)) for p in (0, 3, 25, 200, 300)]
    out += [("long_literals", _long_literals(1020))]
    rng = np.random.default_rng(1030)
    out += [("random_bytes", rng.integers(0, 256, 3 * WIN + 77, dtype=np.uint8).tobytes())]
    out += [("zeros", bytes(2 * WIN + 5)), ("tag_f0", b"\xf0" * (2 * WIN + 9)), ("tag_fc", b"\xfc" * (WIN + 300))]
    return out


STREAMS = _streams()


@pytest.mark.parametrize("name", [n for n, _ in STREAMS])
def test_two_pointer_is_the_first_common_position(name):
    b = dict(STREAMS)[name]
    checked = resolved = 0
    for W in range(WIN, len(b), WIN):
        own = chain(b, W)
        for e in range(W, min(W + 200, len(b))):
            want = by_definition(b, e, W, own)
            got = two_pointer(b, e, W)
            assert got == want, f"{name}: window at {W}, entry {e}: walk {got}, definition {want}"
            lim = two_pointer(b, e, W, IDX_EXT, IDX_STEPS)
            assert lim == "slow" or lim == want, f"{name}: window at {W}, entry {e}: limited walk {lim}, definition {want}"
            checked += 1
            resolved += want is not None
    assert checked >= 200
    if name.startswith("mixed") or name == "copy1_runs_3":
        assert resolved >= 100, f"{name}: only {resolved} of {checked} entries merge: the stream tests little"


def test_entry_on_the_window_start_merges_at_once():
    b = dict(STREAMS)["mixed_0"]
    assert two_pointer(b, WIN, WIN) == (WIN, 0) == by_definition(b, WIN, WIN)


def test_limits_turn_answers_into_slow_only():
    """copy1_runs_200: chains one byte apart merge after up to 200 tokens each, more than IDX_STEPS together (in 400
    bytes, inside the extension); and a merge past W + IDX_EXT (copy1_runs_300 needs up to 600 bytes)."""
    saw = set()
    for name in ("copy1_runs_200", "copy1_runs_300"):
        b = dict(STREAMS)[name]
        for e in range(WIN, WIN + 200):
            free, lim = two_pointer(b, e, WIN), two_pointer(b, e, WIN, IDX_EXT, IDX_STEPS)
            if lim == "slow" and free is not None:
                saw.add(name)
    assert saw == {"copy1_runs_200", "copy1_runs_300"}
