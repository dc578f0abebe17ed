"""k_snappy_index's successor record and k_snappy_chain's use of it (pf_snappy_parse.hip: succ_walk, IDX_EXT,
IDX_STEPS), on hand-assembled streams (snappy_tokens.Stream).

The wave of index window w resolves one entry of window w + 1, its own exit X: two pointers p = X and q = W1 (the
start of window w + 1) step one token at a time, the one behind first, over IDX_EXT staged bytes past W1, until
they meet (ENT_MERGE at m, with the output difference). More than IDX_STEPS steps, or out of staged bytes after
DEEP_STEPS tokens of the chain from X: ENT_SLOW (the chain pass parses the window exactly, whatever its entry turns
out to be); a byte at or past W1 + IDX_EXT or the stream end needed before that, X past the extension, window w
broken: no answer, and the chain pass walks in HBM (deep_walk, DEEP_STEPS tokens) as it does for an entry that a
resolved record was not made for. Whatever path answers, the result is the same chain.

Every stream here is 2 to 4 index windows long (16 to 32 KiB compressed, output about as long, so one 64 KiB block)
unless its case says otherwise; the filler is literals of random bytes and short near copies, so the chains guessed
from window starts run through garbage as they do in real pages. Every stream must come out bit-exact AND report
FB_OK (the serial kernel would decode a wrong chain correctly and hide it), and the chain pass's tables must name
every window's true entry. _walk() is this file's own model of the walk; the sweeps assert on it that they cover
the distances their names promise, so a retune of IDX_EXT, IDX_STEPS or DEEP_STEPS moves the cases with it."""
import ctypes as C

import numpy as np
import pytest

import snappy_tokens as T
from golden_util import assert_chunk_equal
from test_gpu_snappy_pages import DIRECT_VALUES, FB_OK, NV_OPT, _data_page, _debug, _end, _levels, _write

pytestmark = pytest.mark.gpu

WIN = 8192            # SNAP_WIN
IDX_EXT = 512         # pf_snappy_parse.hip (today's values: a retune moves the cases with it)
IDX_STEPS = 384
DEEP_STEPS = 24
WM_SKIP = 17


# ---------------------------------------------------------------- the model

def _tok(b, p):
    """(input bytes, output bytes) of the token at b[p]; None: a 4-byte literal length (the kernels break the chain)."""
    tag = b[p]
    kind, hi = tag & 3, tag >> 2
    if kind:
        return (2, 4 + (hi & 7)) if kind == 1 else ((3, hi + 1) if kind == 2 else (5, hi + 1))
    if hi < 60:
        return 2 + hi, hi + 1
    if hi == 63:
        return None
    ln = int.from_bytes((b[p + 1:p + hi - 58] + bytes(3))[:hi - 59], "little") + 1
    return hi - 58 + ln, ln


def _walk(b, X, W1):
    """The unlimited two-pointer walk: {m: meeting point or None, steps: tokens both pointers took, kp: tokens the
    chain from X took (deep_walk's count), need: bytes past W1 the walk read}."""
    n = len(b)
    p, q, steps, kp, need = X, W1, 0, 0, 0
    while p != q:
        lo = min(p, q)
        t = _tok(b, lo) if lo < n else None
        if t is None or lo + t[0] > n:
            return dict(m=None, steps=steps, kp=kp, need=need)
        need = lo + 4 - W1
        if p < q:
            p, kp = p + t[0], kp + 1
        else:
            q += t[0]
        steps += 1
    wend = min(W1 + WIN, n)
    return dict(m=p if p < wend else None, steps=steps, kp=kp, need=need)


def _entries(stream):
    """[(window, true entry X, W1)] for every window behind the first: X = the first token start at or past W1."""
    _declared, toks = T.parse(stream)
    starts = [t[3] for t in toks] + [len(stream)]
    out = []
    for w in range(1, (len(stream) + WIN - 1) // WIN):
        out.append((w, next(s for s in starts if s >= w * WIN), w * WIN))
    return out


def _answer(b, X, W1):
    """What the index pass records for the entry X of the window at W1, with its limits: 'merge', 'slow' (the
    step cap, or the extension's end after DEEP_STEPS tokens from X) or 'none' (a byte past the extension or the
    stream end needed, or nothing to ask)."""
    n = len(b)
    wend, lim = min(W1 + WIN, n), min(W1 + IDX_EXT, n)
    if X >= wend or X - W1 >= IDX_EXT:
        return "none"
    p, q, steps, kp = X, W1, 0, 0
    while True:
        if p == q:
            return "merge" if p < wend else "none"
        lo = min(p, q)
        if lo >= lim:
            return "slow" if kp >= DEEP_STEPS else "none"
        if steps == IDX_STEPS:
            return "slow"
        t = _tok(b, lo)
        if t is None or lo + t[0] > n:
            return "none"
        if p < q:
            p, kp = p + t[0], kp + 1
        else:
            q += t[0]
        steps += 1


# ---------------------------------------------------------------- stream building

def _filler(s, until):
    """Literals of random bytes and short near copies (input about as long as output) up to input position
    <= until - 70."""
    rng = s.rng
    while s.ipos < until - 160:
        r = rng.random()
        if r < 0.6 or s.opos < 64:
            s.lit(s.rand(int(rng.integers(1, 90))))
        elif r < 0.8:
            s.copy(1, int(rng.integers(1, min(s.opos, 2047) + 1)), int(rng.integers(4, 12)))
        else:
            s.copy(2, int(rng.integers(1, min(s.opos, 60000) + 1)), int(rng.integers(1, 9)))
    return s


def _lit_to(s, end, tail=b""):
    """One literal that ends exactly at input position `end` (its last bytes: tail)."""
    gap = end - s.ipos
    for h, top in ((1, 60), (2, 256), (3, 65536)):
        ln = gap - h
        if max(1, len(tail)) <= ln <= top:
            return s.lit(s.rand(ln - len(tail)) + tail, nb=h - 1)
    raise AssertionError(f"no literal of {gap} bytes")


def _build(fn, seed):
    s = T.build(fn, seed=seed)
    stream, exp = s.finish()
    assert exp is not None
    return stream, exp


def _overshoot(d, windows=3, seed=0, tail=b""):
    """The last token of window 0 (a literal) ends d bytes into window 1 (its last bytes: tail)."""
    def fn(s):
        _filler(s, WIN - 100 if d < 3000 else WIN - 3000)
        _lit_to(s, WIN + d, tail)
        _filler(s, max(windows * WIN - 300, s.ipos + 200))
        s.lit(s.rand(7))
    return _build(fn, 2000 + d + 17 * seed)


# Chains that stay apart. Copy-1 form: the true chain is 2-byte copy-1 tokens 01 05 (offset 5, length 4) whose
# offset byte 05 is a copy-1 tag too, so a chain one byte off reads 05 01 05 01 ... and stays one byte off; the
# 3-byte copy-2 22 05 01 (offset 261) ends it: the chain one byte off reads 05 01 there and lands on the next
# token. Literal form, 32 bytes a token: literals of 31 bytes whose last byte is 78, the tag of such a literal,
# so the chain that starts on that byte stays 31 bytes off; a last byte 7c (a 33-byte token) ends it.

def _apart_copy1(n, extra=False, through=None, windows=3, seed=0, trail=True):
    """Window 0's last literal ends 1 byte into window 1 (3 with `extra`: one more token on the window's own
    chain) on the byte 05; then n copy-1 tokens and the copy-2. through = an input position: no copy-2, the run
    goes on to there (the chains never meet before it), and with trail=False the stream ends there."""
    d = 3 if extra else 1

    def fn(s):
        _filler(s, WIN - 100)
        _lit_to(s, WIN + d, tail=b"\x05\x00\x05" if extra else b"\x05")
        if through is None:
            for _ in range(n):
                s.copy(1, 5, 4)
            s.copy(2, 261, 9)
            assert s.body[-3:] == b"\x22\x05\x01"
        else:
            while s.ipos + 2 <= through:
                s.copy(1, 5, 4)
        if trail:
            _filler(s, max(windows * WIN - 300, s.ipos + 200))
            s.lit(s.rand(7))
    return _build(fn, 2100 + n + 1000 * extra + 17 * seed)


def _apart_copy2(n, seed=0):
    """3-byte tokens: copy-2 tokens 22 06 01 (offset 262); a chain that reads 06, a copy-2 tag too, as its tag goes
    from each token's second byte to the next one's. Window 0's last literal ends 1 byte into window 1 on 06 00: the
    window's own chain starts on the 06, takes the first token's 01 (a copy-1 tag, with the next 22 as its offset)
    and is on the second bytes from there on. n tokens, then the filler."""
    def fn(s):
        _filler(s, WIN - 100)
        _lit_to(s, WIN + 1, tail=b"\x06")
        for _ in range(n):
            s.copy(2, 262, 9)
        assert s.body[-3:] == b"\x22\x06\x01"
        _filler(s, 3 * WIN - 300)
        s.lit(s.rand(7))
    return _build(fn, 2300 + n + 17 * seed)


def _apart_lit32(n, seed=0):
    def fn(s):
        _filler(s, WIN - 100)
        _lit_to(s, WIN + 1, tail=b"\x78" if n else b"\x7c")
        for j in range(n):
            s.lit(s.rand(30) + (b"\x78" if j < n - 1 else b"\x7c"))
        s.lit(s.rand(30) + b"\x00")      # 32 bytes more: the chains meet behind it
        _filler(s, 3 * WIN - 300)
        s.lit(s.rand(7))
    return _build(fn, 2200 + n + 17 * seed)


# ---------------------------------------------------------------- the cases

def _case_overshoot():
    ds = list(range(71)) + [127, 128, 129, IDX_EXT - 1, IDX_EXT, IDX_EXT + 1, 8191]
    out = [(f"d{d}", *_overshoot(d)) for d in ds]
    seen = set()
    for name, stream, _exp in out:
        w, X, W1 = _entries(stream)[0]
        seen.add(X - W1)
    assert seen == set(ds)
    # a literal that covers window 1 whole (WM_SKIP) and ends e bytes into window 2
    for e in (0, 1, 63, 64, IDX_EXT - 1, IDX_EXT, IDX_EXT + 1, 3000):
        name, (stream, exp) = f"skip_e{e}", _overshoot(WIN + e, windows=4)
        ent = _entries(stream)
        assert ent[0][1] == 2 * WIN + e and ent[1][1] == 2 * WIN + e      # window 1: no token; window 2: e bytes in
        out.append((name, stream, exp))
    return out


def _case_merge_distance():
    out, kp, steps = [], set(), set()
    # k tokens of the chain from the true entry before it meets the window's own chain (deep_walk counts these)
    plan = [("k0", _overshoot(2, seed=5, tail=b"\x01\x00"))]      # byte W1 is a copy-1 tag: 2 bytes, onto X
    plan += [(f"k{k}", _apart_copy1(k - 1)) for k in (1, 2, DEEP_STEPS - 1, DEEP_STEPS, DEEP_STEPS + 1)]
    # the index pass's step cap: both pointers' tokens together (2 n + 3; 2 n + 4 with the extra own token)
    for st in (IDX_STEPS - 1, IDX_STEPS, IDX_STEPS + 1):
        plan.append((f"steps{st}", _apart_copy1((st - 3) // 2, extra=False) if (st - 3) % 2 == 0
                     else _apart_copy1((st - 4) // 2, extra=True)))
    # a merge around W1 + IDX_EXT, in few steps (32-byte tokens): under it; just past it, which still resolves, since
    # no token at or past W1 + IDX_EXT is read; and one token further, which does not
    n = (IDX_EXT - 33) // 32 + 1
    plan += [("under_ext", _apart_lit32(n - 1)), ("past_ext", _apart_lit32(n)), ("past_ext_read", _apart_lit32(n + 1))]
    # the extension ends first, but after more than DEEP_STEPS tokens from X: recorded as slow (3-byte tokens)
    plan.append(("ext_after_deep_steps", _apart_copy2(IDX_EXT // 3 + 40)))
    for name, (stream, exp) in plan:
        w, X, W1 = _entries(stream)[0]
        r = _walk(stream, X, W1)
        if name == "ext_after_deep_steps":      # (wherever the chains meet behind the run, if they do)
            assert (r["m"] is None or r["m"] > W1 + IDX_EXT) and 2 * (IDX_EXT // 3) < IDX_STEPS, r
            assert _answer(stream, X, W1) == "slow"
            out.append((name, stream, exp))
            continue
        assert r["m"] is not None, name
        kp.add(r["kp"])
        steps.add(r["steps"])
        if name == "k0":
            # the window's own chain reaches X by itself: byte W1 must be a 2-byte token's tag
            assert X == W1 + 2 and r["kp"] == 0, (name, r)
        if name == "under_ext":
            assert r["m"] < W1 + IDX_EXT and _answer(stream, X, W1) == "merge", r
        if name == "past_ext":
            assert 0 < r["m"] - (W1 + IDX_EXT) <= 32 and r["steps"] < IDX_STEPS and _answer(stream, X, W1) == "merge", r
        if name == "past_ext_read":
            assert 32 < r["m"] - (W1 + IDX_EXT) <= 64 and r["steps"] < IDX_STEPS and _answer(stream, X, W1) == "none", r
        out.append((name, stream, exp))
    assert kp >= {0, 1, 2, DEEP_STEPS - 1, DEEP_STEPS, DEEP_STEPS + 1}, kp
    assert steps >= {IDX_STEPS - 1, IDX_STEPS, IDX_STEPS + 1}, steps
    by = {name: _answer(stream, *_entries(stream)[0][1:]) for name, stream, _e in out}
    assert by[f"steps{IDX_STEPS}"] == "merge" and by[f"steps{IDX_STEPS + 1}"] == "slow", by
    return out


def _case_never_merges():
    out = []
    # the second of four windows: the pattern runs through all of window 1 and 100 bytes on
    out.append(("second_window", *_apart_copy1(0, through=2 * WIN + 100, windows=4)))
    # the last window, the pattern up to the end of the page: a whole window, a short one, and windows 1 and 2
    out.append(("last_window", *_apart_copy1(0, through=2 * WIN - 1, seed=1, trail=False)))
    out.append(("last_window_short", *_apart_copy1(0, through=WIN + 3000, seed=2, trail=False)))
    out.append(("last_two_windows", *_apart_copy1(0, through=3 * WIN - 1, seed=3, trail=False)))
    for name, stream, _exp in out:
        w, X, W1 = _entries(stream)[0]
        r = _walk(stream, X, W1)
        assert r["m"] is None or r["m"] >= W1 + WIN, (name, r)
    return out


def _case_changed_entry():
    """Window 1 never merges, so window 2's record was made for window 1's own exit, one byte off the true
    entry; ordinary tokens follow at once, or the pattern runs on a little."""
    out = []
    for i, extra in enumerate((0, 1, 2, 60, 300)):
        name, (stream, exp) = f"run_ends_{extra}_into_window_2", _apart_copy1(0, through=2 * WIN + extra, windows=4, seed=3 + i)
        (w1, X1, W1), (w2, X2, W2) = _entries(stream)[:2]
        assert _walk(stream, X1, W1)["m"] is None or _walk(stream, X1, W1)["m"] >= W2
        # the own chain of window 1 (from W1) leaves it at another byte than the true chain
        q = W1
        while q < W2:
            q += _tok(stream, q)[0]
        assert q != X2, (name, q, X2)
        out.append((name, stream, exp))
    return out


def _case_ends():
    out = []

    def two(tail_len, d, seed):
        """Two windows, the second `tail_len` bytes long; window 0's last token ends d bytes into it."""
        def fn(s):
            _filler(s, WIN - 100)
            _lit_to(s, WIN + d)
            rest = tail_len - d
            assert rest == 0 or rest >= 2
            while rest:
                take = rest if rest <= 40 else min(rest - 2, 30)
                s.lit(s.rand(take - 1))
                rest -= take
            assert s.ipos == WIN + tail_len
        return _build(fn, seed)

    # the stream ends inside the extension / the last window is shorter than IDX_EXT
    for tail_len in (1, 2, 5, 100, IDX_EXT - 1, IDX_EXT, IDX_EXT + 1):
        for d in sorted({0, min(3, tail_len - 2), tail_len}):
            if 0 <= d <= tail_len and (tail_len - d == 0 or tail_len - d >= 2):
                out.append((f"second_window_{tail_len}_bytes_d{d}", *two(tail_len, d, 2400 + tail_len + d)))
    assert any(n.startswith("second_window_1_bytes") for n, _s, _e in out)
    # the stream ends exactly on a window boundary: one window, two windows
    out.append(("ends_on_boundary_1", *two(0, 0, 2450)))
    assert len(out[-1][1]) == WIN

    def full2(s):
        _filler(s, WIN - 100)
        _lit_to(s, WIN + 9)
        _filler(s, 2 * WIN - 100)
        _lit_to(s, 2 * WIN)
    out.append(("ends_on_boundary_2", *_build(full2, 2451)))
    assert len(out[-1][1]) == 2 * WIN

    # a page of one window
    def one(s):
        _filler(s, 5000)
        s.lit(s.rand(7))
    out.append(("one_window", *_build(one, 2452)))
    assert len(out[-1][1]) < WIN
    return out


CASES = {
    "overshoot": _case_overshoot,
    "merge_distance": _case_merge_distance,
    "never_merges": _case_never_merges,
    "changed_entry": _case_changed_entry,
    "ends": _case_ends,
}


@pytest.fixture(scope="module")
def dec():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _window_entries(dec, n_win):
    from pfloor import _native
    L = _native.lib()
    L.pf_debug_snappy_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    wins = np.zeros((n_win, 4), np.uint32)
    assert L.pf_debug_snappy_tables(dec.h, None, 0, wins.ctypes.data, n_win, None, None) == 0
    return wins


@pytest.mark.parametrize("group", list(CASES))
def test_successor_record(dec, group):
    wrong = []
    cases = CASES[group]()
    for name, stream, exp in cases:
        assert len(stream) <= 4 * WIN and len(exp) <= T.BLOCK, name
        got, code = dec.snappy_decompress(stream, cap=len(exp))
        if got != exp:
            at = next((i for i, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp))) if isinstance(got, bytes) else got
            wrong.append(f"{name}: output differs (first at byte {at} of {len(exp)}; status / code {code})")
            continue
        if code != FB_OK:
            wrong.append(f"{name}: pf_snappy_last_fallback {code}, expected FB_OK")
            continue
        ent = _entries(stream)
        wins = _window_entries(dec, len(ent) + 1)
        for w, X, W1 in ent:
            if int(wins[w][0]) != X:
                wrong.append(f"{name}: window {w} entry {int(wins[w][0])}, true entry {X}")
            if X >= min(W1 + WIN, len(stream)) and int(wins[w][3]) != WM_SKIP:
                wrong.append(f"{name}: window {w} mode {int(wins[w][3])}, expected WM_SKIP")
    assert not wrong, "\n".join(wrong)


def test_direct_page_overshoot(dec, oracle, tmp_path):
    """The overshoot sweep d = 0..8 through DIRECT_VALUES pages (built as test_gpu_snappy_pages.py builds its
    pages: OPTIONAL INT64, 8192 values, so each page's output is 8 + 65536 bytes and crosses the 64 KiB mark
    by 8 bytes; the compressed body is kept to four windows by 64-byte copies behind the boundary under test)."""
    from pfloor.decoder import decode_file
    nv = NV_OPT
    head = _levels(nv)
    total = len(head) + 8 * nv
    body, values, unc, ds = bytearray(), [], 0, list(range(9))
    for d in ds:
        def fn(s):
            s.lit(head + s.rand(100))
            _filler(s, WIN - 100)
            _lit_to(s, WIN + d)
            _filler(s, 2 * WIN + 500)
            while s.opos < T.BLOCK - 400:
                s.lit(s.rand(int(s.rng.integers(1, 24)))).copy(2, 8 * int(s.rng.integers(1, 500)), 64)
            _end(s, total)
        stream, exp = _build(fn, 2500 + d)
        assert len(exp) == total and exp[:len(head)] == head and 2 * WIN < len(stream) <= 4 * WIN
        assert _entries(stream)[0][1] == WIN + d
        values.append(np.frombuffer(exp[len(head):], dtype=np.int64))
        page = _data_page(stream, total, nv, statistics=True)
        body += page
        unc += len(page) - len(stream) + total
    path = str(tmp_path / "entry_direct.parquet")
    _write(path, 2, True, body, nv * len(ds), len(ds), unc=unc)
    got = decode_file(path, decoder=dec)
    assert got["_status"] == 0, got["_error"]
    gv = np.frombuffer(got[(0, 0)]["values"].tobytes(), np.int64)
    jobs, direct = _debug(dec)
    for p, d in enumerate(ds):
        ne = np.flatnonzero(gv[p * nv:(p + 1) * nv] != values[p])
        assert not len(ne), f"d={d}: {len(ne)} values differ, first {ne[0]} (fallback {jobs[p][0]}, direct {direct[p]})"
    with oracle.open(path) as of:
        ref = of.decode(0, 0)
        assert ref["status"] == 0, ref["error"]
        assert_chunk_equal(got[(0, 0)], ref, "successor record, direct pages")
    assert [(jobs[p][0], direct[p]) for p in range(len(ds))] == [(FB_OK, DIRECT_VALUES)] * len(ds)
