"""k_snappy_compress (pf_encode.hip) token by token: what the compressor chose, not only whether it decodes.

Every input goes through pf_snappy_compress and the stream is checked four ways:
 a. round trip: the oracle, pyarrow's Google Snappy and the GPU read path give the input back;
 b. read path: pf_snappy_last_fallback is pinned to 0. pf_snappy_decompress runs the parse and executor kernels
    without k_snappy_head, so the literal-only codes of pf_snappy_par.h (FB_INPLACE = 4, FB_LITCOPY = 5) cannot
    occur on it: they belong to pages and are pinned in test_gpu_write_bytes.py. FB_REDO (2) or FB_SERIAL (3)
    would mean a stream the block-parallel executor refused: a copy across a 64 KiB mark, or a broken chain;
 c. token grammar and d. size: snappy_tokens.compressor_errors over the parsed tokens (copy lengths 4..64,
    copy-1 only for 4..11 bytes below offset 2048 and copy-2 otherwise, minimal literal headers, no copy out of
    its 8 KiB job, no token across a job boundary, canonical preamble, every job within job_bound).

The 12-bit hash table loses planted sources to collisions, and the winner among the lanes of one store is not
defined, so no token list is ever asserted: a statement about a planted copy holds where the GPU's own tokens
show that the copy was found. The planted cases run under 8 seeds each, and test_edge_classes_are_reached fails
if any class of edge was never produced."""
import collections

import numpy as np
import pytest

import snappy_tokens as T
from test_gpu_write import gpu_compress

pytestmark = pytest.mark.gpu

JOB = T.JOB
SEEDS = range(8)


@pytest.fixture(scope="module")
def dec():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def pa():
    return pytest.importorskip("pyarrow")


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ---------------------------------------------------------------- inputs
def planted(seed, off, L, lead=None, tail=10):
    """`lead` random bytes (default: off, and at least 300 so that the literal in front of the copy has a 3-byte
    header), then L bytes copied one at a time from `off` back, one byte that breaks the match, a random tail."""
    rng = np.random.default_rng((2, seed, off, L))
    lead = max(off, 300) if lead is None else lead
    assert lead >= off
    out = bytearray(_rand(rng, lead))
    for _ in range(L):
        out.append(out[-off])
    out.append(out[-off] ^ 0x5A)
    out += _rand(rng, tail)
    return bytes(out)


PLANTED_AT_200 = [4, 5, 11, 12] + list(range(59, 70)) + list(range(124, 133)) + list(range(188, 197))
PLANTED_OFFSETS = [64, 65, 2046, 2047, 2048, 2049, 4095, 4096, 8100]
PLANTED_SAME_WINDOW = [1, 2, 3, 7, 63]         # the candidate lies in the window of the match: found one window later
PLANTED_LENGTHS = [4, 11, 12, 64, 65]
PLANTED = {"at_200": [(200, L) for L in PLANTED_AT_200],
           "offsets": [(o, L) for o in PLANTED_OFFSETS for L in PLANTED_LENGTHS],
           "same_window": [(o, L) for o in PLANTED_SAME_WINDOW for L in PLANTED_LENGTHS]}


def planted_inputs(group):
    return {f"planted off={off} L={L} seed={s}": planted(s, off, L) for off, L in PLANTED[group] for s in SEEDS}


def two_copies(seed, N):
    """200 random bytes, a copy of bytes 20..40, a literal of N bytes (the break byte and N - 1 random ones), a copy
    of bytes that occurred once: 150 back where the literal is long enough to hold them, else bytes 60..80."""
    rng = np.random.default_rng((3, seed, N))
    out = bytearray(_rand(rng, 200))
    out += out[20:40]
    out.append(out[40] ^ 0x5A)
    out += _rand(rng, N - 1)
    src = len(out) - 150 if N >= 160 else 60
    assert len(out) - src >= 150
    out += out[src:src + 20]
    out.append(out[src + 20] ^ 0x5A)
    out += _rand(rng, 10)
    return bytes(out)


LITERALS_BETWEEN = [1, 2, 59, 60, 61, 62, 255, 256, 257, 258, 1000]


def literal_inputs():
    return {f"literal N={N} seed={s}": two_copies(s, N) for N in LITERALS_BETWEEN for s in SEEDS}


def _repetitive(rng, n):
    """n bytes of 40-byte random pieces drawn from a pool of 24: matches at many offsets."""
    pool = [_rand(rng, 40) for _ in range(24)]
    return b"".join(pool[i] for i in rng.integers(0, 24, n // 40 + 1))[:n]


def full_job_with_match(seed, short):
    """A job of exactly JOB bytes whose last 50 bytes (or the 50 before the last one) repeat the bytes 200 back."""
    rng = np.random.default_rng((4, seed, short))
    head = bytearray(_rand(rng, JOB - 50 - short))
    for _ in range(50):
        head.append(head[-200])
    if short:
        head.append(head[-200] ^ 0x5A)
    assert len(head) == JOB
    return bytes(head)


def boundary_cases():
    rng = np.random.default_rng(4)
    out = {}
    first = _repetitive(rng, JOB)
    out["second_job_repeats_first"] = first + first + first[:5]
    a = _rand(rng, JOB)
    out["source_ends_at_8191"] = a + a[JOB - 40:] + bytes([a[0] ^ 0x5A]) + _rand(rng, 20)
    for s in SEEDS:
        for short in (0, 1):
            job = full_job_with_match(s, short)
            out[f"match_ends_{short}_short_of_job seed={s}"] = job
            out[f"match_ends_{short}_short_of_job then_job seed={s}"] = job + _rand(rng, 100)
    return out


def pressure_cases():
    rng = np.random.default_rng(5)
    groups = (np.arange(JOB // 4, dtype=np.uint64) * 2654435761 % (1 << 32)).astype("<u4")   # odd multiplier: distinct
    assert len(set(groups.tolist())) == JOB // 4
    return {"two_symbols": rng.integers(0, 2, JOB, dtype=np.uint8).tobytes(),
            "two_symbols_runs": np.repeat(rng.integers(0, 2, JOB, dtype=np.uint8), rng.integers(1, 9, JOB))[:JOB].tobytes(),
            "distinct_groups": groups.tobytes(), "counter_groups": np.arange(JOB // 4, dtype="<u4").tobytes()}


SWEEP = list(range(401)) + list(range(8125, 8201)) + [16383, 16384, 16385, 65535, 65536, 65537]


# ---------------------------------------------------------------- the checks
STREAMS = {}        # label -> the GPU's stream, kept for test_edge_classes_are_reached


def check(dec, oracle, pa, data):
    """(stream, [what is wrong with it]) of one input: checks a-d of the module docstring."""
    comp = gpu_compress(dec, data)
    errs = T.compressor_errors(comp, len(data))                                   # c, d
    if oracle.snappy_uncompress(comp) != data:                                    # a
        return comp, errs + ["the oracle does not give the input back"]           # (the GPU is not handed a stream known bad)
    try:
        if data and pa.decompress(comp, decompressed_size=len(data), codec="snappy").to_pybytes() != data:
            errs.append("pyarrow does not give the input back")
    except Exception as e:
        errs.append(f"pyarrow refuses the stream: {e}")
    got, code = dec.snappy_decompress(comp, cap=max(1, len(data)))
    if got != data:
        errs.append(f"the GPU read path does not give the input back (status / code {code})")
    elif code != T.FB_OK:                                                         # b
        errs.append(f"pf_snappy_last_fallback {code}, expected {T.FB_OK}")
    return comp, errs


def check_all(dec, oracle, pa, inputs):
    """{label: stream} of `inputs` ({label: bytes}); every failing label is reported together."""
    streams, wrong = {}, []
    for label, data in inputs.items():
        streams[label], errs = check(dec, oracle, pa, data)
        wrong += [f"{label}: {e}" for e in errs[:4]]
    STREAMS.update(streams)
    assert not wrong, f"{len(wrong)} failures\n" + "\n".join(wrong[:60])
    return streams


def planted_copy(stream, at):
    """The copies that cover the match planted at output position `at`, if the compressor found it there: the
    copies from the one that starts at `at` on, as long as they follow one another at its offset."""
    _n, toks = T.parse(stream)
    mine = []
    for kind, off, ln, _at, op in toks:
        if kind != T.LITERAL and ((not mine and op == at) or (mine and op == mine[-1][1] + mine[-1][2] and off == mine[0][0])):
            mine.append((off, op, ln))
        elif mine:
            break
    return mine


CLASSES = ("copy60_then_copy5", "copy60_then_copy6", "copy60_then_copy7", "copy64_then_copy4", "literal_3byte_header_then_copy",
           "literal_60", "literal_61", "literal_256", "literal_257", "copy1_at_2047", "copy2_short_at_2048",
           "copy1_len11_below_2048", "copy2_len12_below_2048")


def classify(stream, reached):
    _n, toks = T.parse(stream)
    sizes = T.token_sizes(stream, toks)
    for i, ((kind, off, ln, _at, _op), size) in enumerate(zip(toks, sizes)):
        nxt = toks[i + 1] if i + 1 < len(toks) else None
        if kind == T.LITERAL:
            if ln in (60, 61, 256, 257) and nxt is not None and i > 0:      # between two copies
                reached[f"literal_{ln}"] += 1
            if size - ln == 3 and nxt is not None:
                reached["literal_3byte_header_then_copy"] += 1
            continue
        if nxt is not None and nxt[0] != T.LITERAL and nxt[1] == off:
            if ln == 60 and nxt[2] in (5, 6, 7):
                reached[f"copy60_then_copy{nxt[2]}"] += 1
            if ln == 64 and nxt[2] == 4:
                reached["copy64_then_copy4"] += 1
        if kind == T.COPY1 and off == 2047:
            reached["copy1_at_2047"] += 1
        if kind == T.COPY2 and off == 2048 and ln <= 11:
            reached["copy2_short_at_2048"] += 1
        if kind == T.COPY1 and ln == 11 and off < 2048:
            reached["copy1_len11_below_2048"] += 1
        if kind == T.COPY2 and ln == 12 and off < 2048:
            reached["copy2_len12_below_2048"] += 1


# ---------------------------------------------------------------- 1. length sweep
@pytest.mark.parametrize("family", ["zeros", "abcdefg"])
def test_length_sweep(dec, oracle, pa, family):
    """Every length 0..400, around one job (8125..8200), two jobs and 64 KiB. After the first 64-byte window the match
    runs to the end of the job, so its last copies take every residue of the length mod 64: the 60 + 5..7 split, tails
    of 0..3 bytes behind a copy, and the same behind a job boundary."""
    src = bytes(65537) if family == "zeros" else b"abcdefg" * (65537 // 7 + 1)
    check_all(dec, oracle, pa, {f"{family} n={n}": src[:n] for n in SWEEP})


# ---------------------------------------------------------------- 2. planted matches
@pytest.mark.parametrize("group", list(PLANTED))
def test_planted_matches(dec, oracle, pa, group):
    inputs = planted_inputs(group)
    assert max(len(d) for d in inputs.values()) <= JOB
    streams = check_all(dec, oracle, pa, inputs)
    if group == "same_window":      # found a window later, somewhere inside the planted bytes: no length to expect
        return
    # where the compressor found the planted source, its copies add up to the planted length
    wrong = []
    for off, L in PLANTED[group]:
        for s in SEEDS:
            mine = planted_copy(streams[f"planted off={off} L={L} seed={s}"], max(off, 300))
            if mine and mine[0][0] == off and sum(m[2] for m in mine) != L:
                wrong.append((off, L, s, mine))
    assert not wrong, wrong[:10]


# ---------------------------------------------------------------- 3. literal lengths between two copies
def test_literals_between_copies(dec, oracle, pa):
    check_all(dec, oracle, pa, literal_inputs())


# ---------------------------------------------------------------- 4. job boundaries
def test_job_boundaries(dec, oracle, pa):
    cases = boundary_cases()
    streams = check_all(dec, oracle, pa, cases)
    # jobs are independent: every job's tokens, behind a preamble of their own, are a stream of that job's bytes
    for name, data in cases.items():
        for j, (a, b) in enumerate(T.job_slices(streams[name], len(data))):
            part = data[j * JOB:(j + 1) * JOB]
            assert oracle.snappy_uncompress(T.varint(len(part)) + streams[name][a:b]) == part, (name, j)
    # a source that ends at byte 8191 is out of reach of the repeat at 8192: job 1 is one literal
    _n, toks = T.parse(streams["source_ends_at_8191"])
    assert [t[0] for t in toks if t[4] >= JOB] == [T.LITERAL]
    # a match planted up to the job's last byte, or one short of it, ends there wherever it was found
    for short in (0, 1):
        for follow in ("", " then_job"):
            found = 0
            for s in SEEDS:
                mine = planted_copy(streams[f"match_ends_{short}_short_of_job{follow} seed={s}"], JOB - 50 - short)
                if mine and mine[0][0] == 200:
                    found += 1
                    assert mine[-1][1] + mine[-1][2] == JOB - short, (short, follow, s, mine)
            assert found > 0, (short, follow)


# ---------------------------------------------------------------- 5. table pressure
def test_table_pressure(dec, oracle, pa):
    """A 2-symbol alphabet (every window matches, the 4096 entries are overwritten all the time) and 2048 distinct
    aligned groups (hardly a match, every store lands in a fresh or a colliding entry)."""
    check_all(dec, oracle, pa, pressure_cases())


# ---------------------------------------------------------------- coverage
def test_edge_classes_are_reached(dec):
    """Every edge class was produced at least once by the GPU's own tokens over the planted inputs (8 seeds each):
    the streams the tests above checked, or, when this test runs alone, compressed here."""
    reached = collections.Counter()
    inputs = dict(literal_inputs())
    for group in ("at_200", "offsets"):
        inputs.update(planted_inputs(group))
    broken = []
    for label, data in inputs.items():
        try:
            classify(STREAMS[label] if label in STREAMS else gpu_compress(dec, data), reached)
        except ValueError as e:
            broken.append(f"{label}: {e}")
    assert not broken, f"{len(broken)} streams do not parse\n" + "\n".join(broken[:20])
    print("edge classes reached:", {c: reached[c] for c in CLASSES})
    missing = [c for c in CLASSES if reached[c] == 0]
    assert not missing, (missing, dict(reached))
