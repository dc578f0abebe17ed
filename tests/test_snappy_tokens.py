"""Hand-assembled Snappy streams (snappy_tokens.py) on the CPU: three independent readers must agree on
what every stream means before the kernels are asked (test_gpu_snappy_tokens.py). For a valid stream
the assembler's expectation (plain definition of the format), the oracle (pfo_snappy_uncompress) and
pyarrow's Google Snappy give the same bytes; an invalid stream is refused by the oracle and by pyarrow.
The streams hold tokens no compressor of the suite emits (over-wide literal length fields, adjacent
literals, copies of 1-3 bytes, copy-4 with small offsets, ...): valid Snappy that a reader gets from
writers other than snappy-java. The token parser the compressor's tests read streams with (snappy_tokens.parse)
must find in every valid stream exactly the tokens the assembler put there and refuse every invalid one, and
compressor_errors must name each single departure from the compressor's grammar."""
import pyarrow as pa
import pytest

import snappy_tokens as T

GROUPS = "abcdefgh"


def test_assembler_by_hand():
    """The assembler itself against streams written out byte by byte."""
    s = T.Stream()
    s.lit(b"abcd").copy(1, 4, 6).copy(2, 1, 3).lit(b"xy", nb=2).copy(3, 2, 2)
    stream, exp = s.finish()
    assert stream == bytes([17, 3 << 2]) + b"abcd" + bytes([1 | (2 << 2), 4, 2 | (2 << 2), 1, 0, 61 << 2, 1, 0]) + b"xy" + \
        bytes([3 | (1 << 2), 2, 0, 0, 0])
    assert exp == b"abcdabcdabbbbxyxy"
    assert T.varint(5, pad=2) == b"\x85\x80\x00" and T.varint(300) == b"\xac\x02"
    s = T.Stream(pre=1)
    s.lit(b"q" * 10).next_tag_at(125, 128)
    assert s.ipos == 125
    s.fill_output_to(4096)
    assert s.opos == 4096
    stream, exp = T.Stream().raw(b"\x01\x00", 4).finish()
    assert stream == b"\x04\x01\x00" and exp is None


def test_parser_by_hand():
    """parse on a stream written out byte by byte: kinds, offsets, lengths, input and output positions."""
    stream = bytes([17, 3 << 2]) + b"abcd" + bytes([1 | (2 << 2), 4, 2 | (2 << 2), 1, 0, 61 << 2, 1, 0]) + b"xy" + \
        bytes([3 | (1 << 2), 2, 0, 0, 0])
    declared, toks = T.parse(stream)
    assert declared == 17
    assert toks == [(T.LITERAL, 0, 4, 1, 0), (T.COPY1, 4, 6, 6, 4), (T.COPY2, 1, 3, 8, 10), (T.LITERAL, 0, 2, 11, 13),
                    (T.COPY4, 2, 2, 16, 15)]
    assert T.token_sizes(stream, toks) == [5, 2, 3, 5, 5]
    assert T.expand(stream, toks) == b"abcdabcdabbbbxyxy"
    assert T.parse(b"\x00") == (0, [])
    assert T.parse(b"\x85\x80\x00" + bytes([4 << 2]) + b"hello")[1] == [(T.LITERAL, 0, 5, 3, 0)]


@pytest.mark.parametrize("group", GROUPS)
def test_parser_inverts_assembler(group):
    """On every valid stream of the corpus parse finds the tokens Stream was given, and they expand to the
    assembler's output."""
    for name, stream, exp, _fb, _tags in T.valid_corpus()[group]:
        declared, toks = T.parse(stream)
        assert declared == len(exp), name
        pre = len(stream) - sum(T.token_sizes(stream, toks)) if toks else len(stream)
        assert [(k, o, ln, at - pre, op) for k, o, ln, at, op in toks] == list(T.ASSEMBLED[name]), name
        assert T.expand(stream, toks) == exp, name


def test_parser_refuses_invalid_streams():
    for name, stream, _declared in T.invalid_corpus():
        with pytest.raises(ValueError):
            T.parse(stream)
            pytest.fail(f"{name}: parse accepted it")


def test_compressor_grammar_checker():
    """compressor_errors passes a stream in the compressor's grammar and names every single departure from it."""
    def errors(build, n=None, pad=0):
        s = T.Stream(7, pad=pad)
        build(s)
        stream, exp = s.finish()
        return T.compressor_errors(stream, len(exp) if n is None else n)

    def good(s):
        s.lit(s.rand(2100)).copy(2, 200, 64).copy(1, 200, 4).lit(s.rand(60)).copy(1, 2047, 11).lit(s.rand(61))
        s.copy(2, 2048, 11).copy(2, 100, 12).lit(s.rand(256)).copy(2, 90, 60).copy(1, 90, 5)
        s.fill_output_to(T.JOB)
        s.lit(s.rand(70)).copy(1, 70, 9).lit(s.rand(3))
    assert errors(good) == []
    assert errors(lambda s: None) == [] and errors(lambda s: s.lit(b"x")) == []
    bad = {
        "copy length": lambda s: s.lit(s.rand(9)).copy(2, 5, 3),
        "copy-2 where the compressor writes copy-1": lambda s: s.lit(s.rand(2100)).copy(2, 2047, 11),
        "copy-4 where": lambda s: s.lit(s.rand(300)).copy(3, 200, 20),
        "literal header of 2 bytes, minimal is 1": lambda s: s.lit(s.rand(60), nb=1).copy(1, 9, 4),
        "literal header of 3 bytes, minimal is 2": lambda s: s.lit(s.rand(256), nb=2).copy(1, 9, 4),
        "reads before the start of its own job": lambda s: s.lit(s.rand(T.JOB)).copy(1, 1, 4),
        "crosses a multiple": lambda s: s.lit(s.rand(T.JOB - 2)).copy(1, 9, 4),
        "is not the canonical varint": lambda s: s.lit(s.rand(9)),
        "bytes for 10, bound 13": lambda s: [s.lit(b"z") for _ in range(10)],     # ten literals of one byte: 20 bytes
    }
    for what, build in bad.items():
        got = errors(build, pad=1 if "varint" in what else 0)
        assert len(got) >= 1 and any(what in e for e in got), (what, got)
    assert any("declares" in e for e in errors(lambda s: s.lit(b"abc"), n=4))
    assert T.compressor_errors(b"\x05\x01\x00", 5)[0].startswith("not a Snappy stream")
    assert T.job_bound(8192) == 8192 + 126 + 3 and T.job_bound(64) == 67 and T.job_bound(65) == 69


@pytest.mark.parametrize("group", GROUPS)
def test_valid_streams_three_readers_agree(oracle, group):
    for name, stream, exp, _fb, _tags in T.valid_corpus()[group]:
        got = oracle.snappy_uncompress(stream)
        assert got == exp, f"{name}: oracle"
        if exp:   # (pyarrow has no zero-length output buffer; the empty stream is the oracle's and the assembler's)
            assert pa.decompress(stream, decompressed_size=len(exp), codec="snappy").to_pybytes() == exp, f"{name}: pyarrow"


def test_every_tag_byte_is_covered():
    """All 256 tag byte values appear as a valid token somewhere in the corpus."""
    tags = set()
    for cases in T.valid_corpus().values():
        for case in cases:
            tags |= case[4]
    assert tags == set(range(256)), sorted(set(range(256)) - tags)


def test_fallback_codes_are_pinned():
    """Block-structured classes a-f and h take the block-parallel path (code 0) except the literal with
    a 4-byte length field; g pins its two cross-block cases to the whole-page re-run."""
    for group, cases in T.valid_corpus().items():
        for name, _s, _e, fb, _t in cases:
            if group != "g" and "nb4" not in name:
                assert fb == T.FB_OK, name
    assert sorted(n for n, _s, _e, fb, _t in T.valid_corpus()["g"] if fb == T.FB_REDO) == \
        ["g.block2_reaches_1_back", "g.block2_reaches_70000_back"]
    assert [n for n, _s, _e, fb, _t in T.valid_corpus()["a"] if fb == T.FB_SERIAL] == ["a.lit_nb4_len1", "a.lit_nb4_len300"]


def test_block_structure_of_the_corpus():
    """What the expected codes rest on, checked on the token lists themselves: in a code-0 stream no copy
    reads across a 64 KiB mark at which a token starts."""
    for group, cases in T.valid_corpus().items():
        for name, stream, exp, fb, _t in cases:
            marks, crossing = _walk(stream)
            bad = [c for c in crossing if any(c[0] < m <= c[1] for m in marks)]
            assert (not bad) == (fb != T.FB_REDO), (name, bad[:3])


def _walk(stream):
    """Token starts at 64 KiB output marks, and (source start, copy start) of every copy."""
    i, v, sh = 0, 0, 0
    while True:
        c = stream[i]
        i += 1
        v |= (c & 0x7F) << sh
        sh += 7
        if not c & 0x80:
            break
    op, marks, copies = 0, set(), []
    while i < len(stream):
        tag = stream[i]
        if op and op % T.BLOCK == 0:
            marks.add(op)
        kind, L = tag & 3, tag >> 2
        if kind == 0:
            nb = L - 59 if L >= 60 else 0
            ln = (int.from_bytes(stream[i + 1:i + 1 + nb], "little") if nb else L) + 1
            i += 1 + nb + ln
            op += ln
            continue
        if kind == 1:
            ln, off, i = 4 + (L & 7), ((tag >> 5) << 8) | stream[i + 1], i + 2
        elif kind == 2:
            ln, off, i = L + 1, int.from_bytes(stream[i + 1:i + 3], "little"), i + 3
        else:
            ln, off, i = L + 1, int.from_bytes(stream[i + 1:i + 5], "little"), i + 5
        copies.append((op - off, op))
        op += ln
    assert op == v
    return marks, copies


def test_invalid_streams_are_refused(oracle):
    cases = T.invalid_corpus()
    assert len(cases) == len({c[0] for c in cases}) and len(cases) > 60
    for name, stream, declared in cases:
        got = oracle.snappy_uncompress(stream)
        assert got is None or (isinstance(got, int) and got < 0), f"{name}: the oracle accepted it"
        with pytest.raises(Exception):
            pa.decompress(stream, decompressed_size=max(declared, 1), codec="snappy")
            pytest.fail(f"{name}: pyarrow accepted it")
