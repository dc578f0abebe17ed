"""Token-level Snappy stream assembler and the hand-assembled corpus built with it.

Every other Snappy stream of the suite comes out of a compressor, which emits a narrow grammar and
chooses its own tokens. Here a stream is an explicit token list: Stream.lit / Stream.copy append one
token each and keep the expected output by the plain definition of the format (a literal appends its
data; a copy appends `length` bytes taken one at a time from `offset` back, so it may overlap its own
output). Neither the oracle nor a library is called: test_snappy_tokens.py checks on the CPU that the
oracle and pyarrow's Google Snappy read every stream the same way, and test_gpu_snappy_tokens.py then
asks the kernels.

parse() is the assembler's inverse (stream -> token list) and compressor_errors() holds a parsed stream to the
grammar of k_snappy_compress: test_gpu_snappy_compress.py and test_gpu_write_bytes.py read the compressor's own
choices with them.

valid_corpus() / invalid_corpus() return the case tables, grouped by the letters of the comments below.
A valid case is (name, stream, expected, fb, tags) with fb the pf_snappy_last_fallback code it must take
and tags the tag byte values of its tokens; an invalid one is (name, stream, declared length). The decoder constants a case guards are named next to it (they are today's values: a retune moves the
case with the constant)."""
import functools

import numpy as np

BLOCK = 65536       # SNAP_BLOCK (pf_snappy_par.h): Google Snappy block = executor piece
# pf_snappy_last_fallback codes (pf_snappy_par.h)
FB_OK, FB_WHOLE, FB_REDO, FB_SERIAL = 0, 1, 2, 3


def varint(v, pad=0):
    """LEB128 of v; pad > 0 appends that many redundant bytes (0x85 0x80 0x00 is 5 with pad=2)."""
    out = bytearray()
    while v >= 128:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    if pad:
        out[-1] |= 0x80
        out += b"\x80" * (pad - 1) + b"\x00"
    assert len(out) <= 5, "a Snappy preamble is at most 5 bytes"
    return bytes(out)


class Stream:
    """One raw Snappy stream under construction.

    pre: the preamble length the input positions are computed with (next_tag_at needs input
    positions before the total output, and so the preamble, is known); finish() asserts it.
    pad: redundant preamble bytes (non-canonical varint)."""

    def __init__(self, seed=0, pre=None, pad=0):
        self.rng = np.random.default_rng(seed)
        self.body = bytearray()
        self.out = bytearray()
        self.pre = pre
        self.pad = pad
        self.tags = set()      # tag bytes emitted as valid tokens
        self.tokens = []       # (kind, offset, length, position in the body, output position): what parse() must find
        self.valid = True

    # ---- positions
    @property
    def opos(self):
        return len(self.out)

    @property
    def ipos(self):
        assert self.pre is not None, "input positions need Stream(pre=...)"
        return self.pre + len(self.body)

    def rand(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    # ---- tokens
    def lit(self, data, nb=None):
        """Literal; nb in 0..4 forces the width of the length field (0: length in the tag)."""
        n = len(data) - 1
        assert n >= 0
        if nb is None:
            nb = 0 if n < 60 else 1 if n < 1 << 8 else 2 if n < 1 << 16 else 3 if n < 1 << 24 else 4
        assert 0 <= nb <= 4
        if nb == 0:
            assert n < 60, "a literal longer than 60 bytes needs a length field"
            tag = n << 2
            self.body.append(tag)
        else:
            assert n < 1 << (8 * nb), "length field too narrow"
            tag = (59 + nb) << 2
            self.body.append(tag)
            self.body += n.to_bytes(nb, "little")
        self.tags.add(tag)
        self.body += data
        self.tokens.append((0, 0, len(data), len(self.body) - len(data) - 1 - nb, len(self.out)))
        self.out += data
        return self

    def copy(self, kind, offset, length):
        """Copy with a 1- (kind 1), 2- (kind 2) or 4-byte (kind 3) offset."""
        if kind == 1:
            assert 4 <= length <= 11 and 0 < offset < 2048
            tag = 1 | ((length - 4) << 2) | ((offset >> 8) << 5)
            enc = bytes([tag, offset & 0xFF])
        elif kind == 2:
            assert 1 <= length <= 64 and 0 < offset < 1 << 16
            tag = 2 | ((length - 1) << 2)
            enc = bytes([tag]) + offset.to_bytes(2, "little")
        else:
            assert kind == 3 and 1 <= length <= 64 and 0 < offset < 1 << 32
            tag = 3 | ((length - 1) << 2)
            enc = bytes([tag]) + offset.to_bytes(4, "little")
        assert offset <= len(self.out), "copy reaches before the output start"
        self.tags.add(tag)
        self.tokens.append((kind, offset, length, len(self.body), len(self.out)))
        self.body += enc
        a = len(self.out) - offset
        if offset >= length:
            self.out += self.out[a:a + length]
        else:
            for k in range(length):       # overlaps its own output: byte by byte
                self.out.append(self.out[a + k])
        return self

    def auto_copy(self, offset, length):
        """The kind a compressor would pick."""
        kind = 1 if 4 <= length <= 11 and offset < 2048 else 2 if offset < 65536 else 3
        return self.copy(kind, offset, length)

    def raw(self, data, produces=0):
        """Arbitrary tag / operand bytes (invalid streams): the expectation becomes None. `produces`
        keeps the output position moving so that valid tokens can follow."""
        self.valid = False
        self.body += data
        self.out += bytes(produces)
        return self

    # ---- placement
    def fill_output_to(self, multiple, before=0):
        """A filler literal of random bytes so that the next token starts at an output multiple
        (or `before` bytes short of one)."""
        need = (-len(self.out) - before) % multiple
        if need:
            self.lit(self.rand(need))
        return self

    def room(self):
        """Output bytes left in the current 64 KiB block."""
        return BLOCK - len(self.out) % BLOCK

    def next_tag_at(self, k, modulus, min_pos=0):
        """A filler literal sized so that the next tag byte lands at input offset == k (mod modulus),
        at or after min_pos."""
        pos = self.ipos
        gap = (k - pos) % modulus
        while gap < 2 or pos + gap < min_pos:
            gap += modulus
        for h, top in ((1, 60), (2, 1 << 8), (3, 1 << 16), (4, 1 << 24)):
            d = gap - h
            if 1 <= d <= top:
                self.lit(self.rand(d), nb=h - 1)
                break
        else:
            raise AssertionError("gap too long for one filler literal")
        assert self.ipos % modulus == k % modulus and self.ipos >= min_pos
        return self

    # ---- result
    def finish(self, declared=None):
        """(stream bytes, expected output or None for a stream made invalid on purpose)."""
        total = len(self.out) if declared is None else declared
        pre = varint(total, self.pad)
        if self.pre is not None:
            assert len(pre) == self.pre, f"preamble is {len(pre)} bytes, positions assumed {self.pre}"
        if declared is not None and declared != len(self.out):
            self.valid = False
        return pre + bytes(self.body), (bytes(self.out) if self.valid else None)


def build(fn, **kw):
    """fn(Stream) for streams that place tokens at input positions: the preamble length is found by trial."""
    for pre in (1, 2, 3, 4):
        s = Stream(pre=pre, **kw)
        fn(s)
        if len(varint(len(s.out), s.pad)) == pre:
            return s
    raise AssertionError("no consistent preamble length")


def mixed_block_tokens(s, nbytes):
    """About nbytes of mixed literals and copies that keep Google's block structure: a token starts
    at every 64 KiB mark and no copy reads across one."""
    rng = s.rng
    end = s.opos + nbytes
    while s.opos < end:
        inblk = s.opos % BLOCK
        if inblk < 64:
            s.lit(s.rand(int(rng.integers(64, 200))))
            continue
        if s.room() < 300:
            s.fill_output_to(BLOCK)
            continue
        if rng.random() < 0.3:
            s.lit(s.rand(int(rng.integers(1, 90))))
        else:
            off = int(min(inblk, rng.integers(1, 6000) if rng.random() < 0.8 else rng.integers(1, 65536)))
            s.auto_copy(max(off, 1), int(rng.integers(1, 65)))
    return s


# ============================================================================ the token parser
# The inverse of Stream, by the plain definition of the format: what a compressor emitted, token by token
# (test_gpu_snappy_compress.py reads k_snappy_compress's choices off it). test_snappy_tokens.py checks that
# it finds in every stream of valid_corpus() the tokens the assembler put there.

LITERAL, COPY1, COPY2, COPY4 = 0, 1, 2, 3     # token kinds = the tag's low two bits (Stream.copy's `kind`)


def parse(stream):
    """stream -> (declared length, [(kind, offset, length, in_pos, out_pos)]).

    kind: LITERAL / COPY1 / COPY2 / COPY4; offset: 0 for a literal; length: output bytes of the token;
    in_pos: position of its tag byte in `stream`; out_pos: output position it starts at. A stream that is
    not valid Snappy (truncated token, offset 0 or before the output start, output != declared length)
    raises ValueError."""
    stream = bytes(stream)
    i, declared, sh = 0, 0, 0
    while True:
        if i >= len(stream) or sh > 28:
            raise ValueError("bad length preamble")
        c = stream[i]
        i += 1
        declared |= (c & 0x7F) << sh
        sh += 7
        if not c & 0x80:
            break
    tokens, op, n = [], 0, len(stream)
    while i < n:
        tag, at = stream[i], i
        kind, hi = tag & 3, tag >> 2
        if kind == LITERAL:
            nb = hi - 59 if hi >= 60 else 0
            if i + 1 + nb > n:
                raise ValueError(f"literal length field cut off at input byte {at}")
            ln = (int.from_bytes(stream[i + 1:i + 1 + nb], "little") if nb else hi) + 1
            i += 1 + nb + ln
            off = 0
        else:
            opnd = (1, 2, 4)[kind - 1]
            if i + 1 + opnd > n:
                raise ValueError(f"copy operand cut off at input byte {at}")
            if kind == COPY1:
                ln, off = 4 + (hi & 7), ((tag >> 5) << 8) | stream[i + 1]
            else:
                ln, off = hi + 1, int.from_bytes(stream[i + 1:i + 1 + opnd], "little")
            i += 1 + opnd
            if off == 0 or off > op:
                raise ValueError(f"copy at input byte {at}: offset {off} with {op} bytes of output")
        if i > n:
            raise ValueError(f"literal data cut off (token at input byte {at})")
        tokens.append((kind, off, ln, at, op))
        op += ln
    if op != declared:
        raise ValueError(f"tokens give {op} bytes, preamble declares {declared}")
    return declared, tokens


def token_sizes(stream, tokens):
    """Input bytes of every token (tag, operand / length field, literal data)."""
    ends = [t[3] for t in tokens[1:]] + [len(stream)]
    return [e - t[3] for t, e in zip(tokens, ends)]


def expand(stream, tokens):
    """The output of a parsed stream: literals append their data, copies append byte by byte."""
    out = bytearray()
    for (kind, off, ln, at, op), size in zip(tokens, token_sizes(stream, tokens)):
        assert op == len(out)
        if kind == LITERAL:
            out += stream[at + size - ln:at + size]
        elif off >= ln:
            out += out[op - off:op - off + ln]
        else:
            for k in range(ln):
                out.append(out[op - off + k])
    return bytes(out)


# ============================================================================ the compressor's grammar
# What k_snappy_compress (pf_encode.hip) promises about its own streams, read off the parsed tokens. One
# wave compresses one job of JOB input bytes on its own, and a page's stream is the preamble followed by
# its jobs' outputs, so the tokens of job j are those whose output starts in [j * JOB, (j + 1) * JOB).

JOB = 8192          # SC_BLOCK (pf_enc_tables.h)


def job_bound(n):
    """Most bytes a job of n input bytes may take: n + n // 65 + 3.

    From the format: a literal of l bytes costs l + h with h = 1 (l <= 60), 2 (l <= 256) or 3; a copy of
    >= 4 bytes costs <= 3, so it saves >= 1. The compressor emits a literal only in front of a copy or as
    the job's last token, so every literal but the last pairs with the copy behind it, and the pair costs
    at most h - 1 over its bytes: 0 up to 60 literal bytes, 1 from 61 (the pair then covers >= 61 + 4 = 65
    bytes), 2 from 257 (>= 261 bytes): never more than one excess byte per 65 bytes covered. The last
    literal stands alone and costs at most 3 over its data."""
    return n + n // 65 + 3


def compressor_errors(stream, n):
    """[violation, ...] of the compressor's grammar in `stream`, the compressed form of n bytes."""
    try:
        declared, toks = parse(stream)
    except ValueError as e:
        return [f"not a Snappy stream: {e}"]
    errs = []
    if declared != n:
        errs.append(f"declares {declared} bytes for {n}")
    pre = toks[0][3] if toks else len(stream)
    if bytes(stream[:pre]) != varint(n):
        errs.append(f"preamble {bytes(stream[:pre]).hex()} is not the canonical varint of {n}")
    per_job = {}
    for (kind, off, ln, at, op), size in zip(toks, token_sizes(stream, toks)):
        j = op // JOB
        per_job[j] = per_job.get(j, 0) + size
        where = f"token at input byte {at} (output {op}, length {ln}, offset {off})"
        if (op + ln - 1) // JOB != j:
            errs.append(f"{where}: its output crosses a multiple of {JOB}")
        if kind == LITERAL:
            want = 1 if ln <= 60 else 2 if ln <= 256 else 3 if ln <= 65536 else 4
            if size - ln != want:
                errs.append(f"{where}: literal header of {size - ln} bytes, minimal is {want}")
            continue
        if not 4 <= ln <= 64:
            errs.append(f"{where}: copy length outside 4..64")
        if off < 1:
            errs.append(f"{where}: copy offset < 1")
        want = COPY1 if ln <= 11 and off < 2048 else COPY2
        if kind != want:
            errs.append(f"{where}: copy-{(1, 2, 4)[kind - 1]} where the compressor writes copy-{want}")
        if op - off < JOB * j:
            errs.append(f"{where}: reads before the start of its own job")
    for j, size in sorted(per_job.items()):
        ln = min(JOB, n - j * JOB)
        if size > job_bound(ln):
            errs.append(f"job {j}: {size} bytes for {ln}, bound {job_bound(ln)}")
    return errs


def job_slices(stream, n):
    """[(input start, input end)] of every job's tokens in `stream` (cut where a token starts at a multiple
    of JOB output bytes; needs a stream without compressor_errors)."""
    _declared, toks = parse(stream)
    starts = [t[3] for t in toks if t[4] % JOB == 0]
    assert len(starts) == (n + JOB - 1) // JOB, "a job does not start with a token"
    return list(zip(starts, starts[1:] + [len(stream)]))


# ============================================================================ the valid corpus

ASSEMBLED = {}      # case name -> the token list its Stream recorded (positions relative to the body)


def _case(name, s, fb=FB_OK):
    stream, exp = s.finish()
    assert exp is not None, name
    ASSEMBLED[name] = tuple(s.tokens)
    return (name, stream, exp, fb, frozenset(s.tags))


def _grammar():
    out = []
    # literals, length in the tag: every tag 0..59 << 2 (a canonical near copy between them)
    s = Stream(1)
    for n in range(1, 61):
        s.lit(s.rand(n), nb=0).copy(1, 1, 4)
    out.append(_case("a.lit_short_1_60", s))
    # literals with a length field wider than needed. Long ones run across a 64 KiB mark, so no token
    # starts there and the pieces merge (exec5_piece: sp[k] == SNAP_INVALID) -- still code 0.
    for nb, lens in ((1, (1, 60, 61, 256)), (2, (1, 257, 65536)), (3, (1, 65537))):
        s = Stream(10 + nb)
        s.lit(s.rand(3))
        for n in lens:
            s.lit(s.rand(n), nb=nb).copy(1, 1, 4)
        out.append(_case(f"a.lit_wide_nb{nb}", s))
    # a 4-byte length field: walk_tok (pf_snappy_parse.hip, "nb >= 4u ? 0xffffffffu") breaks the chain on
    # purpose, the index pass marks the page FB_SERIAL and the serial kernel decodes it.
    for n in (1, 300):
        s = Stream(20 + n)
        s.lit(s.rand(40)).copy(1, 7, 9).lit(s.rand(n), nb=4).copy(1, 1, 4).lit(s.rand(9))
        out.append(_case(f"a.lit_nb4_len{n}", s, FB_SERIAL))
    # copy-1: every length 4..11 x offset high bits 0..7 = all 64 tag values
    s = Stream(30)
    s.lit(s.rand(2100))
    for hi in range(8):
        for ln in range(4, 12):
            s.copy(1, (hi << 8) | (37 + 5 * hi + ln), ln).lit(s.rand(1))
    out.append(_case("a.copy1_all_tags", s))
    # copy-2 / copy-4: every length 1..64, including lengths 1..3 and offsets a compressor would give
    # another kind. One 70001-byte literal in front carries the large offsets; it runs across the first
    # 64 KiB mark and the stream ends before the second, so the whole stream is one merged piece (code 0).
    for kind, offs in ((2, (1, 2, 3, 255, 256, 2047, 2048, 65535)), (3, (1, 255, 256, 65535, 65536, 70000))):
        s = Stream(40 + kind)
        s.lit(s.rand(70001))
        for ln in range(1, 65):
            for off in offs:
                s.copy(kind, off, ln).lit(s.rand(1))
        assert s.opos < 2 * BLOCK
        out.append(_case(f"a.copy{kind if kind == 2 else 4}_len_1_64", s))
    # copy-4 offsets 65536 / 70000 in a stream whose whole input is one SNAP_WIN = 8 KiB index window:
    # 70 KB of output from 64-byte copies (32 + 64 k is never 65536: a copy straddles the mark)
    s = Stream(44)
    s.lit(s.rand(32))
    for _ in range(1100):
        s.copy(2, 32, 64)
    for ln in range(1, 65):
        for off in (65536, 70000):
            s.copy(3, off, ln).lit(s.rand(1))
    assert s.opos < 2 * BLOCK and len(s.body) + 3 < 8192
    out.append(_case("a.copy4_single_window", s))
    # the same lengths with small offsets inside one ordinary 64 KiB block
    s = Stream(45)
    s.lit(s.rand(300))
    for ln in range(1, 65):
        for kind in (2, 3):
            for off in (1, 2, 3, 255, 256):
                s.copy(kind, off, ln).lit(s.rand(1))
    assert s.opos < BLOCK
    out.append(_case("a.copy2_copy4_small_offsets", s))
    # adjacent literals: two, and a run of forty
    s = Stream(50)
    s.lit(s.rand(17)).lit(s.rand(44)).copy(1, 30, 8)
    out.append(_case("a.two_literals", s))
    s = Stream(51)
    for i in range(40):
        s.lit(s.rand(1 + (i * 37) % 60))
    s.copy(2, 100, 20)
    out.append(_case("a.forty_literals", s))
    # 100 adjacent copies of every kind, no literal between them
    s = Stream(52)
    s.lit(s.rand(100))
    for i in range(100):
        k = 1 + i % 3
        s.copy(k, 1 + (i * 7) % 100, 4 + i % 8 if k == 1 else 1 + (i * 5) % 64)
    out.append(_case("a.hundred_copies", s))
    return out


GRID_OFFSETS = (list(range(1, 81)) + [127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097,
                                      8191, 8192, 16383, 32767, 32768, 65535])
GRID_LENGTHS = (1, 2, 3, 4, 5, 11, 12, 15, 16, 17, 31, 32, 33, 63, 64)


def _grid():
    """b. Overlap / offset grid. A copy may not read across a 64 KiB mark in a block-structured stream,
    so every block starts with its own random preamble, long enough for the offsets used in it, and ends
    with fill_output_to(65536). Offset 65535 fits a block only as a 1-byte copy that ends it; the other
    lengths at that offset run in a stream whose first literal crosses the mark (merged pieces, code 0)."""
    s = Stream(60)
    started = False
    for off in GRID_OFFSETS[:-1]:
        for ln in GRID_LENGTHS:
            if not started or s.opos % BLOCK < off or s.room() < 200:
                s.fill_output_to(BLOCK)
                s.lit(s.rand(max(off, 64)))
                started = True
            s.auto_copy(off, ln).lit(s.rand(1))
    s.fill_output_to(BLOCK)
    s.lit(s.rand(65535)).copy(2, 65535, 1)          # the copy ends the block exactly
    assert s.opos % BLOCK == 0
    s.lit(s.rand(5))
    out = [_case("b.grid_in_blocks", s)]
    s = Stream(61)
    s.lit(s.rand(70001))
    for ln in GRID_LENGTHS:
        s.copy(2, 65535, ln).lit(s.rand(1))
    out.append(_case("b.grid_off_65535", s))
    return out


def _near_far():
    """c. A copy is far when its source starts more than XRING - X5_BATCH = 4096 - 764 = 3332 bytes behind
    the batch's start (exec5_piece: farc), so offsets 3332..4095 are near or far by their place in the
    batch; the literal width between the copies shifts that phase."""
    out = []
    for gap in (1, 5):
        s = Stream(70 + gap)
        s.lit(s.rand(4300))
        for off in range(3200, 4201):
            s.copy(2, off, 8).lit(s.rand(gap))
        assert s.opos < BLOCK
        out.append(_case(f"c.near_far_gap{gap}", s))
    return out


def _far_align():
    """d. Far-copy sources (offset >= 4200 > XRING): every source alignment mod 16 x every length 1..64
    (X5_FSLOT = 80: five aligned 16-byte chunks cover 64 bytes + a shift < 16)."""
    out = []
    s = Stream(80)
    s.lit(s.rand(8192))
    seen = set()
    for ln in range(1, 65):
        for al in range(16):
            off = 4200 + (s.opos - 4200 - al) % 16
            assert (s.opos - off) % 16 == al
            seen.add((al, ln, s.opos % 4))
            s.copy(2, off, ln).lit(s.rand(1))
    assert len({(a, l) for a, l, _ in seen}) == 1024 and {d for _, _, d in seen} == {0, 1, 2, 3}
    assert s.opos < BLOCK
    out.append(_case("d.far_alignment_grid", s))
    # XFAR = 24 far copies end a batch: 100 back to back, of 1 byte and of 64 bytes
    for ln in (1, 64):
        s = Stream(81 + ln)
        s.lit(s.rand(8192))
        for i in range(100):
            s.copy(2, 5000 + i % 7, ln)
        out.append(_case(f"d.far_x100_len{ln}", s))
    # the first token after a long literal is a far copy of bytes the executor is still storing: the
    # producer waits a batch (R5_NOP) for them to land
    s = Stream(83)
    s.lit(s.rand(50))
    for n, off in ((4200, 3400), (6000, 4000), (9000, 3333), (9000, 8999), (4200, 4200)):
        s.lit(s.rand(n)).copy(2, off, 40).lit(s.rand(3)).copy(1, 9, 6)
    assert s.opos < BLOCK
    out.append(_case("d.far_after_long_literal", s))
    s = Stream(84)
    s.lit(s.rand(5000)).copy(2, 5000, 64).lit(s.rand(2)).copy(2, 5066, 1)
    out.append(_case("d.far_source_byte0", s))
    return out


def _batch_edges():
    """e. Batch cuts and literal sizes."""
    out = []
    # 64 x X5_TPL = 128 tokens a batch: 1-byte tokens end a batch by count long before X5_BATCH = 764 bytes
    s = Stream(90)
    s.lit(s.rand(2))
    for i in range(5000):
        s.lit(s.rand(1)).copy(2, 2, 1)
    out.append(_case("e.one_byte_tokens_x5000", s))
    # 64-byte copies end a batch by bytes in mid-run (each block starts with a literal: copies stay in it)
    s = Stream(91)
    for _ in range(2):
        s.lit(s.rand(64))
        for _ in range(1023):
            s.copy(2, 64, 64)
        assert s.opos % BLOCK == 0
    s.lit(s.rand(7))
    out.append(_case("e.copies64_x2046", s))
    # literal sizes, each followed by a near copy of its own tail: 64 bytes a token step; XCHUNK = 1024;
    # XCHUNK + 64 = 1088 staging bound (lstaged); 2 KiB / 4 KiB = XRING; 8 KiB = SNAP_WIN (a whole index
    # window skipped); XS_SAT = 0x7fff; 64 KiB. A 3-byte literal in front keeps them off the 64 KiB marks.
    for n in (63, 64, 65, 66, 1023, 1024, 1025, 1087, 1088, 1089, 2047, 2048, 2049, 4095, 4096, 4097,
              8191, 8192, 8193, 32766, 32767, 32768, 32769, 32770, 65535, 65536):
        s = Stream(100 + n)
        s.lit(s.rand(3)).lit(s.rand(n)).copy(2, 20, 10).lit(s.rand(2)).copy(1, 5, 7)
        out.append(_case(f"e.literal_{n}", s))
    return out


def _straddle():
    """f. Tokens whose bytes straddle a parse unit of the input: SNAP_RB = 128-byte lane regions and
    SNAP_WIN = 8 KiB windows of the index pass, XCHUNK = 1 KiB chunks of the executor. Each in the first
    window and in the third."""
    toks = {
        "lit3": lambda s: s.lit(s.rand(300), nb=3),        # 4 header bytes
        "copy4": lambda s: s.copy(3, 50, 20),              # 5 bytes
        "copy2": lambda s: s.copy(2, 70, 33),              # 3 bytes
    }
    places = [("lit3", 128, (124, 125, 126, 127)), ("lit3", 8192, (8188, 8189, 8190, 8191)),
              ("copy4", 128, (123, 124, 125, 126, 127)), ("copy4", 8192, (8187, 8188, 8189, 8190, 8191)),
              ("copy2", 128, (126, 127))]
    places += [(t, 1024, (1020, 1021, 1022, 1023)) for t in toks]
    out = []
    for tok, mod, ks in places:
        for k in ks:
            for min_pos in (0, 2 * 8192):
                def fn(s):
                    s.lit(s.rand(100)).copy(1, 10, 5).copy(2, 40, 3)
                    s.next_tag_at(k, mod, min_pos)
                    toks[tok](s)
                    s.lit(s.rand(5)).copy(1, 3, 9).lit(s.rand(31))
                s = build(fn, seed=200 + k)
                out.append(_case(f"f.{tok}_at_{k}_mod_{mod}_from_{min_pos}", s))
    return out


def _pieces():
    """g. 64 KiB piece boundaries: three blocks and a tail."""
    out = []
    # a token ends exactly at each mark and the next starts there
    s = Stream(300)
    for _ in range(3):
        mixed_block_tokens(s, 60000)
        s.fill_output_to(BLOCK)
    mixed_block_tokens(s, 3000)
    out.append(_case("g.token_ends_at_each_mark", s))
    # a 64-byte copy straddles each mark: k_snappy_splits finds no token at the boundary
    # (sp[k] = SNAP_INVALID) and exec5_piece ("no token at this boundary: an earlier piece covers it")
    # runs the pieces as one from output byte 0 -- code 0
    s = Stream(301)
    for _ in range(3):
        mixed_block_tokens(s, 60000)
        s.fill_output_to(BLOCK, before=32)
        s.copy(2, 100, 64)
    mixed_block_tokens(s, 3000)
    out.append(_case("g.copy64_straddles_each_mark", s))
    # a copy that starts block 2 and reads the last byte of block 1, and one that reads 70000 bytes
    # back: exec5_piece's `bad` (off > otok - out_start) fails the piece, FB_REDO re-runs the page whole
    for name, off, lead in (("g.block2_reaches_1_back", 1, 0), ("g.block2_reaches_70000_back", 70000, 500)):
        s = Stream(302 + off)
        for _ in range(2):
            mixed_block_tokens(s, 60000)
            s.fill_output_to(BLOCK)
        if lead:
            s.lit(s.rand(lead))
        s.copy(3 if off > 65535 else 2, off, 30)
        mixed_block_tokens(s, 50000)
        s.fill_output_to(BLOCK)
        mixed_block_tokens(s, 3000)
        out.append(_case(name, s, FB_REDO))
    # one literal is a whole block
    s = Stream(304)
    mixed_block_tokens(s, 60000)
    s.fill_output_to(BLOCK)
    s.lit(s.rand(BLOCK))
    mixed_block_tokens(s, 60000)
    s.fill_output_to(BLOCK)
    mixed_block_tokens(s, 3000)
    out.append(_case("g.literal_is_one_block", s))
    return out


def _ends():
    """h. Stream ends and preambles."""
    out = []
    s = Stream(400)
    out.append(_case("h.declared_0", s))                      # the stream b"\x00"
    assert out[-1][1] == b"\x00"
    s = Stream(401)
    s.lit(b"Z")
    out.append(_case("h.declared_1", s))
    for n in (100, 200, 20000):                               # 1-, 2- and 3-byte preambles
        s = Stream(402 + n)
        s.lit(s.rand(n // 2)).copy(2, 30, 25)
        s.lit(s.rand(n - s.opos))
        out.append(_case(f"h.preamble_len_{n}", s))
    s = Stream(405, pad=2)
    s.lit(b"hello")
    out.append(_case("h.padded_preamble", s))
    assert out[-1][1][:3] == b"\x85\x80\x00"
    s = Stream(406, pad=1)
    s.lit(s.rand(300)).copy(1, 9, 11)
    out.append(_case("h.padded_preamble_311", s))
    # each token kind as the last token, total input length == 0, 1, 15 (mod 16): the executor stages
    # input in 16-byte chunks and the last one is partial
    last = {"lit": (lambda s: s.lit(s.rand(6)), 7), "copy1": (lambda s: s.copy(1, 33, 8), 2),
            "copy2": (lambda s: s.copy(2, 33, 50), 3), "copy4": (lambda s: s.copy(3, 33, 2), 5)}
    for name, (emit, tl) in last.items():
        for r in (0, 1, 15):
            def fn(s):
                s.lit(s.rand(200)).copy(1, 20, 6)
                s.next_tag_at((r - tl) % 16, 16)
                emit(s)
            s = build(fn, seed=410 + r)
            assert (s.pre + len(s.body)) % 16 == r
            out.append(_case(f"h.last_{name}_len_mod16_{r}", s))
    return out


@functools.lru_cache(maxsize=None)
def valid_corpus():
    """{group letter: [(name, stream, expected, fb, tags)]}"""
    return {"a": _grammar(), "b": _grid(), "c": _near_far(), "d": _far_align(), "e": _batch_edges(),
            "f": _straddle(), "g": _pieces(), "h": _ends()}


# ============================================================================ invalid streams

DEPTHS = {"first": 0, "mid": 70_000, "final": 200_000}   # valid output bytes in front of the damage
TOTAL = 200_000                                          # (mid: in the second 64 KiB piece)


@functools.lru_cache(maxsize=None)
def _valid_prefix(depth):
    s = Stream(500 + depth)
    if depth:
        mixed_block_tokens(s, depth)
    return bytes(s.body), bytes(s.out)


def _prefixed(depth, seed):
    s = Stream(seed)
    body, out = _valid_prefix(depth)
    s.body += body
    s.out += out
    return s


def _wide(v, nbytes):
    return int(v).to_bytes(nbytes, "little")


# damaged tokens that valid tokens can follow: name -> fn(stream)
_BAD_TOKENS = {
    "offset0_copy1": lambda s: s.raw(bytes([1 | (4 << 2), 0]), 8),
    "offset0_copy2": lambda s: s.raw(bytes([2 | (7 << 2), 0, 0]), 8),
    "offset0_copy4": lambda s: s.raw(bytes([3 | (7 << 2), 0, 0, 0, 0]), 8),
    # one past the bytes produced so far (at the first token: offset 1 with nothing produced)
    "offset_past_start": lambda s: s.raw(bytes([3 | (7 << 2)]) + _wide(s.opos + 1, 4), 8),
    # a literal longer than the rest of the input
    "literal_past_input": lambda s: s.raw(bytes([62 << 2]) + _wide(0xFFFFFF, 3), 0),
}

# operand bytes missing after the last tag: name -> (bytes, output the whole token would give)
_TRUNCATED = {
    "copy1": (bytes([1 | (4 << 2)]), 8), "copy2": (bytes([2 | (7 << 2)]), 8), "copy2_half": (bytes([2 | (7 << 2), 9]), 8),
    "copy4": (bytes([3 | (7 << 2)]), 8), "copy4_3of4": (bytes([3 | (7 << 2), 9, 0, 0]), 8),
    "lit_nb1": (bytes([60 << 2]), 70), "lit_nb2": (bytes([61 << 2, 70]), 71), "lit_nb3": (bytes([62 << 2, 70, 0]), 71),
    "lit_nb4": (bytes([63 << 2, 70, 0, 0]), 71),
    # a literal whose data runs past the input end (length field complete)
    "lit_data_short": (bytes([9 << 2]) + b"abcde", 10), "lit_nb1_data_short": (bytes([60 << 2, 99]) + b"x" * 99, 100),
}


@functools.lru_cache(maxsize=None)
def invalid_corpus():
    """[(name, stream, declared length)]: streams every decoder must refuse."""
    out = []

    def add(name, s, declared=None):
        stream, exp = s.finish(declared)
        assert exp is None, name
        out.append((name, stream, len(s.out) if declared is None else declared))

    for depth_name, depth in DEPTHS.items():
        for name, bad in _BAD_TOKENS.items():
            s = _prefixed(depth, 600)
            bad(s)
            if TOTAL > depth:       # valid block-structured tokens behind the damage
                if depth:
                    s.fill_output_to(BLOCK)
                mixed_block_tokens(s, TOTAL - depth)
            add(f"x.{name}@{depth_name}", s)
        # the damage is the stream's end: `depth` valid bytes, then
        for name, (data, produces) in _TRUNCATED.items():
            s = _prefixed(depth, 601)
            if depth == 0 and data[0] & 3:
                s.lit(s.rand(20))           # (something for the copy to read, were it whole)
            s.raw(data, produces)
            add(f"x.truncated_{name}@{depth_name}", s)
        s = _prefixed(depth, 602)                       # a copy that crosses the declared length
        s.lit(s.rand(40)).copy(2, 30, 64)
        add(f"x.copy_crosses_declared@{depth_name}", s, s.opos - 54)
        s = _prefixed(depth, 603)                       # a literal that crosses the declared length
        s.lit(s.rand(40))
        add(f"x.literal_crosses_declared@{depth_name}", s, s.opos - 1)
        for name, d in (("declared_larger", 1), ("declared_much_larger", 70_000), ("declared_smaller", -1)):
            s = _prefixed(depth, 604)
            s.lit(s.rand(40)).copy(1, 30, 6)
            add(f"x.{name}@{depth_name}", s, s.opos + d)
        for name, extra in (("extra_literal", lambda s: s.lit(b"!")), ("extra_copy", lambda s: s.copy(2, 9, 1))):
            s = _prefixed(depth, 605)
            s.lit(s.rand(40)).copy(1, 30, 6)
            done = s.opos
            extra(s)
            add(f"x.{name}@{depth_name}", s, done)
    return out
