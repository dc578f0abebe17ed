"""LZ4 block format test material (parquet-format codec LZ4_RAW): a pure-Python model of the
acceptance rules (the specification csrc/pf_lz4_core.h is held to), a sequence builder, the corpus
liblz4 compresses for us (pyarrow's "lz4_raw"), hand-assembled blocks, streams at the kernel's batch
and window edges, and the seeded mutations. No GPU, no native code."""
import os
import random
import re
import struct

import numpy as np
import pyarrow as pa

from zstd_frames import _text

B = 256     # sequences per LDS batch of k_lz4      (LZ4_BATCH in csrc/pf_lz4_core.h)
W = 8192    # bytes of the input window it stages   (LZ4_WINDOW)


def kernel_constants(root):
    """{name: value} of the constexpr uint32_t constants in the core's header text."""
    text = open(os.path.join(root, "parquet-floor_amd", "csrc", "pf_lz4_core.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint32_t (\w+) = (\d+);", text)}


# ---------------------------------------------------------------- the model
def model(src, size, why=None):
    """One raw LZ4 block that must produce exactly size bytes -> the bytes, or None when refused
    (why, a list, then gets the reason). The rules of DESIGN 4.35, one line each."""
    def refuse(reason):
        if why is not None:
            why.append(reason)
        return None

    n, ip, out = len(src), 0, bytearray()
    while True:
        if ip >= n:
            return refuse("input used up before a token")            # (an empty input too)
        tok = src[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                if ip >= n:
                    return refuse("input used up in a literal-length extension")
                b = src[ip]
                ip += 1
                ll += b
                if ll > n - ip or ll > size - len(out):
                    return refuse("literal length past the input or the output")
                if b != 255:
                    break
        if ll > n - ip or ll > size - len(out):
            return refuse("literal length past the input or the output")
        out += src[ip:ip + ll]
        ip += ll
        if ip == n:                                                    # the last sequence: its low nibble is ignored
            return bytes(out) if len(out) == size else refuse("output is not size bytes")
        if n - ip < 2:
            return refuse("input used up in the offset")
        off = src[ip] | src[ip + 1] << 8
        ip += 2
        if off == 0:
            return refuse("offset 0")
        if off > len(out):
            return refuse("offset past the bytes produced")
        ml = (tok & 15) + 4
        if tok & 15 == 15:
            while True:
                if ip >= n:
                    return refuse("input used up in a match-length extension")
                b = src[ip]
                ip += 1
                ml += b
                if ml > size - len(out):
                    return refuse("match length past the output")
                if b != 255:
                    break
        if ml > size - len(out):
            return refuse("match length past the output")
        pat = bytes(out[-off:])
        out += pat[:ml] if off >= ml else (pat * (ml // off + 1))[:ml]


def first_offset_at(src):
    """Position of the offset field of the block's first sequence (walked as the model walks it)."""
    ll, ip = src[0] >> 4, 1
    if ll == 15:
        while True:
            ll += src[ip]
            ip += 1
            if src[ip - 1] != 255:
                break
    assert ip + ll + 2 <= len(src)
    return ip + ll


# ---------------------------------------------------------------- builder
def _ext(v):
    """The extension bytes of a length whose nibble is 15: v = length - 15 (literals) or - 19 (match)."""
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return bytes(out)


def seq(literals, off=None, ml=None, low=0):
    """One sequence. off=None: the last one (no offset field; low = its ignored low nibble)."""
    ll = len(literals)
    nib = low if off is None else min(ml - 4, 15)
    out = bytes([min(ll, 15) << 4 | nib]) + (_ext(ll - 15) if ll >= 15 else b"") + literals
    if off is not None:
        out += struct.pack("<H", off) + (_ext(ml - 19) if ml >= 19 else b"")
    return out


def expand(parts):
    """Expected bytes of [(literals, off, ml)] (off None: no match), byte by byte."""
    out = bytearray()
    for lits, off, ml in parts:
        out += lits
        if off is not None:
            assert 0 < off <= len(out)
            for _ in range(ml):
                out.append(out[-off])
    return bytes(out)


def build(parts, low=0):
    """(block, content) of [(literals, off, ml)]; the last part has off None."""
    assert parts[-1][1] is None and all(p[1] is not None for p in parts[:-1])
    return b"".join(seq(l, o, m, low if o is None else 0) for l, o, m in parts), expand(parts)


def _rand(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


# ---------------------------------------------------------------- corpus
def corpus_inputs():
    """name -> bytes, in a fixed order."""
    rng = np.random.default_rng(17)
    out = {"empty": b"", "one": b"x"}
    for n in (300, 5000, 70000):
        out[f"text{n}"] = _text(n)
    out["zeros"] = bytes(100_000)
    out["random4k"] = rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()   # one literal run: a length of many 255s
    out["small_i32"] = rng.integers(0, 50, 4000).astype(np.int32).tobytes()
    out["abc5000"] = b"abc" * 5000                                            # offset 3, one very long match
    out["a70000_random"] = b"a" * 70_000 + rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    return out


def corpus():
    """[(name, block, content)]: every input as liblz4 compresses it."""
    codec = pa.Codec("lz4_raw")
    return [(name, codec.compress(data, asbytes=True), data) for name, data in corpus_inputs().items()]


# ---------------------------------------------------------------- hand blocks
def hand_blocks():
    """[(name, block, size, content or None)]: None = refused."""
    rng = random.Random(5)
    out = []

    def ok(name, parts, low=0):
        blk, content = build(parts, low)
        out.append((name, blk, len(content), content))

    def bad(name, blk, size):
        out.append((name, blk, size, None))

    tail = b"tail!"
    for ll in (14, 15, 16, 270, 525):                      # 15: extension byte 0; 270 = 15 + 255 + 0
        ok(f"ll{ll}", [(_rand(rng, ll), None, None)])
        ok(f"ll{ll}_then_match", [(_rand(rng, ll), 7, 9), (tail, None, None)])
    for ml in (4, 18, 19, 274, 1000):                      # 19: extension byte 0; 274 = 19 + 255 + 0
        ok(f"ml{ml}", [(b"abcdefgh", 8, ml), (tail, None, None)])
    for off in (1, 2, 3, 15, 16, 17):                      # matches longer than the offset, and than 256
        for ml in (max(4, off + 1), 40, 300):
            ok(f"off{off}_ml{ml}", [(_rand(rng, 17), off, ml), (tail, None, None)])
    ok("off65535", [(_rand(rng, 65535), 65535, 20), (tail, None, None)])
    ok("off_all_produced", [(b"0123456789", 10, 6), (tail, None, None)])
    bad("off_one_more", seq(b"0123456789", 11, 6) + seq(tail), 21)
    bad("off0", seq(b"0123456789", 0, 6) + seq(tail), 21)
    ok("tail4", [(b"abcdefgh", 8, 8), (b"wxyz", None, None)])          # liblz4's end-of-block rules are not enforced
    bad("ends_after_match", seq(b"abcdefgh", 8, 8), 16)
    bad("two_literal_only", seq(b"abc") + seq(b"def"), 6)
    ok("last_low_nibble", [(b"hello", None, None)], low=7)
    ok("last_low_nibble_after_match", [(b"abcdefgh", 8, 8), (tail, None, None)], low=15)
    ok("last_without_literals", [(b"abcdefgh", 8, 8), (b"", None, None)])
    out.append(("00", b"\x00", 0, b""))
    bad("empty_input", b"", 0)
    bad("00_size1", b"\x00", 1)
    bad("ll_run_of_255_to_the_end", b"\xf0" + b"\xff" * 40, 5000)
    bad("ml_run_of_255_to_the_end", seq(b"abcdefgh", 8, 19)[:-1] + b"\xff" * 40, 20000)
    bad("cut_in_offset", seq(b"abcdefgh", 8, 8)[:-1], 16)
    bad("cut_in_literals", seq(b"abcdefgh", 8, 8)[:5], 16)
    return out


# ---------------------------------------------------------------- batch edges
def batch_blocks():
    """[(name, block, size, content)]: streams of B-1 .. 2B+1 sequences (the last one included), and
    one of 2B+1 whose matches at the first and last slot of each batch read the batch's own output,
    the first of the second batch from a source that starts before the batch and ends inside it."""
    out = []
    for count in (B - 1, B, B + 1, 2 * B, 2 * B + 1):
        rng = random.Random(count)
        parts, produced = [], 0
        for _ in range(count - 1):
            ll = rng.randrange(0, 4) if produced else 3
            off = rng.randrange(1, min(produced + ll, 200) + 1)
            ml = rng.choice((4, 5, 9, 20, 33))
            parts.append((_rand(rng, ll), off, ml))
            produced += ll + ml
        parts.append((b"[end]", None, None))
        blk, content = build(parts)
        out.append((f"seqs{count}", blk, len(content), content))
    rng = random.Random(99)
    parts, produced = [], 0
    for i in range(2 * B):
        ll, ml = 3, 6
        off = rng.randrange(40, 60) if produced > 100 else produced + ll   # far back: before the batch, mostly
        if i in (0, B - 1, 2 * B - 1):
            off = 1                                    # a dependent match: it repeats its own last literal
        elif i == B:
            off, ml = ll + 3, 12                       # source: 3 bytes of the batch before, then this batch's literals
        elif i == B + 1:
            off = 2
        parts.append((_rand(rng, ll), off, ml))
        produced += ll + ml
    parts.append((b"[end]", None, None))
    blk, content = build(parts)
    out.append(("dependent_at_batch_ends", blk, len(content), content))
    return out


# ---------------------------------------------------------------- window edges
_PATTERN = [(b"ABCDEFGHIJKLMNOPQRST", 7, 30), (b"[end]", None, None)]   # token, ll ext, 20 literals, offset, ml ext: 25 bytes


def window_blocks():
    """[(name, block, size, content)]: the fixed pattern behind a leading literal run of every length
    that puts each of its fields -- token, extension byte, first and last literal, both offset bytes,
    match extension -- at, before and after an input offset k * W (k = 1, 2). The kernel's first window
    starts at the stream's first byte; it rebases the next one at the token after the last sequence
    walked, so a third family puts the pattern across the end of a rebased second window."""
    rng = random.Random(8)
    lead = _rand(rng, 2 * W + 64)
    out = []

    def add(name, parts):
        blk, content = build(parts)
        out.append((name, blk, len(content), content))
        return blk

    def lead_seq(target):
        """(literals, off, ml) of a leading sequence that encodes to exactly target bytes."""
        for ml in (4, 19):                                 # (ml 19 has an extension byte: one byte more)
            for L in range(target - 3 - target // 255 - 3, target):   # token, about L / 255 extension bytes, offset
                if L >= 5 and len(seq(lead[:L], 5, ml)) == target:
                    return lead[:L], 5, ml
        raise AssertionError(target)

    for k in (1, 2):
        for d in range(-2, 28):          # the pattern starts at k * W - d: its byte d is the first past the edge
            add(f"edge{k}W_d{d}", [lead_seq(k * W - d)] + _PATTERN)
    # a first sequence that ends past the first window: the second window starts at its successor's
    # token, rounded down to 16 bytes (the one-shot call's source is aligned)
    first = (lead[:W + 100], 9, 4)
    n_first = len(seq(*first))
    for d in range(-2, 28):
        add(f"edge_rebased_d{d}", [first, lead_seq(n_first // 16 * 16 + W - d - n_first)] + _PATTERN)
    return out


def valid_cases():
    """[(name, block, size, content or None)] of everything above."""
    return [(n, b, len(c), c) for n, b, c in corpus()] + hand_blocks() + batch_blocks() + window_blocks()


# ---------------------------------------------------------------- the host model (tests/native/pf_lz4_check.cpp)
def build_checker(tmp, root):
    """g++ build of the stand-alone host decoder under AddressSanitizer + UBSan."""
    import subprocess
    csrc = os.path.join(root, "parquet-floor_amd", "csrc")
    exe = os.path.join(str(tmp), "pf_lz4_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(root, "include"),
                    "-I", csrc, os.path.join(root, "tests", "native", "pf_lz4_check.cpp"), "-o", exe], check=True)
    return exe


def run_checker(exe, cases, tmp, tag):
    """cases = [(name, block, expected size)] -> [(status, bytes)]; a sanitizer report fails the run."""
    import subprocess
    src, dst = os.path.join(str(tmp), tag + ".cases"), os.path.join(str(tmp), tag + ".results")
    with open(src, "wb") as f:
        for _, blk, size in cases:
            f.write(struct.pack("<II", len(blk), size) + blk)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert f"cases {len(cases)} " in r.stdout, r.stdout
    blob, at, out = open(dst, "rb").read(), 0, []
    for _ in cases:
        st, n = struct.unpack_from("<iI", blob, at)
        out.append((st, blob[at + 8:at + 8 + n]))
        at += 8 + n
    return out


# ---------------------------------------------------------------- mutations
MUTATED = ("text300", "text5000", "random4k", "small_i32", "abc5000")
MUTANTS_PER_STREAM = 400


def mutants(streams):
    """[(name, bytes, expected size)]: seeded truncations, bit flips, 0x00 and 0xFF bytes of the
    MUTATED corpus streams (each <= 20 KB)."""
    by_name = {name: (b, c) for name, b, c in streams}
    out = []
    for si, name in enumerate(MUTATED):
        blk, c = by_name[name]
        assert len(blk) <= 20_000, name
        rng = random.Random(2000 + si)
        for k in range(MUTANTS_PER_STREAM):
            kind = k % 4
            # half of the hits in the first 64 bytes, where the first tokens and offsets lie
            at = rng.randrange(min(64, len(blk))) if rng.random() < 0.5 else rng.randrange(len(blk))
            m = bytearray(blk)
            if kind == 0:
                m = m[:max(1, at)]
            elif kind == 1:
                m[at] ^= 1 << rng.randrange(8)
            else:
                m[at] = 0x00 if kind == 2 else 0xFF
            out.append((f"{name}#{k}", bytes(m), len(c)))
    return out
