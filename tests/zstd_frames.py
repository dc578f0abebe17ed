"""ZSTD test material (RFC 8878): the corpus libzstd compresses for us, a census of the header modes
its frames use, a hand-assembler for the frames it never writes, an LZ77 executor for their
expected bytes, XXH64 for the content checksum, and the seeded mutations. No GPU, no native code."""
import random
import struct

import numpy as np
import pyarrow as pa

LEVELS = (-5, 1, 3, 9, 19)
MAGIC = 0xFD2FB528


# ---------------------------------------------------------------- corpus
def _text(n, seed=7):
    rng = np.random.default_rng(seed)
    vocab = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(k))) for k in rng.integers(2, 10, 2000)]
    words, size = [], 0
    ids = rng.zipf(1.3, n // 3 + 8) % len(vocab)
    for i in ids:
        words.append(vocab[int(i)])
        size += len(vocab[int(i)]) + 1
        if size >= n:
            break
    return " ".join(words).encode()[:n]


def corpus_inputs():
    """name -> bytes, in a fixed order."""
    rng = np.random.default_rng(11)
    out = {}
    for n in (1, 20, 300, 5000, 70000, 1_100_000):
        out[f"text{n}"] = _text(n)
    out["zeros"] = bytes(200_000)
    out["random"] = rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes()
    out["bits01"] = rng.integers(0, 2, 50_000, dtype=np.uint8).tobytes()
    out["sorted_i64"] = np.cumsum(rng.integers(1, 1000, 20_000)).astype(np.int64).tobytes()
    out["small_i32"] = rng.integers(0, 50, 20_000).astype(np.int32).tobytes()
    out["doubles"] = np.round(rng.normal(100.0, 20.0, 20_000), 2).astype(np.float64).tobytes()
    rec = rng.integers(0, 256, (3000, 8), dtype=np.uint8)
    out["records_twice"] = np.repeat(rec, 2, axis=0).tobytes()
    five = bytes(rng.integers(1, 256, 5, dtype=np.uint8))
    out["no_seq"] = bytes(3) + five + five   # (this libzstd stores it raw; flat48 below has the block without sequences)
    # (added until the census found every mode: ML RLE, and a compressed block without sequences)
    rec5 = np.random.default_rng(14).integers(0, 256, (300, 5), dtype=np.uint8)
    out["records5_twice"] = np.repeat(rec5, 2, axis=0).tobytes()
    out["flat48"] = np.random.default_rng(13).integers(0, 48, 1000, dtype=np.uint8).tobytes()
    out["mixed"] = _text(150_000, 8) + bytes(140_000) + rng.integers(0, 256, 140_000, dtype=np.uint8).tobytes() + _text(150_000, 9)
    return out


def corpus_frames():
    """[(name, frame, content)] for every input at every level (no_seq: level 1 only)."""
    frames = []
    for name, data in corpus_inputs().items():
        for lv in ((1,) if name == "no_seq" else LEVELS):
            frames.append((f"{name}@{lv}", pa.Codec("zstd", lv).compress(data, asbytes=True), data))
    return frames


def libzstd(frame, size):
    """pyarrow's verdict: the bytes, or None when libzstd refuses or produces another length."""
    try:
        return pa.Codec("zstd").decompress(frame, decompressed_size=size, asbytes=True)
    except Exception:
        return None


# ---------------------------------------------------------------- census (header parse only)
def census(frame):
    """The set of mode names a frame's headers show."""
    seen, at, n = set(), 0, len(frame)
    while at < n:
        magic = struct.unpack_from("<I", frame, at)[0]
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            at += 8 + struct.unpack_from("<I", frame, at + 4)[0]
            seen.add("skippable")
            continue
        assert magic == MAGIC
        d = frame[at + 4]
        at += 5
        single, fcs_flag = (d >> 5) & 1, d >> 6
        if not single:
            at += 1
        at += (0, 1, 2, 4)[d & 3]
        fcs_len = (single, 2, 4, 8)[fcs_flag]
        at += fcs_len
        seen.add(f"fcs{fcs_len}_{'single' if single else 'window'}")
        if d & 4:
            seen.add("checksum")
        blocks = []
        while True:
            v = frame[at] | frame[at + 1] << 8 | frame[at + 2] << 16
            at += 3
            last, bt, size = v & 1, (v >> 1) & 3, v >> 3
            blocks.append(bt)
            seen.add(("block_raw", "block_rle", "block_compressed")[bt])
            if bt == 2:
                _census_block(frame[at:at + size], seen)
            at += 1 if bt == 1 else size
            if last:
                break
        if len(blocks) > 1:
            seen.add("multi_block")
        if len(set(blocks)) > 1:
            seen.add("mixed_blocks")
        if d & 4:
            at += 4
    return seen


def _census_block(b, seen):
    t, sf = b[0] & 3, (b[0] >> 2) & 3
    if t < 2:
        hdr = (1, 2, 1, 3)[sf]
        regen = b[0] >> 3 if hdr == 1 else (int.from_bytes(b[:hdr], "little") >> 4)
        at = hdr + (regen if t == 0 else 1)
        seen.add(("lit_raw", "lit_rle")[t])
    else:
        hdr, w = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        v = int.from_bytes(b[:hdr], "little")
        csize = (v >> (4 + w)) & ((1 << w) - 1)
        streams = 1 if sf == 0 else 4
        seen.add(f"{'huf' if t == 2 else 'treeless'}_{streams}")
        if t == 2:
            seen.add("weights_fse" if b[hdr] < 128 else "weights_direct")
        at = hdr + csize
    ns = b[at]
    if ns == 0:
        seen.add("no_sequences")
        return
    form = 1 if ns < 128 else (3 if ns == 255 else 2)
    seen.add(f"nseq_{form}byte")
    modes = b[at + form]
    for name, sh in (("ll", 6), ("of", 4), ("ml", 2)):
        seen.add(f"{name}_{('predefined', 'rle', 'compressed', 'repeat')[(modes >> sh) & 3]}")


# what the corpus must show (observed with pyarrow 25.0.0's libzstd; the test fails if one goes missing)
CORPUS_MODES = {
    "multi_block", "treeless_4", "weights_fse", "ml_repeat", "huf_1", "block_rle", "block_raw", "weights_direct",
    "of_rle", "treeless_1", "ll_rle", "of_repeat", "ll_repeat", "ml_rle", "no_sequences", "mixed_blocks",
    "fcs1_single", "fcs2_single", "fcs4_single", "fcs4_window", "huf_4", "block_compressed",
}


# ---------------------------------------------------------------- XXH64
_P1, _P2, _P3, _P4, _P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
_M = (1 << 64) - 1


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _round(acc, v):
    return (_rotl((acc + v * _P2) & _M, 31) * _P1) & _M


def _merge(h, v):
    return ((h ^ _round(0, v)) * _P1 + _P4) & _M


def xxh64(data, seed=0):
    n, at = len(data), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M]
        while at + 32 <= n:
            for k, x in enumerate(struct.unpack_from("<4Q", data, at)):
                v[k] = _round(v[k], x)
            at += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for x in v:
            h = _merge(h, x)
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while at + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", data, at)[0]), 27) * _P1 + _P4) & _M
        at += 8
    if at + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", data, at)[0] * _P1 & _M), 23) * _P2 + _P3) & _M
        at += 4
    while at < n:
        h = (_rotl(h ^ (data[at] * _P5 & _M), 11) * _P1) & _M
        at += 1
    h ^= h >> 33
    h = (h * _P2) & _M
    h ^= h >> 29
    h = (h * _P3) & _M
    return h ^ (h >> 32)


# ---------------------------------------------------------------- hand assembler
def block(btype, payload, last, size=None):
    """A block: 0 raw (payload = bytes), 1 RLE (payload = one byte, size = repeat), 2 compressed."""
    size = len(payload) if size is None else size
    return struct.pack("<I", (size << 3) | (btype << 1) | int(last))[:3] + payload


def frame(blocks, content_size, fcs_len=None, window=None, checksum=None):
    """fcs_len 0 / 1 / 2 / 4 / 8 (None: the narrowest); window: a Window_Descriptor byte (else
    single segment); checksum: the content, to append the low 32 bits of its XXH64."""
    if fcs_len is None:
        fcs_len = 1 if content_size < 256 else (2 if content_size < 65792 else 4)
    single = window is None
    assert fcs_len or not single
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_len]
    d = flag << 6 | int(single) << 5 | (4 if checksum is not None else 0)
    out = struct.pack("<IB", MAGIC, d)
    if not single:
        out += bytes([window])
    if fcs_len:
        out += (content_size - (256 if fcs_len == 2 else 0)).to_bytes(fcs_len, "little")
    out += b"".join(blocks)
    if checksum is not None:
        out += struct.pack("<I", xxh64(checksum) & 0xFFFFFFFF)
    return out


def raw_literals(lits):
    n = len(lits)
    if n < 32:
        return bytes([n << 3]) + lits
    if n < 4096:
        return struct.pack("<H", (n << 4) | 4) + lits
    return struct.pack("<I", (n << 4) | 12)[:3] + lits


def back_bits(fields):
    """A backward bitstream from (value, nbits) pairs in the order the decoder reads them."""
    acc = nb = 0
    for v, k in reversed(fields):
        acc |= (v & ((1 << k) - 1)) << nb
        nb += k
    acc |= 1 << nb   # end mark
    return acc.to_bytes(nb // 8 + 1, "little")


def lz77(literals, seqs):
    """Expected bytes of one block: seqs = [(ll, ml, offset)], the literals left over appended."""
    out, lp = bytearray(), 0
    for ll, ml, off in seqs:
        out += literals[lp:lp + ll]
        lp += ll
        assert 0 < off <= len(out)
        for _ in range(ml):
            out.append(out[-off])
    out += literals[lp:]
    return bytes(out)


def hand_frames():
    """[(name, frame, content)]: what the corpus does not produce."""
    rng = random.Random(5)
    out = []
    # RLE literals, zero sequences
    out.append(("rle_literals_no_seq", frame([block(2, bytes([(29 << 3) | 1, 0x5A, 0x00]), True)], 29), b"\x5A" * 29))
    # all three modes RLE, 32,600 sequences of LL 1 / ML 3 / OF code 2 (+ two extra bits): the count in
    # its 3-byte form, and a bitstream of extra bits only
    nseq = 32600
    lits = bytes(rng.randrange(256) for _ in range(nseq + 7))
    seqs, produced = [], 0
    for _ in range(nseq):
        off = rng.randint(1, min(4, produced + 1))
        seqs.append((1, 3, off))
        produced += 4
    sec = bytes([0xFF]) + struct.pack("<H", nseq - 0x7F00) + bytes([1 << 6 | 1 << 4 | 1 << 2, 1, 2, 0])
    sec += back_bits([(off + 3 - 4, 2) for _, _, off in seqs])
    content = lz77(lits, seqs)
    out.append(("all_rle_32600_seq", frame([block(2, raw_literals(lits) + sec, True)], len(content)), content))
    text = _text(3000, 21)
    out.append(("checksum", frame([block(0, text, True)], len(text), checksum=text), text))
    a, b = _text(700, 22), _text(90, 23)
    out.append(("two_frames", frame([block(0, a, True)], len(a)) + frame([block(1, b"Q", True, size=333)], 333), a + b"Q" * 333))
    out.append(("skippable_then_frame", struct.pack("<II", 0x184D2A53, 11) + bytes(range(11)) + frame([block(0, b, True)], len(b)), b))
    out.append(("empty_frame", frame([block(0, b"", True)], 0), b""))
    out.append(("raw_blocks_window", frame([block(0, a[:400], False), block(0, a[400:], True)], len(a), fcs_len=4, window=0x08), a))
    out.append(("no_fcs_window", frame([block(0, a, False), block(1, b"z", True, size=50)], 0, fcs_len=0, window=0x00), a + b"z" * 50))
    out.append(("fcs8", frame([block(0, b, True)], len(b), fcs_len=8), b))
    return out


# ---------------------------------------------------------------- the host model (tests/native/pf_zstd_check.cpp)
def build_checker(tmp, root):
    """g++ build of the stand-alone host decoder under AddressSanitizer + UBSan."""
    import os
    import subprocess
    csrc = os.path.join(root, "parquet-floor_amd", "csrc")
    exe = os.path.join(str(tmp), "pf_zstd_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(root, "include"),
                    "-I", csrc, os.path.join(root, "tests", "native", "pf_zstd_check.cpp"), "-o", exe], check=True)
    return exe


def run_checker(exe, cases, tmp, tag):
    """cases = [(name, frame, expected size)] -> [(status, bytes)]; a sanitizer report fails the run."""
    import os
    import subprocess
    src, dst = os.path.join(str(tmp), tag + ".cases"), os.path.join(str(tmp), tag + ".results")
    with open(src, "wb") as f:
        for _, fr, size in cases:
            f.write(struct.pack("<II", len(fr), size) + fr)
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
MUTATED = ("text300@3", "text5000@3", "text70000@19", "bits01@3", "small_i32@19", "records5_twice@19")
MUTANTS_PER_FRAME = 250


def mutants(frames):
    """[(name, bytes, expected size)]: seeded truncations, bit flips, 0x00 and 0xFF bytes of the
    MUTATED corpus frames (each <= 20 KB, no checksum)."""
    by_name = {name: (f, c) for name, f, c in frames}
    out = []
    for fi, name in enumerate(MUTATED):
        f, c = by_name[name]
        assert len(f) <= 20_000 and not f[4] & 4, name
        rng = random.Random(1000 + fi)
        for k in range(MUTANTS_PER_FRAME):
            kind = k % 4
            # half of the hits in the first 64 bytes, where the headers and table descriptions lie
            at = rng.randrange(min(64, len(f))) if rng.random() < 0.5 else rng.randrange(len(f))
            m = bytearray(f)
            if kind == 0:
                m = m[:max(1, at)]
            elif kind == 1:
                m[at] ^= 1 << rng.randrange(8)
            else:
                m[at] = 0x00 if kind == 2 else 0xFF
            out.append((f"{name}#{k}", bytes(m), len(c)))
    return out
