"""Inputs of the ZSTD write route (csrc/pf_zstd_enc_core.h, k_zstd_compress) and the runner of its host
model (tests/native/pf_zstd_enc_check.cpp). No GPU. test_zstd_enc_core.py checks the model against
libzstd under sanitizers; test_gpu_zstd_compress.py holds the kernel to the model byte for byte."""
import os
import struct
import subprocess

import numpy as np

import zstd_frames as Z

JOB = 8192                      # ZC_BLOCK (pf_enc_tables.h)
CUTS = (0, 1, 2, 3, 4, 5, 8191, 8192, 8193, 16384, 65537)


def _bitpack7(ids):
    bits = ((ids[:, None] >> np.arange(7)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little").tobytes()


def base_inputs():
    """name -> bytes, in a fixed order."""
    rng = np.random.default_rng(2024)
    out = dict(Z.corpus_inputs())
    out["one_byte"] = b"\xa7" * 70_000
    out["two_bytes"] = b"\x00\xff" * 35_000
    out["uniform"] = rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes()
    low = rng.integers(0, 64, 65536, dtype=np.uint8)
    out["iid64"] = low.tobytes()
    out["iid64_high"] = (low + 192).astype(np.uint8).tobytes()
    out["plain_i64_arith"] = (1_000_000 + 37 * np.arange(9000, dtype=np.int64)).tobytes()
    out["ids_w7"] = _bitpack7(rng.zipf(1.4, 80_000).astype(np.int64) % 128)
    # the first job raw (random bytes), the later ones repetitive (prices with two decimals: the same offset comes
    # back with literals in between): repeat codes in a block after a raw one
    prices = np.round(rng.normal(100.0, 20.0, 3 * JOB // 8), 2).astype(np.float64).tobytes()
    out["raw_then_repeats"] = rng.integers(0, 256, JOB, dtype=np.uint8).tobytes() + prices
    # >= 128 sequences in one job: short random records, each repeated at once
    rec = rng.integers(0, 256, (400, 9), dtype=np.uint8)
    out["many_sequences"] = np.repeat(rec, 2, axis=0).tobytes()
    # a skewed alphabet whose plain Huffman tree is deeper than 11: the length limit and its repair
    skew = np.concatenate([np.full(max(1, 4000 >> k), k, np.uint8) for k in range(20)])
    out["skewed"] = rng.permutation(skew).tobytes()
    return out


def cases():
    """[(name, bytes)]: every input whole and cut to CUTS (cuts beyond its length, and whole inputs over
    300 KB cut again to one length, are left out)."""
    out, seen = [], set()
    for name, data in base_inputs().items():
        for n in (len(data),) + CUTS:
            if n > len(data) or (name, n) in seen:
                continue
            seen.add((name, n))
            out.append((f"{name}[:{n}]", data[:n]))
    return out


def assembled():
    """[(name, content, literals, [(ll, ml, offset)])] for the block assembler alone. Every job of compress_host
    starts without history, so each byte value's first occurrence in it is a literal: a job with one distinct
    literal has one distinct byte and is an RLE block. RLE literals are therefore reachable only with sequences
    that a caller hands to the assembler, as here (offsets past the literal they follow are what the kernel's
    match finder never produces; the format allows them within the frame)."""
    out = []
    lits, seqs = b"z" * 40, [(20, 50, 1), (19, 30, 5)]
    out.append(("rle_literals", Z.lz77(lits, seqs), lits, seqs))
    lits, seqs = bytes(range(1, 9)) * 4, [(8, 8, 8), (8, 8, 8), (8, 4, 16)]
    out.append(("raw_literals_repeat", Z.lz77(lits, seqs), lits, seqs))
    return out


def bound(n):
    """Frame header + one 3-byte block header per job + the input: no frame may be longer."""
    hdr = 6 if n < 256 else (7 if n < 65536 + 256 else 9)
    return hdr + 3 * max(1, -(-n // JOB)) + n


def build_checker(tmp, root, sanitize=True):
    """g++ build of the stand-alone host encoder (with the host decoder behind it)."""
    csrc = os.path.join(root, "parquet-floor_amd", "csrc")
    exe = os.path.join(str(tmp), "pf_zstd_enc_check")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", *san, "-I", os.path.join(root, "include"), "-I", csrc,
                    os.path.join(root, "tests", "native", "pf_zstd_enc_check.cpp"), "-o", exe], check=True)
    return exe


def run_checker(exe, inputs, tmp, tag):
    """inputs = [(name, bytes)] or assembled() entries -> [dict(status, frame, rep_codes, raw, rle, compressed)];
    a sanitizer report fails the run."""
    src, dst = os.path.join(str(tmp), tag + ".cases"), os.path.join(str(tmp), tag + ".results")
    with open(src, "wb") as f:
        for case in inputs:
            data = case[1]
            f.write(struct.pack("<II", len(case) > 2, len(data)) + data)
            if len(case) > 2:
                f.write(struct.pack("<I", len(case[2])) + case[2] + struct.pack("<I", len(case[3])))
                for ll, ml, off in case[3]:
                    f.write(struct.pack("<HHH", ll, ml, off))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert f"cases {len(inputs)} " in r.stdout, r.stdout
    blob, at, out = open(dst, "rb").read(), 0, []
    for _ in inputs:
        st, n, reps, raw, rle, comp = struct.unpack_from("<iIIIII", blob, at)
        out.append(dict(status=st, frame=blob[at + 24:at + 24 + n], rep_codes=reps, raw=raw, rle=rle, compressed=comp))
        at += 24 + n
    return out
