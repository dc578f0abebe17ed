"""k_zstd (csrc/pf_zstd.hip) through pf_zstd_decompress: every corpus and hand-assembled frame of
zstd_frames.py bit-exact, and every seeded mutant with the host core's verdict -- its status and,
when 0, its bytes. The mutants are damaged on purpose, so the host model runs over them first,
under AddressSanitizer + UBSan (tests/native/pf_zstd_check.cpp): what the GPU sees has passed the
same bounds checks, in the same code, on the host."""
import pytest

import zstd_frames as Z
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def corpus():
    return Z.corpus_frames()


def test_frames_bit_exact(decoder, corpus):
    bad = []
    for name, f, c in corpus + Z.hand_frames():
        got = decoder.zstd_decompress(f, len(c))
        if got != c:
            bad.append((name, got if isinstance(got, int) else "bytes differ"))
    assert not bad, bad


def test_short_and_long_destination(decoder, corpus):
    """The expected size is part of the verdict: one byte less or more is -2, never a write past it."""
    name, f, c = next(x for x in corpus if x[0] == "text5000@3")
    assert decoder.zstd_decompress(f, len(c) - 1) == -2
    assert decoder.zstd_decompress(f, len(c) + 1) == -2
    assert decoder.zstd_decompress(b"", 0) == b""


def test_mutants_get_the_host_cores_verdict(decoder, corpus, tmp_path):
    muts = Z.mutants(corpus)
    exe = Z.build_checker(tmp_path, ROOT)
    host = Z.run_checker(exe, muts, tmp_path, "mutants")   # sanitizer-clean on the host first
    bad = []
    for (name, m, size), (st, b) in zip(muts, host):
        got = decoder.zstd_decompress(m, size)
        want = b if st == 0 else st
        if got != want:
            bad.append((name, st, got if isinstance(got, int) else "bytes"))
    assert not bad, bad[:20]
