"""k_lz4 (csrc/pf_lz4.hip) through pf_lz4_decompress: every corpus stream, hand-assembled block and
batch- and window-edge stream of lz4_blocks.py bit-exact or refused as built, and every seeded mutant
with the host core's verdict -- its status and, when 0, its bytes. The mutants are damaged on
purpose, so the host model runs over them first, under AddressSanitizer + UBSan
(tests/native/pf_lz4_check.cpp): what the GPU sees has passed the same bounds checks, in the same
code, on the host."""
import pytest

import lz4_blocks as L
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def streams():
    return L.corpus()


def test_blocks_bit_exact(decoder):
    bad = []
    for name, b, size, c in L.valid_cases():
        got = decoder.lz4_decompress(b, size)
        if got != (c if c is not None else -2):
            bad.append((name, got if isinstance(got, int) else "bytes differ"))
    assert not bad, bad


def test_short_and_long_destination(decoder, streams):
    """The expected size is part of the verdict: one byte less or more is -2, never a write past it."""
    for name in ("text5000", "zeros", "random4k", "abc5000"):
        b, c = next((b, c) for n, b, c in streams if n == name)
        assert decoder.lz4_decompress(b, len(c)) == c, name
        assert decoder.lz4_decompress(b, len(c) - 1) == -2, name
        assert decoder.lz4_decompress(b, len(c) + 1) == -2, name
    assert decoder.lz4_decompress(b"\x00", 0) == b""
    assert decoder.lz4_decompress(b"", 0) == -2


def test_mutants_get_the_host_cores_verdict(decoder, streams, tmp_path):
    muts = L.mutants(streams)
    exe = L.build_checker(tmp_path, ROOT)
    host = L.run_checker(exe, muts, tmp_path, "mutants")   # sanitizer-clean on the host first
    bad = []
    for (name, m, size), (st, b) in zip(muts, host):
        got = decoder.lz4_decompress(m, size)
        want = b if st == 0 else st
        if got != want:
            bad.append((name, st, got if isinstance(got, int) else "bytes"))
    assert not bad, bad[:20]
