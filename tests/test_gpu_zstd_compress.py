"""k_zstd_compress (csrc/pf_zstd_enc.hip) through pf_zstd_compress: the kernel's frames equal the host model's
(compress_host, csrc/pf_zstd_enc_core.h) byte for byte over every case of zstd_enc_cases.py, libzstd and this
library's own GPU decoder (k_zstd) read them back to the input, and a short destination is PF_ERR_CAPACITY.
test_zstd_enc_core.py checks the model itself on the CPU, under sanitizers."""
import pytest

import zstd_enc_cases as E
import zstd_frames as Z
from conftest import ROOT

pytestmark = pytest.mark.gpu

PF_ERR_CAPACITY = -6


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def frames(decoder, tmp_path_factory):
    """[(name, input, the host model's frame, the kernel's frame)], each computed once."""
    tmp = tmp_path_factory.mktemp("zstd_enc_gpu")
    cs = E.cases()
    host = E.run_checker(E.build_checker(tmp, ROOT, sanitize=False), cs, tmp, "enc")
    return [(name, data, h["frame"] if h["status"] == 0 else None, decoder.zstd_compress(data)) for (name, data), h in zip(cs, host)]


def test_kernel_equals_the_host_model(frames):
    bad = []
    for name, data, want, got in frames:
        if want is None or got != want:
            where = "status" if not isinstance(got, bytes) or want is None else next(
                (i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            bad.append((name, len(data), got if isinstance(got, int) else len(got), None if want is None else len(want), where))
    assert not bad, bad[:20]


def test_libzstd_reads_the_kernels_frames(frames):
    bad = [name for name, data, _want, got in frames if not isinstance(got, bytes) or Z.libzstd(got, len(data)) != data]
    assert not bad, bad[:20]


def test_k_zstd_reads_the_kernels_frames(decoder, frames):
    bad = [name for name, data, _want, got in frames if not isinstance(got, bytes) or decoder.zstd_decompress(got, len(data)) != data]
    assert not bad, bad[:20]


def test_destination_one_byte_short(decoder, frames):
    for want_name in ("text70000[:16384]", f"uniform[:{E.JOB + 1}]", "zeros[:0]"):
        (data, got), = [(d, g) for name, d, _w, g in frames if name == want_name]
        assert decoder.zstd_compress(data, cap=len(got)) == got
        assert decoder.zstd_compress(data, cap=len(got) - 1) == PF_ERR_CAPACITY
