"""The LZ4 decode core (csrc/pf_lz4_core.h) checked on the CPU: tests/native/pf_lz4_check.cpp runs
the host model, built with g++ under AddressSanitizer + UBSan, over the corpus, the hand-assembled
blocks, the batch- and window-edge streams and 2,000 seeded mutants, and has to give the verdict and
the bytes of the Python model (lz4_blocks.model); the model in turn is compared with liblz4. No GPU."""
import ctypes
import ctypes.util

import pyarrow as pa
import pytest

import lz4_blocks as L
from conftest import ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return L.build_checker(tmp_path_factory.mktemp("lz4"), ROOT)


@pytest.fixture(scope="module")
def streams():
    return L.corpus()


@pytest.fixture(scope="module")
def muts(streams):
    """[(name, block, size, the model's bytes or None, met an offset 0)]"""
    out = []
    for name, m, size in L.mutants(streams):
        why = []
        out.append((name, m, size, L.model(m, size, why), why == ["offset 0"]))
    return out


def test_helper_constants_are_the_kernels():
    """The batch and window edges the streams are built around are the ones k_lz4 is compiled with."""
    k = L.kernel_constants(ROOT)
    assert (k["LZ4_BATCH"], k["LZ4_WINDOW"]) == (L.B, L.W)
    text = open(f"{ROOT}/parquet-floor_amd/csrc/pf_lz4.hip").read()
    assert "sq[LZ4_BATCH]" in text and "win[LZ4_WINDOW]" in text


def test_model_gives_the_written_expectations(streams):
    """Corpus: the input; hand, batch and window blocks: the bytes of the builder's own byte-by-byte
    expansion, or a refusal where the block was built to be refused."""
    cases = L.valid_cases()
    assert {"tail4", "off0", "off_one_more", "off65535", "ends_after_match", "two_literal_only", "00", "empty_input",
            f"seqs{L.B - 1}", f"seqs{2 * L.B + 1}", "edge1W_d0", "edge2W_d27", "edge_rebased_d0"} <= {c[0] for c in cases}
    bad = [n for n, b, size, c in cases if L.model(b, size) != c]
    assert not bad, bad
    assert sum(c is None for *_, c in cases) >= 10


def test_corpus_decodes_to_its_input_and_pyarrow_agrees(streams):
    codec = pa.Codec("lz4_raw")
    for name, b, c in streams:
        assert L.model(b, len(c)) == c, name
        assert codec.decompress(b, decompressed_size=len(c), asbytes=True) == c, name
    assert dict((n, b) for n, b, _ in streams)["empty"] == b"\x00"
    random4k = dict((n, b) for n, b, _ in streams)["random4k"]
    assert random4k[0] >> 4 == 15 and random4k[1:17] == b"\xff" * 16      # a literal length of many 255s


def test_core_gives_the_models_verdict_under_sanitizers(checker, muts, tmp_path):
    cases = [(n, b, size, c) for n, b, size, c in L.valid_cases()] + [(n, b, size, c) for n, b, size, c, _ in muts]
    for name, b, size, c in list(cases):                # one byte less and one more than each accepted block produces
        if c is not None and not name.count("#"):
            cases.append((name + "-1", b, size - 1, None) if size else (name + "+2", b, size + 2, None))
            cases.append((name + "+1", b, size + 1, None))
    got = L.run_checker(checker, [(n, b, size) for n, b, size, _ in cases], tmp_path, "all")   # sanitizer-clean, or this fails
    bad = []
    for (name, _, _, c), (st, out) in zip(cases, got):
        if st not in (0, -2) or (st == 0) != (c is not None) or (st == 0 and out != c):
            bad.append((name, st))
    assert not bad, bad[:20]


def test_model_against_liblz4(muts):
    """LZ4_decompress_safe with capacity = size; accepted = it returns size. Over the mutants whose walk
    meets no offset 0 (liblz4 1.9.3 accepts that and copies unspecified bytes) verdicts and bytes are equal."""
    path = ctypes.util.find_library("lz4")
    if not path:
        pytest.skip("no liblz4 on this machine")
    lib = ctypes.CDLL(path)
    lib.LZ4_decompress_safe.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.LZ4_decompress_safe.restype = ctypes.c_int
    both, neither, left_out, wrong = 0, 0, 0, []
    for name, m, size, c, off0 in muts:
        if off0:
            left_out += 1
            continue
        dst = ctypes.create_string_buffer(max(size, 1))
        ref = dst.raw[:size] if lib.LZ4_decompress_safe(m, dst, len(m), size) == size else None
        if ref != c:
            wrong.append((name, "liblz4 " + ("accepts" if ref is not None else "refuses"), "model " + ("accepts" if c is not None else "refuses")))
        both += ref is not None and c is not None
        neither += ref is None and c is None
    print(f"mutants {len(muts)}: both accept {both}, both refuse {neither}, left out (offset 0) {left_out}, differ {len(wrong)}")
    assert len(muts) == 2000
    assert not wrong, wrong[:20]
    assert left_out <= len(muts) // 10
    assert both >= len(muts) // 4 and neither >= len(muts) // 4
