"""The ZSTD decode core (csrc/pf_zstd_core.h) checked on the CPU against libzstd (pyarrow's codec):
tests/native/pf_zstd_check.cpp runs the host model, built with g++ under AddressSanitizer + UBSan,
over the corpus, the hand-assembled frames and seeded mutations of six frames. No GPU."""
import pytest

import zstd_frames as Z
from conftest import ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return Z.build_checker(tmp_path_factory.mktemp("zstd"), ROOT)


@pytest.fixture(scope="module")
def corpus():
    return Z.corpus_frames()


def test_corpus_shows_every_mode(corpus):
    seen = set()
    for _, f, _ in corpus:
        seen |= Z.census(f)
    assert not Z.CORPUS_MODES - seen, f"libzstd no longer writes {sorted(Z.CORPUS_MODES - seen)}: add an input"


def test_hand_frames_are_what_libzstd_reads():
    seen = set()
    for name, f, c in Z.hand_frames():
        assert Z.libzstd(f, len(c)) == c, name
        seen |= Z.census(f)
    assert {"lit_rle", "no_sequences", "nseq_3byte", "ll_rle", "of_rle", "ml_rle", "checksum", "skippable", "fcs0_window",
            "fcs8_single", "fcs4_window"} <= seen
    assert Z.xxh64(b"") == 0xEF46DB3751D8E999 and Z.xxh64(b"a") == 0xD24EC4F1A98C6E5B


def test_core_decodes_corpus_and_hand_frames(checker, corpus, tmp_path):
    cases = corpus + Z.hand_frames()
    got = Z.run_checker(checker, [(n, f, len(c)) for n, f, c in cases], tmp_path, "valid")
    bad = [n for (n, _, c), (st, b) in zip(cases, got) if st != 0 or b != c]
    assert not bad, bad


def test_mutants_run_clean_and_agree_with_libzstd(checker, corpus, tmp_path):
    """Hard conditions per mutant: status 0 or -2; where both accept, equal bytes; whatever libzstd
    accepts at the expected length, the core accepts. What only the core accepts is printed.

    Measured with pyarrow 25.0.0's libzstd: 1500 mutants run sanitizer-clean, both accept 626, only
    the core accepts 6, none misses a condition. 83 of them hold only because the core follows
    libzstd where a Huffman stream is not used up exactly; RFC 8878's own rule
    refuses all 83, which libzstd accepts."""
    muts = Z.mutants(corpus)
    assert len(muts) == 1500
    got = Z.run_checker(checker, muts, tmp_path, "mutants")   # sanitizer-clean, or this fails
    only_core, both, wrong = [], 0, []
    for (name, m, size), (st, b) in zip(muts, got):
        ref = Z.libzstd(m, size)
        if st not in (0, -2):
            wrong.append((name, "status", st))
        elif ref is not None and st != 0:
            wrong.append((name, "libzstd accepts, core rejects"))
        elif ref is not None and b != ref:
            wrong.append((name, "bytes differ"))
        elif ref is None and st == 0:
            only_core.append(name)
        both += ref is not None and st == 0
    print(f"mutants {len(muts)}: both accept {both}, only the core accepts {len(only_core)}: {only_core}")
    assert not wrong, wrong[:20]
