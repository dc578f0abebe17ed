"""The host model of the ZSTD write route (compress_host, csrc/pf_zstd_enc_core.h): every frame it writes is read
back by libzstd and by the project's own decompress_host, under AddressSanitizer + UBSan in a stand-alone
program (tests/native/pf_zstd_enc_check.cpp). No GPU: k_zstd_compress is held to this model byte for byte in
test_gpu_zstd_compress.py, so what is proved here about the bytes holds for the kernel's."""
import pytest

import zstd_enc_cases as E
import zstd_frames as Z
from conftest import ROOT

# what the outputs must show between them (zstd_frames.census), besides the repeat codes counted by the model
MODES = {"block_raw", "block_rle", "block_compressed", "multi_block", "mixed_blocks", "lit_raw", "lit_rle", "huf_1", "huf_4",
         "weights_direct", "weights_fse", "no_sequences", "nseq_1byte", "nseq_2byte", "ll_predefined", "of_predefined",
         "ml_predefined", "fcs1_single", "fcs2_single", "fcs4_single"}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Every case through the sanitized checker, once: [(case, result)]. The checker itself compresses each
    input twice (status 1: the runs differ) and decodes the frame with decompress_host (status 2)."""
    tmp = tmp_path_factory.mktemp("zstd_enc")
    exe = E.build_checker(tmp, ROOT)
    cs = E.cases() + E.assembled()
    return list(zip(cs, E.run_checker(exe, cs, tmp, "enc")))


def test_frames_decode_to_the_input(run):
    """libzstd and decompress_host return the input exactly; two runs give the same bytes; no sanitizer report
    (run_checker fails on one)."""
    bad = []
    for case, r in run:
        if r["status"] != 0:
            bad.append((case[0], "status", r["status"]))
        elif Z.libzstd(r["frame"], len(case[1])) != case[1]:
            bad.append((case[0], "libzstd"))
    assert not bad, bad[:20]


def test_every_mode_is_written(run):
    seen, reps = set(), 0
    for _case, r in run:
        seen |= Z.census(r["frame"])
        reps += r["rep_codes"]
    assert MODES <= seen, sorted(MODES - seen)
    assert seen <= MODES, sorted(seen - MODES)   # nothing the route does not have: no window, checksum, per-block tables
    assert reps > 0
    by_name = {case[0]: r for case, r in run}
    # repeat codes in a block behind a raw block, and none in a job before its own first offset (a frame whose
    # repeat code came first would decode to other bytes: test_frames_decode_to_the_input)
    r = by_name[f"raw_then_repeats[:{4 * E.JOB}]"]
    assert r["raw"] == 1 and r["compressed"] == 3 and r["rep_codes"] > 0, r
    assert by_name["plain_i64_arith[:72000]"]["compressed"] == 9
    assert by_name["uniform[:70000]"]["raw"] == 9 and by_name["uniform[:70000]"]["compressed"] == 0
    assert by_name["one_byte[:70000]"]["rle"] == 9


def test_no_frame_is_longer_than_its_bound(run):
    """Frame header + 3 bytes per job + the input, whatever the input."""
    bad = [(case[0], len(r["frame"]), E.bound(len(case[1]))) for case, r in run if len(r["frame"]) > E.bound(len(case[1]))]
    assert not bad, bad


@pytest.mark.parametrize("name", ["iid64", "iid64_high"])
def test_six_bit_alphabets_shrink(run, name):
    """64 KiB of i.i.d. bytes over 64 symbols: 6 bits of entropy a byte and practically no 4-byte repeats in an
    8 KiB job, so Huffman literals alone give 0.75 plus tables and headers; the bound is 0.80. The alphabet
    192..255 has every symbol above 128: only FSE-compressed weights can describe its tree."""
    (case, r), = [(c, r) for c, r in run if c[0] == f"{name}[:65536]"]
    ratio = len(r["frame"]) / len(case[1])
    print(name, len(r["frame"]), ratio)
    assert ratio <= 0.80, ratio
    if name == "iid64_high":
        assert "weights_fse" in Z.census(r["frame"])
