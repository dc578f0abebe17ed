"""The id unpack of k_flat_dstr (csrc/pf_dstr_ids.h: 16 consecutive dictionary ids from a page's run table) checked
without a GPU: tests/native/pf_dstr_ids_check.cpp compares it entry by entry with a per-entry, bit-by-bit reference
over id widths 0 to 32, all-packed, all-RLE and alternating 8-value RLE / 8-value packed run lists, a run boundary at
every position within the 16 between every pair of run kinds, two boundaries within one group, last partial groups,
streams that end inside the last packed run, and frames that start 0 to 15 bytes before the stream. The word loader
of the check aborts on a word outside what the routine's contract allows. Host code only, built here with g++ under
AddressSanitizer + UBSan as a stand-alone program."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "parquet-floor_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dstr_ids")
    exe = str(tmp / "pf_dstr_ids_check")
    # the sanitizer runtimes linked in, so the program runs the same whatever else the loader brings first
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "pf_dstr_ids_check.cpp"), "-o", exe], check=True)
    return exe


def test_ids16_matches_per_entry_reference_under_asan(checker):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([checker], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # 33 widths x 110 run lists x (4 frame shifts + 1 truncated stream) + 400 random lists
    assert r.stdout.startswith("cases 18550 ") and r.stdout.rstrip().endswith(" failures 0"), r.stdout
