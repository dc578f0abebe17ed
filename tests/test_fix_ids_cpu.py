"""The id unpack of k_flat_fixed's eight-a-thread body (csrc/pf_fix_ids.h: 8 consecutive dictionary ids from a page's run
table and one contiguous load) checked without a GPU: tests/native/pf_fix_ids_check.cpp compares it with a per-entry,
bit-by-bit reference over id widths 0 to 32, every first-bit shift 0 to 7, groups inside a packed run, inside an RLE run
and straddling packed -> packed, packed -> RLE and RLE -> packed at every split 1 to 7, n = 1 to 8, a section that ends
0 to 24 bytes after the last id byte, sections 0 to 3 bytes off a word boundary, and tables of 1 and of RUN_CAP runs.
Which groups the routine calls fast is compared with the rule written out in the check, and its word loader aborts on a
word that is not wholly inside the id section. Host code only, built here with g++ under AddressSanitizer + UBSan as a
stand-alone program."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "parquet-floor_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fix_ids")
    exe = str(tmp / "pf_fix_ids_check")
    # the sanitizer runtimes linked in, so the program runs the same whatever else the loader brings first
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "pf_fix_ids_check.cpp"), "-o", exe], check=True)
    return exe


def test_ids8_matches_per_entry_reference_under_asan(checker):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([checker], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # 33 widths x (8 shifts x 23 run lists x 4 section offsets + 50 section ends + 1 full table) + 600 random lists
    assert r.stdout.startswith("cases 26571 ") and r.stdout.rstrip().endswith(" failures 0"), r.stdout
    # the fast path is what was compared: a third of the groups (n = 8 in one run, or RLE)
    assert int(r.stdout.split()[5]) > 300000, r.stdout
