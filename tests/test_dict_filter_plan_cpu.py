"""The host side of windows and predicates over kept dictionaries (pf_decode_row_group_dict_filter: csrc/pf_plan.cpp,
csrc/pf_result.cpp, csrc/pf_pred.h), without a GPU: tests/native/pf_dict_filter_check.cpp checks that a batch without a
predicate on a kept chunk plans and lays out its filter stage field for field as before, the match bitmaps' word counts
and offsets at the word and tile edges and that no region of the stage's buffer overlaps another, the index width in the
window's and the selection's view of assemble_info, the call errors, and pred_range_at over dictionary entries against
a brute-force loop for every RANGE-able type. Built here with g++ under ASan + UBSan."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "parquet-floor_amd", "csrc")


def test_dict_filter_plan_under_asan(tmp_path):
    exe = str(tmp_path / "pf_dict_filter_check")
    subprocess.run(["g++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "pf_dict_filter_check.cpp"),
                    os.path.join(CSRC, "pf_plan.cpp"), os.path.join(CSRC, "pf_result.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "failures 0" in r.stdout
