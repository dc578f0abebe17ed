"""The decode's host-only result side (csrc/pf_result.cpp) checked without a GPU: tests/native/pf_result_check.cpp
drives the side-table layouts, the arena and chars-rerun decisions, the merge of the decode's, the window's and the
selection's view into pf_column_info, and the batch-copy layout with hand-made tables and hand-written expected
values. Host code only, built here with g++ under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "parquet-floor_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("result")
    gxx = ["g++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", CSRC]
    srcs = [os.path.join(ROOT, "tests", "native", "pf_result_check.cpp"), os.path.join(CSRC, "pf_result.cpp")]
    objs = [str(tmp / (os.path.basename(s) + ".o")) for s in srcs]
    procs = [subprocess.Popen(gxx + ["-c", s, "-o", o]) for s, o in zip(srcs, objs)]
    assert [p.wait() for p in procs] == [0] * len(procs)
    # the sanitizer runtimes linked in, so the program runs the same whatever else the loader brings first
    subprocess.run(gxx + ["-static-libasan", "-static-libubsan"] + objs + ["-o", str(tmp / "pf_result_check")], check=True)
    return str(tmp / "pf_result_check")


def test_result_side_under_asan(checker):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([checker], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert " failures 0" in r.stdout
