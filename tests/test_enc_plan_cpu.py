"""The write path's host planner (csrc/pf_enc_plan.cpp) checked without a GPU: tests/native/pf_enc_plan_check.cpp
plans one grid of columns (every type, REQUIRED / OPTIONAL with and without validity, 0 to 40,007 rows, three page
sizes, the option bits, the codecs, with and without a Bloom filter) and asserts every call error's code and text,
the page plan, the delta / statistics / page-index tables, the arena layout bound to a made-up address, the
sections of every route at sizes up to the reserved worst case, the compression layout, and the assembled chunk
walked back by pf_meta.cpp with each page's CRC recomputed bytewise. Host code only, built here with g++ under
AddressSanitizer + UBSan as a stand-alone program."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "parquet-floor_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("enc_plan")
    # no ROCm include path: the planner and its tables are plain C++
    gxx = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", CSRC]
    srcs = [os.path.join(ROOT, "tests", "native", "pf_enc_plan_check.cpp"), os.path.join(CSRC, "pf_enc_plan.cpp"),
            os.path.join(CSRC, "pf_write.cpp"), os.path.join(CSRC, "pf_meta.cpp")]
    objs = [str(tmp / (os.path.basename(s) + ".o")) for s in srcs]
    procs = [subprocess.Popen(gxx + ["-c", s, "-o", o]) for s, o in zip(srcs, objs)]
    assert [p.wait() for p in procs] == [0] * len(procs)
    # the sanitizer runtimes linked in, so the program runs the same whatever else the loader brings first
    subprocess.run(gxx + ["-static-libasan", "-static-libubsan"] + objs + ["-o", str(tmp / "pf_enc_plan_check")], check=True)
    return str(tmp / "pf_enc_plan_check")


def test_encode_planner_invariants_under_asan(checker):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([checker], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # 6 types x 3 level forms x 9 row counts x 3 page sizes x 8 bit sets x 3 codecs x 2 filter sizes
    assert "cases 23328 " in r.stdout and " failures 0" in r.stdout
