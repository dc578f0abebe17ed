"""The host batch planner (csrc/pf_plan.cpp) on LZ4_RAW chunks, without a GPU:
tests/native/pf_lz4_plan_check.cpp plans hand-made descriptor sets -- an LZ4_RAW chunk, more jobs
than k_lz4 has workgroups, a batch mixing LZ4_RAW, ZSTD, Snappy and uncompressed chunks, pages
without bytes, the codecs still refused -- and asserts the region, job and list invariants. Built
here with g++ under ASan + UBSan."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "parquet-floor_amd", "csrc")


def test_lz4_plan_invariants_under_asan(tmp_path):
    exe = str(tmp_path / "pf_lz4_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "pf_lz4_plan_check.cpp"),
                    os.path.join(CSRC, "pf_plan.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "failures 0" in r.stdout
