"""The host batch planner (csrc/pf_plan.cpp) checked without a GPU: tests/native/pf_plan_check.cpp plans
every golden file as one batch and hand-made descriptor sets at the sizes where a routing decision
flips, binds each plan to made-up arena addresses and asserts the arena, routing, Snappy-table and
failed-chunk invariants. Host code only, built here with g++ under AddressSanitizer + UBSan."""
import glob
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "parquet-floor_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plan")
    gxx = ["g++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", CSRC]
    srcs = [os.path.join(ROOT, "tests", "native", "pf_plan_check.cpp"), os.path.join(CSRC, "pf_plan.cpp"),
            os.path.join(CSRC, "pf_meta.cpp"), os.path.join(CSRC, "pf_file.cpp")]
    objs = [str(tmp / (os.path.basename(s) + ".o")) for s in srcs]
    # (the four translation units side by side: the sanitizers make each take seconds)
    procs = [subprocess.Popen(gxx + ["-c", s, "-o", o]) for s, o in zip(srcs, objs)]
    assert [p.wait() for p in procs] == [0] * len(procs)
    # the sanitizer runtimes linked in, so the program runs the same whatever else the loader brings first
    subprocess.run(gxx + ["-static-libasan", "-static-libubsan"] + objs + ["-o", str(tmp / "pf_plan_check")], check=True)
    return str(tmp / "pf_plan_check")


def test_planner_invariants_under_asan(checker):
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.parquet")) + glob.glob(os.path.join(GOLDEN, "crc", "*.parquet")))
    assert files
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([checker] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert f"files {len(files)} " in r.stdout and " failures 0" in r.stdout
