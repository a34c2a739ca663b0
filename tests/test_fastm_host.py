"""CPU: tests/harness/fastm_check.hip under the host sanitizers.  The program is built a second time with the host side instrumented
(AddressSanitizer and UndefinedBehaviorSanitizer; the device side is compiled as always and never launched) and run with --host: every
input list of the device run is made, libm's sin, cos, atan, sqrt and the IEEE division go through the same ulp checker against long
double in the device forms' place -- each operation at or below 1 ulp of its own argument, sqrt and the division correctly rounded, the
compositions 1 / sqrt(x) and atan(n / w) at the 1.5 and 2 ulp that follows -- which proves the checker and the reference on the machine
at hand; the qlog / qexp / so3_exp table is evaluated with the header's host half against the long-double restatement (no case's bound
over 1e-13 of its largest entry, at least 100 cases in every branch).  A stand-alone program: nothing is preloaded.  (The device run of
the same program is tests/test_gpu_cxx_harness.py::test_fast_math_forms_in_ulps.)"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HARNESS = os.path.join(HERE, "harness")
SRC = os.path.join(HARNESS, "fastm_check.hip")
EXE = os.path.join(HARNESS, "fastm_check_host_asan_bin")
CSRC = os.path.join(ROOT, "mba-vo_amd", "csrc")


def _stale():
    if not os.path.exists(EXE):
        return True
    built = os.path.getmtime(EXE)
    return any(os.path.getmtime(p) > built for p in [SRC] + [os.path.join(CSRC, h) for h in ("se3_math.h", "core_types.h")])


def test_host_fast_math_check_under_sanitizers():
    if os.path.exists("/dev/kfd"):
        pytest.skip("the sanitizer build is for machines without a GPU; with one, the device test runs the uninstrumented program")
    if _stale():
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        "-Xarch_host", "-fsanitize=address,undefined", SRC, "-o", EXE], check=True, cwd=HARNESS)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LD_PRELOAD")}
    r = subprocess.run([EXE, "--host"], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-12000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "FASTM CHECK PASSED" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
