"""CPU: the host half of the bilinear keyframe tap (pixel_math.h: tap_fetch / tap_blend / bilinear_tap) under the host
sanitizers.  tests/harness/tap_check.hip is built a second time with the host side instrumented (AddressSanitizer and
UndefinedBehaviorSanitizer; the device side is compiled as always and never launched) and run with --host: reference A, reference
B, the host half in all four variants at every edge coordinate, and the field sweep, on images allocated at their exact size, so a
tap that reads outside its image is a heap overflow.  A stand-alone program: nothing is preloaded.  (The device run of the same
program is tests/test_gpu_cxx_harness.py::test_bilinear_tap_at_every_edge.)"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HARNESS = os.path.join(HERE, "harness")
SRC = os.path.join(HARNESS, "tap_check.hip")
EXE = os.path.join(HARNESS, "tap_check_host_asan_bin")
CSRC = os.path.join(ROOT, "mba-vo_amd", "csrc")


def _stale():
    if not os.path.exists(EXE):
        return True
    built = os.path.getmtime(EXE)
    return any(os.path.getmtime(p) > built for p in [SRC] + [os.path.join(CSRC, h) for h in ("pixel_math.h", "core_types.h", "se3_math.h")])


def test_host_tap_under_sanitizers():
    if os.path.exists("/dev/kfd"):
        pytest.skip("the sanitizer build is for machines without a GPU; with one, the device test runs the uninstrumented program")
    if _stale():
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        "-Xarch_host", "-fsanitize=address,undefined", SRC, "-o", EXE], check=True, cwd=HARNESS)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LD_PRELOAD")}
    r = subprocess.run([EXE, "--host"], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-6000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "TAP CHECK PASSED" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
