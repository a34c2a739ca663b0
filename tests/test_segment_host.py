"""CPU: the host half of the spline's range gate (se3_math.h: spline_segment_checked, spline_segment_index) under the host
sanitizers.  tests/harness/segment_check.hip is built a second time with the host side instrumented -- AddressSanitizer,
UndefinedBehaviorSanitizer and, named on its own because `undefined` does not include it, float-cast-overflow: the conversion
(int)((t - t0) / dt) of a NaN, infinite or far time is what this is about -- and run with --host: every case of the device run
through the host half against the exact reference, nothing launched.  A stand-alone program: nothing is preloaded.  (The device
run of the same program is tests/test_gpu_cxx_harness.py::test_segment_lookup_at_every_time.)"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HARNESS = os.path.join(HERE, "harness")
SRC = os.path.join(HARNESS, "segment_check.hip")
EXE = os.path.join(HARNESS, "segment_check_host_asan_bin")
CSRC = os.path.join(ROOT, "mba-vo_amd", "csrc")


def _stale():
    if not os.path.exists(EXE):
        return True
    built = os.path.getmtime(EXE)
    return any(os.path.getmtime(p) > built for p in [SRC] + [os.path.join(CSRC, h) for h in ("se3_math.h", "pose_entries.h", "engine.h", "pixel_math.h", "core_types.h")])


def test_host_segment_lookup_under_sanitizers():
    if os.path.exists("/dev/kfd"):
        pytest.skip("the sanitizer build is for machines without a GPU; with one, the device test runs the uninstrumented program")
    if _stale():
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        "-Xarch_host", "-fsanitize=address,undefined,float-cast-overflow", SRC, "-o", EXE], check=True, cwd=HARNESS)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LD_PRELOAD")}
    r = subprocess.run([EXE, "--host"], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-6000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "SEGMENT CHECK PASSED" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
