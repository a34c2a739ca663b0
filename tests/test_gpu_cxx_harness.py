"""-m gpu: the C++ module harness (tests/harness/harness.cpp) -- the counterpart of the reference's
test_blur_aware_tracker_modules, driving the SLAM::VO free functions with hipMalloc'd pointers."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_cxx_module_harness(mbavo):
    exe = os.path.join(HERE, "harness", "harness_bin")
    if not os.path.exists(exe):
        subprocess.run(["bash", os.path.join(HERE, "harness", "build.sh")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:]
    assert "HARNESS PASSED" in r.stdout


def test_device_solvers_against_host(mbavo):
    """One-wave Jacobi SVD / LDL^T of the device-side LM (lm_solvers.h) against host_math.cpp on random systems,
    n = 12 ... 96, full rank and rank deficient; tolerance 1e-8 relative on the solution.  The LDL^T stand-ins against exactly
    known integer solutions: the plain form inside its scaled forward bound, the refined form within 1e-12 and accepted up to
    cond ~1e9.  (The case-by-case check against high-precision references is tests/test_gpu_solvers.py.)"""
    exe = os.path.join(HERE, "harness", "solver_check_bin")
    if not os.path.exists(exe):
        subprocess.run(["bash", os.path.join(HERE, "harness", "build.sh")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0 and "SOLVER CHECK PASSED" in r.stdout, r.stdout[-2000:]


def test_cheap_division_is_the_ieee_division(mbavo):
    """pixel_math.h reciprocal() / quotient() (the runtime's fp64 division sequence minus range scaling and fix-up)
    give the bits of the compiler's IEEE division on 4M operand pairs drawn from the ranges they are used on and far
    beyond; tri_decode equals the row search for every packed index at ten matrix sizes."""
    exe = os.path.join(HERE, "harness", "div_check_bin")
    if not os.path.exists(exe):
        subprocess.run(["bash", os.path.join(HERE, "harness", "build.sh")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "DIV CHECK PASSED" in r.stdout, r.stdout[-2000:]


def test_bilinear_tap_at_every_edge(mbavo):
    """pixel_math.h tap_fetch + tap_blend called directly, one lane per (coordinate pair, variant): cost-only, float pairs, half
    pairs and packed keyframe words on 2x2 ... 33x65 images (0/255 checkerboards, random, independently filled gradient planes) that
    sit off their natural alignment between margins of other values.  Coordinates: the cross product of -inf ... the doubles around
    W - 2 and W - 1 ... 2^31, 2^32 + 0.5, inf, NaN on both axes and 65 536 random pairs per image.  The device's ok, val, gx, gy are
    the bits of a plain restatement of the reference's definition and of the header's host half, the same bits across the formats,
    and inside the derived bound of the long-double interpolant; every 9-bit field value and its half comes back exactly from an
    integer-coordinate tap.  (The host half under the host sanitizers: tests/test_tap_host.py.)"""
    exe = os.path.join(HERE, "harness", "tap_check_bin")
    if not os.path.exists(exe):
        subprocess.run(["bash", os.path.join(HERE, "harness", "build.sh")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-12000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "TAP CHECK PASSED" in r.stdout


def test_fast_math_forms_in_ulps(mbavo):
    """se3_math.h fastm::rcp, sqrt_rsqrt, sincos and atan_ratio called directly, one lane per argument, against long double on the host,
    in ulps of the correctly rounded double: a few 2^20 arguments per form over the ranges the pose chain passes and far beyond, every
    power of two, the doubles round the range limits of atan_ratio and round k pi/2 and (k + 1/2) pi/2 up to k = 65536.  The bounds are
    derived in the source (rcp and sqrt 0.5, rsqrt 1, sin and cos 1.93 plus |k| * 3.52e-27 absolute for the reduction constants, atan_ratio
    2.8); the raw v_rcp_f64 / v_rsq_f64 estimates are held to the premise of the derivation.  Then qlog<true>, qexp<true> and so3_exp on
    the device against the reference's formulas branch for branch in long double, value and Jacobian, within 4 max(host half's error,
    floor) and at most 1e-13, on three axes at ~160 000 angles each with both sides of every threshold.  (The same program without the
    device, under the host sanitizers: tests/test_fastm_host.py.)"""
    exe = os.path.join(HERE, "harness", "fastm_check_bin")
    if not os.path.exists(exe):
        subprocess.run(["bash", os.path.join(HERE, "harness", "build.sh")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-12000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "FASTM CHECK PASSED" in r.stdout


def test_segment_lookup_at_every_time(mbavo):
    """se3_math.h spline_segment_checked / spline_segment_index and pose_entries.h pose_sample_segment<2> / <4> called directly, one lane
    per case, in a kernel that reads no knots: t0 of {0, -3.5, 1.7e9}, dt of {0.5, 1/30, 1e-3}, k of {2, 4}, N of {k, k + 1, 7, 2^20}; segment
    numbers -2 .. N and the doubles beside each, -0.0, the smallest denormal and normal, 2^31 - 5 .. 2^31 + 1, 2^32 .. DBL_MAX of both signs,
    +-inf and NaN, each as a time and its two neighbours; 2^20 random times per (t0, dt); the sample times of S = 1, 2, 8, 21 under
    exposures 0, 0.1, NaN, inf and 1e300.  The flag is the one of an exact host reference (truncl and long long arithmetic), idx lies in
    [0, N - k] for every case, in range idx and u are the reference's bits, and the host half gives the device's bits for every case; no
    class of cases is empty.  (The host half under the host sanitizers: tests/test_segment_host.py.)"""
    exe = os.path.join(HERE, "harness", "segment_check_bin")
    if not os.path.exists(exe):
        subprocess.run(["bash", os.path.join(HERE, "harness", "build.sh")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-12000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "SEGMENT CHECK PASSED" in r.stdout
