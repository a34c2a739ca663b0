"""What tests/test_gpu_pairs_photocal_options.py rests on, asserted without a GPU from the numpy restatements alone: the objects
A - D of tests/pairs_oracle.py under the calibrations of tests/pairs_photocal_support.py.

Keypoints survive: every (pair, level) of the calibrated restatement keeps K > 0, the grid objects A and B at least half the
plain object's K (measured: at least 0.88, A pair 0 level 1, 76 of 86; D's lists are the caller's and unchanged).  The level-0
images reach every branch of the intake: bytes that differ from the uncalibrated intake, bytes that are 0 BECAUSE a vignette pixel
is dead (they are not 0 under the same calibration with the dead pixels set to 1) and bytes at 255.  Every level-0 entry keeps
more than 6 valid pixels for the evaluation (B and D are evaluated on the device).

Rounding edges.  The device comparison is bit for bit and leaves nothing out, so this is a condition, not a tolerance: no value v
that an intake of these inputs rounds to a byte -- object B's second frame included -- has |frac(v) - 0.5| < 1e-9.  A violation is
answered by another calibration, never by a margin.

The quotient.  tests/pairs_photocal_ref.py restates the device's inverse vignette, (float)(1.0 / (double)V), as numpy's float32
division.  That holds if the float of the double quotient is the correctly rounded float quotient (53 >= 2 * 24 + 2 bits); it is
checked here on 2^20 random positive floats over the whole exponent range and the edges of the vignette's domain."""
import numpy as np
import pytest

import pairs_oracle as po
import pairs_photocal_ref as pc
import pairs_photocal_support as ps

NAMES = sorted(po.OBJECTS)
EDGE = 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_keypoints_survive_the_calibration(name):
    o = po.OBJECTS[name]
    cal = np.array([[e["K"] for e in pair] for pair in ps.host_levels(name)])
    plain = np.array([[e["K"] for e in pair] for pair in po.host_levels(name)])
    print("object %s: K per (pair, level) calibrated %s plain %s, smallest share %.3f" % (name, cal.tolist(), plain.tolist(), float((cal / plain).min())))
    assert cal.shape == (o["B"], o["L"]) and (cal > 0).all()
    if name in ("A", "B"):
        assert (2 * cal >= plain).all()
    if name == "C":
        assert (cal[:, 0] > 4096).all()  # still the every-candidate object beyond one workgroup's keypoints


@pytest.mark.parametrize("name", NAMES)
def test_level0_reaches_every_branch_of_the_intake(name):
    cal = ps.calibration(name)
    assert cal["n"] == ps.cameras(name) and len(set(ps.GAMMAS[:cal["n"]])) == cal["n"]
    inv, V = cal["inv"], cal["V"]
    for g in range(cal["n"]):  # what the issue asks of a vignette: a block below v_min, a NaN, a 0, a block above 1
        assert ((V[g] < pc.V_MIN) & (V[g] > 0)).sum() >= 20 and np.isnan(V[g]).sum() == 1 and (V[g] == 0).sum() == 1 and (V[g] > 1).sum() >= 20
        assert (inv[g] == 0).sum() == ps.DEAD_BLOCK[0] * ps.DEAD_BLOCK[1]
    got = ps.level0_images(name, hook=ps.intake(cal))
    plain = ps.level0_images(name)
    alive = ps.level0_images(name, hook=ps.intake(dict(cal, inv=np.where(inv == 0, np.float32(1.0), inv))))
    differ = sum(int((a != b).sum()) for a, b in zip(got, plain))
    dead = sum(int(((a == 0) & (b != 0)).sum()) for a, b in zip(got, alive))
    full = sum(int((a == 255).sum()) for a in got)
    print("object %s: level-0 bytes that differ from the uncalibrated intake %d, at 0 from dead vignette pixels %d, at 255 %d" % (name, differ, dead, full))
    assert differ > 0 and dead > 0 and full > 0


@pytest.mark.parametrize("name", NAMES)
def test_no_value_lies_on_a_rounding_edge(name):
    cal = ps.calibration(name)
    values = []
    ps.level0_images(name, hook=ps.intake(cal, values))
    if name == "B":
        ps.level0_images(name, c=po.second_frame(name), hook=ps.intake(cal, values))
        ps.level0_images(name, hook=ps.intake(ps.swapped(cal), values))  # the control's values: a differing byte is no rounding
    n = on_edge = 0
    nearest = np.inf
    for usable, v in values:
        assert np.isfinite(v[usable]).all() and (v[usable] >= 0).all()
        w = np.fmin(v[usable], 255.0)
        d = np.abs(w - np.floor(w) - 0.5)
        n, on_edge, nearest = n + d.size, on_edge + int((d < EDGE).sum()), min(nearest, float(d.min()))
    print("object %s: %d values, %d within %.0e of a rounding edge, the nearest %.3g away" % (name, n, on_edge, EDGE, nearest))
    assert on_edge == 0


@pytest.mark.parametrize("name", ["B", "D"])
def test_the_calibrated_entries_can_be_evaluated(orc, name):
    for b, pair in enumerate(ps.host_levels(name)):
        for l, e in enumerate(pair):
            p, keep = po.problem_of(orc, dict(e))
            assert orc.count_valid(p)[0] > 6, (name, b, l)


def test_the_wrong_camera_control_can_fail():
    """Object B with the two cameras' calibrations swapped differs from the restatement in level-0 bytes of every pair."""
    cal = ps.calibration("B")
    right, wrong = ps.level0_images("B", hook=ps.intake(cal)), ps.level0_images("B", hook=ps.intake(ps.swapped(cal)))
    counts = [int((a != b).sum()) for a, b in zip(right, wrong)]
    print("object B under swapped calibrations: differing level-0 bytes per image %s" % counts)
    assert all(n > 0 for n in counts)


def test_the_float_of_the_double_quotient_is_the_float_quotient():
    rng = np.random.default_rng(44)
    bits = rng.integers(1, 0x7f800000, 1 << 20, dtype=np.uint32)  # every positive finite float32, subnormals included
    edges = np.array([0.0625, np.nextafter(np.float32(0.0625), np.float32(0)), np.finfo(np.float32).tiny, 1e-40, np.finfo(np.float32).max, 1.0, 3.0,
                      np.float32(1.0) / np.float32(3.0)], np.float32)
    V = np.concatenate([bits.view(np.float32), edges])
    assert V.dtype == np.float32 and (V > 0).all() and np.isfinite(V).all() and (V < np.finfo(np.float32).tiny).any()
    with np.errstate(over="ignore"):
        single = np.float32(1.0) / V
        double = (1.0 / V.astype(np.float64)).astype(np.float32)
    assert single.dtype == np.float32 and np.array_equal(single.view(np.uint32), double.view(np.uint32))
    assert np.isinf(single).any()  # (the inverse of a small subnormal: the corner photocal_math.h documents)
    assert np.array_equal(pc.inverse_vignette(edges, 1e-40).view(np.uint32), double[-len(edges):].view(np.uint32))
