"""The calibrated intake (mbavo_pairs_set_photometric) on the option-laden objects A - D of tests/pairs_oracle.py, held bit for bit
to pairs_oracle.host_levels through the intake hook of tests/pairs_photocal_support.py (tests/pairs_photocal_ref.py: remap, pinhole).
tests/test_gpu_pairs_photocal.py runs the calibration on B = 3, grid keypoints, float gradients, float z depth, undistort 0 or 1, at
most two cameras and 3072 pixels; here it meets what it must coexist with:
  A  75 x 101 pinhole = 7575 pixels: two workgroups of k_pairs_photocal_level0 per image, a ragged end, pairs 1 and 2 off a word;
     packed keyframe, ray-distance depth, k = 4 on segment 1
  B  undistort = 2 (raw 16-bit depth through the same maps), B = 4 on cameras (0, 1, 1, 0), clearance radius 2, raw masks, half
     gradients; its second frame by update and by track_frame
  C  every candidate, 72 x 100 from 80 x 112: eight workgroups per row of the calibrated remap
  D  prepare_points with three cameras and three calibrations, clearance radius 1, packed keyframe, L = 3
What the inputs must provide -- keypoints on every level, dead, saturated and changed bytes, no value on a rounding edge -- is
asserted without a GPU in tests/test_pairs_photocal_options_inputs.py.

Bounds.  The intake is equality: images on all levels, gradients in the object's format, keypoints, depths and counts, no item left
out.  The evaluation on the calibrated entries is held to the oracle with the bounds of tests/test_gpu_pairs_oracle.py (es.tol, the
patch-cost rule); nothing new is measured.  Figures on an MI355X: profiles/r44_photocal_options.txt."""
import ctypes as C

import numpy as np
import pytest

import pairs_device as dv
import pairs_entries_support as pe
import pairs_oracle as po
import pairs_photocal_support as ps
import pairs_track_support as tsup

pytestmark = pytest.mark.gpu

NAMES = sorted(po.OBJECTS)


@pytest.fixture(scope="module")
def made(mbavo, gpu_ctx):
    """name -> dict(pb, counts): each calibrated object made once, read only, closed at the end of the module."""
    held = {}

    def get(name):
        if name not in held:
            pb, counts = ps.make_calibrated(gpu_ctx, name)
            held[name] = dict(pb=pb, counts=counts)
        return held[name]
    yield get
    for h in held.values():
        h["pb"].close()


def _hook(name):
    return ps.intake(ps.calibration(name))


def _level0_differs(got, want, B, L):
    """Per pair: the number of level-0 keyframe bytes of a read-back that differ from the restatement's."""
    return [int((got[b * L]["ref"] != want[b][0]["ref"].ravel()).sum()) for b in range(B)]


@pytest.mark.parametrize("name", NAMES)
def test_every_entry_equals_the_calibrated_restatement(orc, mbavo, gpu_ctx, made, name):
    h = made(name)
    got = pe.check_entries(orc, mbavo.capi, h["pb"], name, intake=_hook(name))
    Ks = [[p[1][-1]["K"] for p in pair] for pair in got]
    assert h["counts"].tolist() == Ks
    assert h["pb"].photocal_stats() == (1, 0, 0)
    full = sum(int((pair[0][1][-1]["ref"] == 255).sum()) for pair in got)
    print("FIGURE entries object %s: %d (pair, level) entries bit for bit, K %s, level-0 keyframe bytes at 255: %d" % (name, sum(map(len, got)), Ks, full))


def test_the_second_frame_of_the_camera_set_object(orc, mbavo, gpu_ctx):
    """Object B's update with the key list [2] under the calibration equals the restatement of the second frame; the same frame
    through track_frame on a second instance leaves the same images."""
    name = "B"
    o, c, c2 = po.OBJECTS[name], po.inputs(name), po.second_frame(name)
    new_frame = lambda: (po._t(c["new_blur"]), [2], po._t(c["new_sharp"]), po._t(c["new_depth"]))
    pb, counts = ps.make_calibrated(gpu_ctx, name)
    twin, _ = ps.make_calibrated(gpu_ctx, name)
    try:
        new = pb.update(*new_frame())
        assert np.array_equal(new[[0, 1, 3]], counts[[0, 1, 3]]) and not np.array_equal(new[2], counts[2])
        po.set_motion(pb, c2["motion"])
        got = pe.check_entries(orc, mbavo.capi, pb, name, c2, intake=_hook(name))
        assert new.tolist() == [[p[1][-1]["K"] for p in pair] for pair in got]
        blur_t, keys, sharp_t, depth_t = new_frame()
        _, tracked, _, _ = dv.frames_of(gpu_ctx, mbavo.capi, twin, dict(B=o["B"]), blur_t, keys, sharp_t, depth_t, o["k"])
        assert tracked.tolist() == new.tolist()
        a, b = dv.read_batch(pb, new), dv.read_batch(twin, tracked)
        for e, (x, y) in enumerate(zip(a, b)):
            for key in ("ref", "cur", "grad", "xy", "z"):
                assert dv.same_bits(x[key], y[key]), ("track_frame", e, key)
        print("FIGURE second frame object B: update [2] bit for bit, K %s; track_frame leaves the same bytes on %d entries" % (new.tolist(), len(a)))
    finally:
        pb.close()
        twin.close()


def test_swapped_calibrations_must_fail(mbavo, gpu_ctx):
    """The comparison sees the fault it is there for: object B with its two cameras' calibrations swapped differs from the
    restatement in level-0 bytes of every pair."""
    name = "B"
    o = po.OBJECTS[name]
    pb, counts = ps.make_calibrated(gpu_ctx, name, cal=ps.swapped(ps.calibration(name)))
    try:
        differ = _level0_differs(dv.read_batch(pb, counts), ps.host_levels(name), o["B"], o["L"])
        print("FIGURE control object B: level-0 keyframe bytes that differ from the restatement under swapped calibrations, per pair: %s" % differ)
        assert all(n > 0 for n in differ)
    finally:
        pb.close()


@pytest.mark.parametrize("name", NAMES)
def test_set_alone_changes_nothing_and_clear_restores(orc, mbavo, gpu_ctx, name):
    """A set_photometric on a prepared object leaves every byte the object holds until the next intake; that intake then goes
    through it; clear_photometric and a prepare give the uncalibrated object."""
    o, other = po.OBJECTS[name], ps.another(name)
    pb, counts = ps.make_calibrated(gpu_ctx, name)
    try:
        before = dv.read_batch(pb, counts)
        keep = ps.set_photometric(pb, other)  # (the vignette's tensor)
        dv.assert_twins(dv.read_batch(pb, counts), before, (name, "set_photometric alone"))
        again = dv.read_batch(pb, po.prepare_object(pb, name))  # the next intake takes the new calibration
        assert _level0_differs(again, ps.host_levels(name, cal=other), o["B"], o["L"]) == [0] * o["B"]
        differ = _level0_differs(again, ps.host_levels(name), o["B"], o["L"])
        assert all(n > 0 for n in differ), differ
        assert pb.clear_photometric() == 0 and pb.photocal_stats() == (0, 0, 0)
        plain = po.prepare_object(pb, name)
        po.set_motion(pb, po.inputs(name)["motion"])
        got = pe.check_entries(orc, mbavo.capi, pb, name)
        assert plain.tolist() == [[p[1][-1]["K"] for p in pair] for pair in got]
        assert keep is not None
        print("FIGURE set / clear object %s: set_photometric alone left %d entries' bytes; the next prepare changed %s level-0 keyframe bytes per pair; "
              "after clear_photometric the uncalibrated restatement, K %s" % (name, len(before), differ, plain.tolist()))
    finally:
        pb.close()


@pytest.mark.parametrize("name", ["B", "D"])
def test_the_evaluation_sees_the_calibrated_bytes(orc, mbavo, gpu_ctx, made, name):
    capi, o = mbavo.capi, po.OBJECTS[name]
    pb = made(name)["pb"]
    po.set_motion(pb, po.inputs(name)["motion"])
    n = o["B"] * o["L"]
    flat = [x for pair in tsup.rebuilt(orc, capi, pb, o["k"]) for x in pair]
    want = [e for pair in ps.host_levels(name) for e in pair]
    for (p, keep), w in zip(flat, want):  # the evaluated entries are the calibrated ones
        assert np.array_equal(keep[-1]["ref"], w["ref"]) and np.array_equal(keep[-1]["curs"][0], w["curs"][0])
    arr = (capi.Problem * n)()
    C.memmove(arr, pb.array, C.sizeof(arr))
    pe.check_evaluation(orc, mbavo, gpu_ctx, arr, flat, o["k"], "calibrated " + name)
