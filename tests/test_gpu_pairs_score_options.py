"""The corner score on the four option-laden objects A - D of tests/pairs_oracle.py (raw images, the unified camera, camera sets,
raw-geometry depth, clearance, masks, packed keyframes; D takes the caller's points and has no detector), switched by
make_object's before_prepare hook: every entry, read back with read_entry, equals host_levels under the swapped response
(tests/pairs_score_ref.py: scored_object) bit for bit, at the shapes those objects have.  One evaluation of B and D on the corner
keypoints is held to the oracle under the bounds of tests/pairs_entries_support.py: the evaluation kernels do not care where
keypoints came from.

RADIUS and THR are fixed here; tests/test_pairs_score_options_inputs.py asserts on the CPU that every (pair, level) keeps
keypoints under them and that the keypoints of A - C differ from those under the gradient magnitude."""
import ctypes as C

import numpy as np
import pytest

import pairs_entries_support as pe
import pairs_oracle as po
import pairs_score_ref as sr
import pairs_track_support as tsup

pytestmark = pytest.mark.gpu

NAMES = sorted(po.OBJECTS)
RADIUS, THR = 2, 2.0


@pytest.fixture(scope="module")
def made(mbavo, gpu_ctx):
    """name -> dict(pb, counts): each object made once under the score, read only, closed at the end of the module."""
    held = {}

    def get(name):
        if name not in held:
            def switch(pb):
                assert pb.set_detector(1, RADIUS, THR) == 0
            pb, counts = po.make_object(gpu_ctx, name, before_prepare=switch)
            held[name] = dict(pb=pb, counts=counts)
        return held[name]
    yield get
    for h in held.values():
        h["pb"].close()


@pytest.mark.parametrize("name", NAMES)
def test_every_entry_equals_the_restatement_under_the_score(orc, mbavo, gpu_ctx, made, name):
    h = made(name)
    with sr.scored_object(name, RADIUS, THR):
        got = pe.check_entries(orc, mbavo.capi, h["pb"], name)
    Ks = [[p[1][-1]["K"] for p in pair] for pair in got]
    assert h["counts"].tolist() == Ks
    assert h["pb"].detector_stats()[:2] == (1, RADIUS) and h["pb"].detector_stats()[2] > 0
    print("FIGURE entries object %s under the corner score: %d (pair, level) entries bit for bit, K %s" % (name, sum(map(len, got)), Ks))


@pytest.mark.parametrize("name", ["B", "D"])
def test_the_evaluation_does_not_care_where_keypoints_came_from(orc, mbavo, gpu_ctx, made, name):
    capi, o = mbavo.capi, po.OBJECTS[name]
    pb = made(name)["pb"]
    po.set_motion(pb, po.inputs(name)["motion"])
    n = o["B"] * o["L"]
    flat = [x for pair in tsup.rebuilt(orc, capi, pb, o["k"]) for x in pair]
    want = [e for pair in sr.host_levels(name, RADIUS, THR) for e in pair]
    for (p, keep), w in zip(flat, want):  # the evaluated entries hold the corner keypoints
        assert np.array_equal(keep[-1]["xy"], w["xy"]) and np.array_equal(keep[-1]["z"], w["z"])
    arr = (capi.Problem * n)()
    C.memmove(arr, pb.array, C.sizeof(arr))
    pe.check_evaluation(orc, mbavo, gpu_ctx, arr, flat, o["k"], "corner score " + name)
