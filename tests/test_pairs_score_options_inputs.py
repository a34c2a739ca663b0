"""The CPU side of tests/test_gpu_pairs_score_options.py: under its radius and threshold the restated selection leaves keypoints
on every (pair, level) of the option-laden objects A - D (the entry comparison asserts K > 0), the keypoints of the detector
objects A - C differ from those under the gradient magnitude (else the test could not tell the responses apart), and object D,
which takes the caller's points, is unchanged."""
import numpy as np
import pytest

import pairs_oracle as po
import pairs_score_ref as sr

RADIUS, THR = 2, 2.0  # those of tests/test_gpu_pairs_score_options.py


@pytest.mark.parametrize("name", sorted(po.OBJECTS))
def test_scored_objects_keep_keypoints_and_differ(mbavo, name):
    assert mbavo.load().mbavo_pairs_detector_opts_size() == 32  # (the objects are switched by this call)
    plain = po.host_levels(name)
    scored = sr.host_levels(name, RADIUS, THR)
    assert po.OBJECTS[name]["thr"] != THR or name == "D"        # (and the swap has been undone)
    same = 0
    for pw, sw in zip(plain, scored):
        for p, s in zip(pw, sw):
            assert s["K"] > 0 and np.array_equal(p["ref"], s["ref"]) and np.array_equal(p["grad"], s["grad"])
            same += int(p["K"] == s["K"] and np.array_equal(p["xy"], s["xy"]))
    n = sum(len(pw) for pw in plain)
    if po.OBJECTS[name]["points"]:
        assert same == n, (name, same, n)
    else:  # every pair's level 0 differs (a coarse level of the every-candidate object may keep nearly every pixel under both)
        assert same < n and all(not np.array_equal(pw[0]["xy"], sw[0]["xy"]) for pw, sw in zip(plain, scored)), (name, same, n)
