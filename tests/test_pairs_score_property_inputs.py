"""The CPU twin of tests/test_gpu_pairs_score_property.py: on the scene of tests/pairs_score_scene.py (vertical stripes, a sparse
set of blobs, a depth plane; 96 x 128, 8 x 8 cells, generated from a seed) the restated keypoints under both responses are
evaluated with the oracle's level-0 Hessian and taken through the report restatement (tests/pairs_report_ref.py); the condition
number of the translational (v_x, v_y) block of info_unit is 46.43 under the gradient magnitude (K = 165) and 7.535 under the
corner score of radius 2 (K = 34): worse by a factor of 6.16, above the 4 the property needs.  Settings tried on the way (stripes
70 / 170, blobs + 40 unless stated; factor = gradient magnitude's condition number over the score's):
    24 blobs 3.57 (25.3 / 7.08)   48 blobs 2.32   16 blobs 4.59   12 blobs 6.16 (kept)   8 blobs 12.8 (K = 23 under the score)
    24 blobs of + 60: 3.19, of + 100: 2.79        stripes 110 / 130: 1.96    stripes 100 / 140: 2.73
    12 blobs with stripes 50 / 200: 6.21 (97.8 / 15.8)
Fewer blobs and stronger stripes widen the gap; stronger blobs close it, because the gradient magnitude then picks them too."""
import numpy as np

import pairs_score_scene as sc


def test_the_scene_is_what_the_property_needs(mbavo):
    assert mbavo.load().mbavo_pairs_detector_opts_size() == 32  # (the property is about this call)
    img = sc.keyframe()
    assert img.shape == (sc.H, sc.W) and sc.H <= 96 and sc.W <= 128 and np.array_equal(img, sc.keyframe())  # deterministic
    e0, e1 = sc.entry(0), sc.entry(sc.RADIUS)
    assert e0["K"] == 165 and e1["K"] == 34
    # the score's keypoints all touch a blob (ky != 0 in their window); most of the gradient magnitude's lie on a bare stripe edge
    ky = np.abs(img[2:, 1:-1].astype(int) - img[:-2, 1:-1].astype(int))
    near = lambda xy: np.array([ky[max(int(y) - 3, 0):int(y) + 2, max(int(x) - 3, 0):int(x) + 2].any() for x, y in xy])
    assert near(e1["xy"]).all() and near(e0["xy"]).mean() < 0.5


def test_the_gradient_magnitude_is_worse_conditioned_by_the_stated_factor(mbavo, orc):
    assert mbavo.load().mbavo_pairs_detector_opts_size() == 32
    c0, K0, b0 = sc.cpu_condition(orc, 0)
    c1, K1, b1 = sc.cpu_condition(orc, sc.RADIUS)
    print("FIGURE conditioning on the CPU: gradient magnitude %.4g (K %d, block %s), corner score r = %d %.4g (K %d, block %s), factor %.4g"
          % (c0, K0, b0.tolist(), sc.RADIUS, c1, K1, b1.tolist(), c0 / c1))
    assert abs(c0 - sc.COND_GRAD) <= 1e-3 * sc.COND_GRAD and abs(c1 - sc.COND_SCORE) <= 1e-3 * sc.COND_SCORE  # the recorded figures
    assert c0 / c1 >= 4.0 and sc.FACTOR >= 4.0
