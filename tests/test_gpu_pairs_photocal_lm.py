"""The photometric calibration end to end on the device: the rendered pairs of tests/golden/filter_scene.npz (keyframe and frame
0) through the synthetic sensor of tests/test_pairs_photocal_api.py (a radial vignette down to 0.5 at the corners, the gamma-1/2.2
response), one object with the matching calibration (scale = min V) and one without, the SAME keypoints with their true depths in
both (mbavo_pairs_prepare_points on the grid of tests/pairs_refine_scene.py, so that the two costs sum over the same pixels; the
objects are every_candidate ones, whose levels have room for the 96 points), the
true knots moved by 3 cm as the start of both (mbavo_pairs_set_motion), mbavo_lm_batch_levels over two levels.  Asserted: the
calibrated run's final level-0 report cost is lower on every pair.  The pose errors of both runs are printed, not bounded
(profiles/r43_pairs_photocal.txt records them)."""
import numpy as np
import pytest

import pairs_device as dv
import pairs_filter_scene as fs
import pairs_photocal_ref as pc
import pairs_refine_scene as sc

pytestmark = pytest.mark.gpu


def test_calibrated_intake_lets_the_lm_end_lower(mbavo, gpu_ctx):
    from mba_vo_amd import workloads
    capi = mbavo.capi
    assert gpu_ctx.lib.mbavo_pairs_photocal_opts_size() == 32
    c, m = sc.scene(), sc.motion()
    V = pc.radial_vignette(sc.H, sc.W, 0.5)
    scale = float(V.min())
    sharp = np.stack([pc.sensor(c["sharp"][b], V) for b in range(sc.B)])
    blur = np.stack([pc.sensor(fs.frames(b, noise=0.0)[0], V) for b in range(sc.B)])
    points = [(sc.entry(b)["xy"], sc.entry(b)["z"]) for b in range(sc.B)]
    ends = {}
    for calibrated in (False, True):
        pb = workloads.PairBatch(gpu_ctx, sc.B, L=2, H=sc.H, W=sc.W, S=sc.S, k=sc.K_DEG, N=sc.N, border=4, huber=sc.HUBER, every_candidate=True)
        try:
            if calibrated:
                assert pb.set_photometric(pc.gamma_G(), dv.dev(V[None].copy())[0], scale=scale) == 0
            counts = pb.prepare_points(*dv.dev(np.ascontiguousarray(sharp), np.ascontiguousarray(blur)), points)
            assert (counts == len(points[0][1])).all()
            if calibrated:  # the object holds the restatement's images
                got = dv.read_batch(pb, counts)
                lut, inv = pc.table(pc.gamma_G(), scale), pc.inverse_vignette(V)
                assert all(np.array_equal(got[2 * b]["ref"], pc.pinhole(sharp[b], lut, inv).ravel()) for b in range(sc.B))
            assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"] + 0.03, m["kR"]) == 0
            start = [r.cost for r in pb.report(3.0)]
            dv.run_lm(gpu_ctx, capi, sc.B, 2, pb.array, sc.K_DEG)
            rep = pb.report(3.0)
            assert all(r.status == 0 for r in rep)
            kt, kR = pb.knots()
            ends[calibrated] = (start, [r.cost for r in rep], [float(np.abs(kt[b] - m["kt"][b]).max()) for b in range(sc.B)],
                                [float(np.abs(kR[b] - m["kR"][b]).max()) for b in range(sc.B)])
        finally:
            pb.close()
    for calibrated in (False, True):
        e = ends[calibrated]
        print("%s: level-0 report cost at the start %s, after the LM %s; largest knot error after the LM: translation %s  quaternion %s"
              % ("calibrated intake" if calibrated else "raw sensor images", np.round(e[0], 2).tolist(), np.round(e[1], 2).tolist(),
                 np.round(e[2], 4).tolist(), np.round(e[3], 5).tolist()))
    assert all(a < b_ for a, b_ in zip(ends[True][1], ends[False][1]))
