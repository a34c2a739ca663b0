"""-m gpu: the layout of the per-wave row slab behind the outer product (engine.hip: OuterAcc<ND>::at / accumulate and every place
that parks a row -- k_fused's round loop, sp_round_rt, the sample-parallel kernel's tile body).

Which address a row entry is parked at, and where the matrix core's operand (step, kq, group, e) is read back from, decides no
arithmetic: the rows, the MFMA order and every sum are what they were.  So every output must be the SAME BITS as the library of the
commit before the layout switch computed; those are recorded under tests/golden/slab_layout/<case>.npy (one float64 vector per case:
frame blocks, per-patch costs, valid counts, then the cost-only call's three; written by tests/golden/make_slab_layout_golden.py
with that library) -- and within the project's oracle bound (eval_support.tol).

Cases: the smallest shapes at which the layout can go wrong, all one tile on a 40 x 30 image (or 160 x 120 for the 8-pixel patches):
  lane_100    100 one-pixel patches, S = 3 (no sample-parallel remainder): one wave with a full 64-row slab, one with 36 rows and 28
              zero rows -- the full-slab path of accumulate
  rem_300     300 one-pixel patches, S = 8: one round of 256 and a remainder of 44 through sp_round_rt (two samples per lane, 16
              pixels per wave: accumulate with nsteps = 4 < 16)
  rem_S64     276 one-pixel patches, S = 64: the remainder's waves hold 2 pixels each, rows 2 and 3 of the one MFMA step are the
              zero padding
  (k = 4: ND = 25, seven groups, the closed-trail form; k = 2: ND = 13, four groups, the generic form)
  semidense   8-pixel patches through k_fused_sp: S = 8 (8 pixels per wave, nsteps = 2) and S = 32 (2 pixels per wave, zero padding)
  zero_rows   keypoints scattered over and beyond the image border, a fifth of them flagged as outliers, two with NaN / inf depth
              (their lanes' Jacobian sums are NaN): such rows park zeros and no NaN reaches a gathered entry; lane-per-pixel and
              through the remainder round
  cost-only   has no slab: guards what aliases into the slabs' space (the wave sums behind them, the prologue's segment records)"""
import os

import numpy as np
import pytest

import eval_support as es
import scenes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slab_layout")
KEYS = ("fb", "pc", "valid", "fc", "pcc", "validc")  # the order inside a case's golden vector

LANE = dict(sample_parallel=-1, fused_pose=1, fused_pose_max_samples=21, min_tile_pixels=1 << 20)  # k_fused, one tile
SP = dict(sample_parallel=1)                                                                          # k_fused_sp


def _one_px(K, S, k, seed, **kw):
    return dict(H=30, W=40, S=S, F=1, k=k, P=1, K=K, margin=3, seed=seed, **kw)


def _patches(K, S, k, seed, **kw):
    return dict(H=120, W=160, S=S, F=1, k=k, P=8, K=K, margin=12, seed=seed, **kw)


SLOW = dict(trans_scale=0.002, rot_scale=0.02)  # (S >= 32: the motion of the other tests' long exposures)
# name -> (k, scene keywords, engine options, non-finite depths {keypoint: value}, expected kernel prefix)
CASES = {}
for _k in (4, 2):
    CASES["k%d_lane_100" % _k] = (_k, _one_px(100, 3, _k, 11), LANE, {}, "k_fused<%d,true," % _k)
    CASES["k%d_rem_300" % _k] = (_k, _one_px(300, 8, _k, 12), LANE, {}, "k_fused<%d,true," % _k)
    CASES["k%d_semidense_S8" % _k] = (_k, _patches(60, 8, _k, 14), SP, {}, "k_fused_sp<%d,true," % _k)
CASES["k4_rem_S64"] = (4, _one_px(276, 64, 4, 13, **SLOW), dict(LANE, fused_pose=-1), {}, "k_fused<4,true,")
CASES["k4_semidense_S32"] = (4, _patches(20, 32, 4, 15, **SLOW), SP, {}, "k_fused_sp<4,true,")
CASES["k4_zero_rows"] = (4, _one_px(150, 3, 4, 16, kp="border", outlier_frac=0.2), LANE, {5: np.nan, 70: np.inf}, "k_fused<4,true,")
CASES["k4_zero_rows_rem"] = (4, _one_px(300, 8, 4, 17, kp="border", outlier_frac=0.2), LANE, {5: np.nan, 270: np.nan, 290: np.inf},
                             "k_fused<4,true,")


def make_scene(name):
    k, kw, opts, bad_z, kern = CASES[name]
    sc = scenes.Scene(**kw)
    for i, z in bad_z.items():
        sc.kp_z[i] = z
    return sc


def evaluate(mbavo, ctx, name):
    """The case through every evaluation entry point (eval_support.run) under its engine options."""
    k, kw, opts, bad_z, kern = CASES[name]
    sc = make_scene(name)
    try:
        ctx.engine_opts(**opts)
        return sc, es.run(mbavo, ctx, k, [sc], [scenes.DeviceScene(sc)])
    finally:
        ctx.engine_opts()


def pack(r):
    return np.concatenate([np.asarray(r[key], np.float64).ravel() for key in KEYS])


_RUNS = {}


def _run(mbavo, ctx, name):
    if name not in _RUNS:  # once per case, shared by the tests below and never modified
        sc, r = evaluate(mbavo, ctx, name)
        for key in KEYS:
            r[key].setflags(write=False)
        _RUNS[name] = (sc, r)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_as_before_the_layout_switch(orc, mbavo, gpu_ctx, name):
    k, kw, opts, bad_z, kern = CASES[name]
    sc, r = _run(mbavo, gpu_ctx, name)
    assert r["kern"].startswith(kern) and r["kern_m"].startswith(kern), (r["kern"], r["kern_m"])
    assert r["lay"]["nprob"] == 1 and (opts is SP or r["lay"]["ntiles"] == sc.F), r["lay"]  # (k_fused: ONE tile holds all the pixels)
    want = np.load(os.path.join(GOLDEN, name + ".npy"))
    got = pack(r)
    assert got.shape == want.shape
    at = 0
    for key in KEYS:  # per output, so that a failure names it
        n = r[key].size
        assert np.array_equal(got[at:at + n], want[at:at + n]), (name, key)
        at += n
    assert np.array_equal(r["fb_m"], r["fb"]) and np.array_equal(r["sys_m"], r["sys_a"])
    # ... and the oracle, within the project's bound
    p, keep = sc.oracle_problem(orc)
    fbo = orc.evaluate(p)["frame_blocks"].reshape(sc.F, sc.E)
    fco = orc.evaluate(p, with_hessian=False)["frame_blocks"].reshape(sc.F, sc.E)[:, 0]
    vo = es.oracle_valid_counts(orc, sc)
    tol = es.tol(sc)
    d_fb, d_fc = es.rel(r["fb"], fbo), es.rel(r["fc"], fco)
    print("slab_layout_figures %s kern=%s fb=%.3g fc=%.3g tol=%.3g valid=%d of %d" % (name, r["kern"], d_fb, d_fc, tol, vo.sum(), sc.K * sc.P))
    assert np.isfinite(fbo).all() and np.isfinite(r["fb"]).all() and np.isfinite(r["pc"]).all()
    assert d_fb <= tol and d_fc <= tol, (name, d_fb, d_fc, tol)
    assert np.array_equal(r["valid"], vo) and np.array_equal(r["validc"], vo)


@pytest.mark.parametrize("name", ["k4_zero_rows", "k4_zero_rows_rem"])
def test_dropped_pixels_park_zero_rows(orc, mbavo, gpu_ctx, name):
    """The reference alone says that the case has valid AND invalid pixels, flagged keypoints among the valid ones and keypoints
    of non-finite depth (invalid: the Jacobian sums of their lanes are NaN); the blocks are finite and the flagged and the
    non-finite keypoints' costs do not reach the frame cost."""
    k, kw, opts, bad_z, kern = CASES[name]
    sc, r = _run(mbavo, gpu_ctx, name)
    vo = es.oracle_valid_counts(orc, sc)
    n_valid, n_invalid = int(vo.sum()), sc.K * sc.P - int(vo.sum())
    assert n_valid > 0 and n_invalid >= len(bad_z) > 0, (n_valid, n_invalid)
    assert 0 < sc.num_bad < sc.K and not any(np.isfinite(sc.kp_z[i]) for i in bad_z)
    if name.endswith("_rem"):  # non-finite depths on both sides of the split: the round of 256 and the remainder
        assert min(bad_z) < 256 <= max(bad_z) < sc.K
    assert np.isfinite(r["fb"]).all() and np.isfinite(r["pc"]).all() and np.array_equal(r["valid"], vo)
    assert (r["pc"][list(bad_z)] == 0.0).all()
    p, keep = sc.oracle_problem(orc)
    po = orc.evaluate(p)["patch_blocks"].reshape(-1, sc.E)[:, 0]
    flagged_valid = (sc.outlier == 1) & (po != 0.0)
    assert flagged_valid.any()  # an outlier whose row would NOT have been zero anyway


def test_cost_only_is_untouched(mbavo, gpu_ctx):
    """The cost-only kernels have no slabs; their wave sums and the prologue's segment records sit where the slabs would be."""
    for name in ("k4_lane_100", "k2_rem_300"):
        k = CASES[name][0]
        sc, r = _run(mbavo, gpu_ctx, name)
        assert r["kern_c"] == "k_fused<%d,false,false,true>" % k, r["kern_c"]
        want = np.load(os.path.join(GOLDEN, name + ".npy"))
        n = sum(r[key].size for key in KEYS[:3])
        assert np.array_equal(pack(r)[n:], want[n:]), name
        assert r["fc"][0] > 0.0 and abs(r["fc"][0] - r["fb"][0, 0]) <= 1e-11 * r["fb"][0, 0]  # (the bound of eval_support's fuzz)
