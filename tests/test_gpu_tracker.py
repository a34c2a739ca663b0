"""-m gpu: the LM loop on the fused engine against the oracle's loop on the same synthetic blurred
sequence.  Integer outputs (knot start indices, accept / reject sequence, outlier counts) must be
identical.  Each evaluation agrees to ~1e-15, but the two solvers (one-sided Jacobi SVD here, Eigen's
two-sided scheme restated in the oracle) differ by rounding x cond(H) and the iterates inherit it: costs along
the trace 1e-6 relative (observed ~3e-9), converged knots 1e-6, ATE within 1e-5 (north_star)."""
import numpy as np
import pytest

import tracking

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,kw", [
    ("k4_semidense", dict(H=120, W=160, levels=3, S=8, k=4, seed=1)),
    ("k2_semidense", dict(H=120, W=160, levels=3, S=8, k=2, seed=2)),
    ("k4_dense_2frames", dict(H=96, W=128, levels=2, S=4, k=4, F=2, seed=3, mode="dense")),
    ("k4_ldlt", dict(H=120, W=160, levels=3, S=8, k=4, seed=4)),
    # BASELINE size: 640x480, 4-level pyramid, 8 blur samples (configs[1]), ~1 080 semi-dense keypoints x 8-pixel pattern
    ("k4_fullsize", dict(H=480, W=640, levels=4, S=8, k=4, seed=5)),
    ("k2_fullsize", dict(H=480, W=640, levels=4, S=8, k=2, seed=6)),
    ("k4_fullsize_2frames", dict(H=480, W=640, levels=4, S=8, k=4, F=2, seed=7)),
])
def test_tracker_matches_oracle(orc, mbavo, gpu_ctx, name, kw):
    sc = tracking.make_tracking_scene(orc, **kw)
    opts = dict(tracking.OPTS)
    if "ldlt" in name:
        opts["solver_type"] = 1
    ro = tracking.run_oracle_tracker(orc, sc, opts)
    rg = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, opts)
    assert np.array_equal(ro["start"], rg["start"])                      # bit-identical pose (knot segment) indices
    assert len(ro["trace"]) == len(rg["trace"])
    for a, b in zip(ro["trace"], rg["trace"]):
        assert a[:4] == b[:4], (a, b)                                    # level, iteration, accept/reject kind, #outliers
        assert a[4] == pytest.approx(b[4], rel=1e-4)                     # LM radius (a ratio of small cost differences)
        assert a[5] == pytest.approx(b[5], rel=1e-6, abs=1e-12)          # evaluation cost
        assert a[6] == pytest.approx(b[6], rel=1e-6, abs=1e-12)          # candidate cost
    # weakly observed knot components (a single short exposure hardly constrains the outer knots) amplify the
    # solver rounding most; what the tracker returns is the pose on the spline at capture time
    assert np.abs(ro["kt"] - rg["kt"]).max() < 1e-4 and np.abs(ro["kR"] - rg["kR"]).max() < 1e-4
    for c in sc["cap"]:
        po, qo = tracking.pose_at(orc, sc["k"], sc["t0"], sc["dt"], ro["kt"], ro["kR"], c)
        pg, qg = tracking.pose_at(orc, sc["k"], sc["t0"], sc["dt"], rg["kt"], rg["kR"], c)
        assert np.abs(po - pg).max() < 1e-5 and np.abs(qo - qg).max() < 1e-5
    ate_o, ate_g = tracking.ate(orc, sc, ro["kt"], ro["kR"]), tracking.ate(orc, sc, rg["kt"], rg["kR"])
    assert abs(ate_o - ate_g) <= 1e-5
    assert rg["cost"] < rg["trace"][0][5]                                # and it actually tracked
    assert tracking.flow_error(orc, sc, rg["kt"], rg["kR"]) < tracking.flow_error(orc, sc, sc["kt0"], sc["kR0"])


@pytest.mark.parametrize("kw", [dict(H=120, W=160, levels=3, S=8, k=2, seed=2), dict(H=480, W=640, levels=4, S=8, k=4, F=2, seed=7)])
def test_tracker_evaluation_paths_agree(orc, mbavo, gpu_ctx, kw):
    """The three ways an evaluation of the host-driven LM loop reaches the GPU -- commands to a persistent kernel (default),
    one single-launch kernel per evaluation (mbavo_engine_opts.persistent = -1), three launches per evaluation (single_launch = -1) -- run the same
    arithmetic per pixel and differ only in the order the tile partials are added (1e-16 per evaluation, amplified by the
    conditioning of the normal equations along the iterates): identical accept / reject / outlier traces; costs 1e-6 and knots 1e-4, the
    tolerances of the oracle comparison above (observed here: 1e-7 on the k = 4 scene, whose outer knots are weakly
    observed), on a small k = 2 scene and on the BASELINE-size two-frame k = 4 scene."""
    import tracking
    sc = tracking.make_tracking_scene(orc, **kw)
    runs = {}
    try:
        for name, eo in (("persistent", {}), ("one_launch", {"persistent": -1}), ("three_launches", {"persistent": -1, "single_launch": -1})):
            gpu_ctx.engine_opts(**eo)
            runs[name] = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(tracking.OPTS))
    finally:
        gpu_ctx.engine_opts()  # back to the defaults for the session's other tests
    ref = runs["persistent"]
    for name in ("one_launch", "three_launches"):
        r = runs[name]
        assert np.array_equal(ref["start"], r["start"]) and len(ref["trace"]) == len(r["trace"]), name
        for a, b in zip(ref["trace"], r["trace"]):
            assert a[:4] == b[:4], (name, a, b)
            assert a[5] == pytest.approx(b[5], rel=1e-6, abs=1e-12) and a[6] == pytest.approx(b[6], rel=1e-6, abs=1e-12)
        assert np.abs(ref["kt"] - r["kt"]).max() < 1e-4 and np.abs(ref["kR"] - r["kR"]).max() < 1e-4, name


@pytest.mark.parametrize("name,kw", [
    ("k2_semidense", dict(H=120, W=160, levels=3, S=8, k=2, seed=2)),
    ("k2_three_frames", dict(H=120, W=160, levels=2, S=4, k=2, F=3, seed=1)),
    ("k4_semidense_jacobi", dict(H=120, W=160, levels=3, S=8, k=4, seed=1)),
    ("k4_ldlt", dict(H=120, W=160, levels=3, S=8, k=4, seed=4)),
])
@pytest.mark.parametrize("fast_solve", ["1", "0"])
def test_lm_loop_shapes_and_solvers_match_oracle(orc, mbavo, gpu_ctx, name, kw, fast_solve):
    """The host-driven loop on the shapes the (removed, round 4) resident LM loop was held to -- three frames on one spline,
    k = 4 with the Jacobi SVD, solver type 1 -- against the oracle's loop, with the LDL^T stand-in of solver type 0 on
    (default) and off (mbavo_track_opts.fast_solve_ratio = -1: solve_normal_equation.h case 0 for every system): identical knot start indices,
    accept / reject / invalid sequence and outlier counts, costs 1e-6, poses at capture time 1e-5."""
    sc = tracking.make_tracking_scene(orc, **kw)
    opts = dict(tracking.OPTS)
    if "ldlt" in name:
        opts["solver_type"] = 1
    ro = tracking.run_oracle_tracker(orc, sc, opts)
    rg = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(opts, fast_solve_ratio=0.0 if fast_solve == "1" else -1.0))
    assert gpu_ctx.lib.mbavo_last_kernel(gpu_ctx.handle).decode().startswith("k_fused_sp<")
    assert np.array_equal(ro["start"], rg["start"]) and len(ro["trace"]) == len(rg["trace"])
    for a, b in zip(ro["trace"], rg["trace"]):
        assert a[:4] == b[:4], (a, b)
        assert a[4] == pytest.approx(b[4], rel=1e-4)
        assert a[5] == pytest.approx(b[5], rel=1e-6, abs=1e-12) and a[6] == pytest.approx(b[6], rel=1e-6, abs=1e-12)
    assert np.abs(ro["kt"] - rg["kt"]).max() < 1e-4 and np.abs(ro["kR"] - rg["kR"]).max() < 1e-4
    assert ro["cost"] == pytest.approx(rg["cost"], rel=1e-6)
    for c in sc["cap"]:
        po, qo = tracking.pose_at(orc, sc["k"], sc["t0"], sc["dt"], ro["kt"], ro["kR"], c)
        pg, qg = tracking.pose_at(orc, sc["k"], sc["t0"], sc["dt"], rg["kt"], rg["kR"], c)
        assert np.abs(po - pg).max() < 1e-5 and np.abs(qo - qg).max() < 1e-5


@pytest.mark.parametrize("kw", [dict(H=120, W=160, levels=3, S=8, k=2, seed=2), dict(H=480, W=640, levels=4, S=8, k=2, seed=5),
                                dict(H=480, W=640, levels=4, S=8, k=4, F=2, seed=7)])
def test_next_level_first_evaluation_rides_along(orc, mbavo, gpu_ctx, kw):
    """mbavo_track_opts.ride_along (default on): every candidate's command of the joint persistent kernel also evaluates the NEXT finer
    level at the current knots, and a level that ends at those knots (a rejected last candidate: A16) finds its successor's iteration 0
    done.  The evaluation is the one the loop would have made -- same kernel, same inputs -- so against the loop with it switched off:
    the same trace records to the last bit (costs included), the same knots, bit for bit; and the oracle's trace."""
    import tracking
    sc = tracking.make_tracking_scene(orc, **kw)
    on = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(tracking.OPTS))
    off = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(tracking.OPTS, ride_along=-1))
    assert on["trace"] == off["trace"] and len(on["trace"]) > 2 * kw["levels"]
    assert np.array_equal(on["kt"], off["kt"]) and np.array_equal(on["kR"], off["kR"]) and on["cost"] == off["cost"]
    want = tracking.run_oracle_tracker(orc, sc, dict(tracking.OPTS))
    assert [t[:4] for t in on["trace"]] == [t[:4] for t in want["trace"]]


@pytest.mark.parametrize("kw", [dict(H=120, W=160, levels=3, S=8, k=2, seed=2), dict(H=480, W=640, levels=4, S=8, k=2, seed=5),
                                dict(H=480, W=640, levels=4, S=8, k=4, F=2, seed=7), dict(H=480, W=640, levels=4, S=8, k=4, seed=11)])
def test_accepted_step_is_summed_again(orc, mbavo, gpu_ctx, kw):
    """mbavo_track_opts.resum (default on): an accepted step whose outlier detection flagged new patches does not evaluate its
    point again (blur_aware_direct_tracker.cpp:896-903 at the candidate's knots) -- the persistent kernel's workgroups add the
    candidate's per-patch sums up again under the new flags and the new residual scale.  Same leaves, same order of additions:
    against the loop with it switched off the trace records (costs included), the knots and the final cost are equal to the
    last bit; the steps that flag something exist in these scenes (outlier counts grow along the trace); and the oracle's trace."""
    import tracking
    sc = tracking.make_tracking_scene(orc, **kw)
    on = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(tracking.OPTS))
    off = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(tracking.OPTS, resum=-1))
    assert on["trace"] == off["trace"] and len(on["trace"]) > 2 * kw["levels"]
    assert np.array_equal(on["kt"], off["kt"]) and np.array_equal(on["kR"], off["kR"]) and on["cost"] == off["cost"]
    grew = sum(1 for a, b in zip(on["trace"], on["trace"][1:]) if b[2] == 1 and a[0] == b[0] and b[3] > a[3])
    assert grew >= 1, "no accepted step of this scene flags a new outlier: the test exercises nothing"
    want = tracking.run_oracle_tracker(orc, sc, dict(tracking.OPTS))
    assert [t[:4] for t in on["trace"]] == [t[:4] for t in want["trace"]]


@pytest.mark.parametrize("kw", [dict(H=480, W=640, levels=4, S=8, k=2, seed=5), dict(H=480, W=640, levels=4, S=8, k=2, seed=9),
                                dict(H=480, W=640, levels=4, S=8, k=4, seed=11), dict(H=240, W=320, levels=3, S=8, k=2, seed=3)])
def test_wasted_ride_along_is_waited_out(orc, mbavo, gpu_ctx, kw):
    """A ride-along taken at other knots than the level ends on shares the next level's ticket counters, tile partials and frame
    blocks with that level's first command, and the persistent kernel's workgroups take commands independently: the host must not
    post the command before the ride-along has finished (tracker.cpp).  ride_along = 2 treats EVERY ride-along as
    wasted, so every level but the coarsest starts behind one that may still be running, on levels of several tiles per slot
    (640x480: ~1000 / ~280 / ~150 keypoints).  Repeated, against the loop without ride-alongs: records with costs, knots and final
    cost to the last bit; the counters say the wait path ran and no ride-along was used."""
    import ctypes as C
    import tracking
    sc = tracking.make_tracking_scene(orc, **kw)
    off = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(tracking.OPTS, ride_along=-1))
    st = (C.c_longlong * 3)()
    gpu_ctx.lib.mbavo_ride_along_stats(st)
    for _ in range(12):
        got = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(tracking.OPTS, ride_along=2))
        assert got["trace"] == off["trace"] and got["cost"] == off["cost"]
        assert np.array_equal(got["kt"], off["kt"]) and np.array_equal(got["kR"], off["kR"])
    gpu_ctx.lib.mbavo_ride_along_stats(st)
    posts, hits, waits = list(st)
    if posts == 0:
        pytest.skip("this shape does not run on the joint persistent kernel: no ride-alongs to waste")
    # (a level that posts no candidate carries no ride-along: at most levels - 1 waits per run, the same number every run)
    assert hits == 0 and posts >= waits and waits % 12 == 0 and 12 <= waits <= 12 * (kw["levels"] - 1), (posts, hits, waits)
    on = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(tracking.OPTS))
    gpu_ctx.lib.mbavo_ride_along_stats(st)
    assert on["trace"] == off["trace"] and st[1] >= 1, list(st)  # (the default: ride-alongs are used where the knots match)


def test_out_of_range_call_leaves_the_context_as_it_was(orc, mbavo, gpu_ctx):
    """A capture time whose blur samples fall outside the knots: mbavo_optimize_trajectory returns MBAVO_E_RANGE (-2) from its host-side
    check, before the first launch.  The error leaves through the same guard as every other way out of the call: a valid call on the same
    context right after it returns what that call returns on a fresh context, bit for bit (records with costs, knots, final cost)."""
    import torch
    sc = tracking.make_tracking_scene(orc, H=120, W=160, levels=3, S=8, k=2, seed=2)
    late = dict(sc, cap=sc["cap"] + 10.0)
    ctxs = [mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream) for _ in range(2)]
    try:
        want = tracking.run_gpu_tracker(mbavo, ctxs[0], sc, dict(tracking.OPTS))
        tracking.run_gpu_tracker(mbavo, ctxs[1], late, dict(tracking.OPTS), want_error=-2)
        got = tracking.run_gpu_tracker(mbavo, ctxs[1], sc, dict(tracking.OPTS))
    finally:
        for c in ctxs:
            c.close()
    assert got["trace"] == want["trace"] and len(got["trace"]) > 2 * 3 and got["cost"] == want["cost"]
    assert np.array_equal(got["kt"], want["kt"]) and np.array_equal(got["kR"], want["kR"])


def test_two_trackers_at_once(orc, mbavo, gpu_ctx):
    """Two contexts (two engines, two streams, two push blocks, two pinned completion areas) driven from two host threads at the same
    time: each LM loop's persistent kernels, commands and re-summations must stay its own.  Every run returns what the same scene
    returns alone, bit for bit (records with costs, knots, final cost)."""
    import threading
    import torch
    import tracking
    scs = [tracking.make_tracking_scene(orc, H=240, W=320, levels=3, S=8, k=2, seed=21),
           tracking.make_tracking_scene(orc, H=120, W=160, levels=3, S=8, k=4, F=2, seed=22)]
    alone = [tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(tracking.OPTS)) for sc in scs]
    streams = [torch.cuda.Stream() for _ in scs]
    ctxs = [mbavo.capi.Context(0, stream=s.cuda_stream) for s in streams]
    out, err = [[] for _ in scs], []

    def work(i):
        try:
            for _ in range(4):
                out[i].append(tracking.run_gpu_tracker(mbavo, ctxs[i], scs[i], dict(tracking.OPTS)))
        except BaseException as e:  # noqa: BLE001 (reported below, in the test's thread)
            err.append(repr(e))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(scs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a tracker did not return"
    assert not err, err
    for i, want in enumerate(alone):
        assert len(out[i]) == 4
        for got in out[i]:
            assert got["trace"] == want["trace"] and got["cost"] == want["cost"]
            assert np.array_equal(got["kt"], want["kt"]) and np.array_equal(got["kR"], want["kR"])
    for c in ctxs:
        c.close()
