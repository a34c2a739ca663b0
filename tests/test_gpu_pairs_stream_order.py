"""The pairs batch and the per-image entries around it on a BUSY stream: every case makes its calls once with the stream idle
(inputs in place, synchronised before and after every call) and once behind a gate, with the inputs arriving late on the stream and
the host arguments overwritten the moment their call has returned, and asserts that the results are the same bits
(tests/stream_backlog.py).  The oracle is invariance to the stream's state; agreement with numpy and the CPU oracle is what the
other pairs tests assert on an idle stream.  The context lives on its own torch pool stream, which the null stream orders nothing
for, so a launch or copy on stream 0, a missing wait on the LM fork or a mirror refilled too early gives other bits here.

Shapes: B = 3, L = 3, 60 x 80 for the objects, 75 x 101 for the per-image entries, k = 2 and k = 4 where kernels are templated on it."""
import ctypes as C

import numpy as np
import pytest

import pairs_cases
import pairs_depth_cases as dc
import pairs_depth_support as ds
import pairs_device as dv
import pairs_points_ref as pref
import pairs_ref
import pairs_step as ps
import pairs_track as pt
import pairs_undistort_ref as uref
import pairs_unified_ref as nref
import scenes
import stream_backlog as sb
from lm_support import lm_batch_opts
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

B, L, H, W = 3, 3, 60, 80
HI, WI = 75, 101
THRESHOLDS = (ps.FLOW0, ps.FLOW1, ps.KERNEL)


@pytest.fixture(scope="module")
def own(mbavo):
    """(S, ctx): a context on its own non-blocking stream."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    S, ctx = sb.own_stream_context(mbavo.capi)
    yield S, ctx
    S.synchronize()
    ctx.close()


def _late_set(real, stale):
    """(device tensor, pinned real, pinned stale) of two arrays of one shape."""
    assert real.shape == stale.shape and real.dtype == stale.dtype and not np.array_equal(real, stale)
    p = sb.pinned(real)
    return sb.device_like(p), p, sb.pinned(stale)


def _zeros(shape, dtype):
    import torch
    t = torch.zeros(shape, dtype=dtype, device="cuda:0")
    torch.cuda.synchronize()
    return t


def _ok(rc):
    assert rc == 0, rc
    return rc


# ---------------------------------------------------------------------------------------------------------------- a, b: per-image entries
def test_a_image_entries_on_their_own_stream_argument(mbavo, own):
    """Case a: pyramid_down, the three gradient formats and the magnitude, each given S, with the source image late."""
    import torch
    S, ctx = own
    lib = ctx.lib
    real, stale = (synth.texture_image(HI, WI, seed=s, octaves=(16, 8, 4)) for s in (3, 4))
    src = _late_set(real, stale)
    outs = dict(down=_zeros((HI // 2, WI // 2), torch.uint8), grad=_zeros((HI, WI, 2), torch.float32), half=_zeros((HI, WI, 2), torch.int16),
                pack=_zeros((HI, WI), torch.int32), mag=_zeros((HI, WI), torch.float32))
    entries = dict(down=lib.mbavo_pyramid_down_u8, grad=lib.mbavo_image_gradients_u8, half=lib.mbavo_image_gradients_u8_half,
                   pack=lib.mbavo_pack_keyframe_u8, mag=lib.mbavo_gradient_magnitude_u8)

    def seq(run):
        run.place([src], outputs=outs.values())
        for name, fn in entries.items():
            run.call(name, lambda: _ok(fn(src[0].data_ptr(), HI, WI, outs[name].data_ptr(), C.c_void_p(S.cuda_stream))), asserted=True)
        run.finish()
        return dict(outs)

    got = sb.run_case("a per-image entries, own stream argument", S, seq)
    assert got["down"] == synth.pyramid(real, 2)[1].tobytes()
    assert got["grad"] == synth.image_gradients(real).tobytes()
    assert got["pack"] == np.ascontiguousarray(synth.pack_keyframe(real)).tobytes()
    assert got["half"] == synth.image_gradients(real).astype(np.float16).tobytes()
    assert got["mag"] == pairs_ref.gradient_magnitude(real).tobytes()


def test_b_image_entries_on_the_context_stream(mbavo, own):
    """Case b: pyramid_levels, depth_to_z in formats 1 and 2 with their sources late and the pointer and intrinsics arrays
    overwritten after the return; undistort_map_batch twice under one gate with two camera sets into two outputs."""
    import torch
    from mba_vo_amd import workloads
    S, ctx = own
    lib, capi = ctx.lib, mbavo.capi
    real, stale = (synth.texture_image(HI, WI, seed=s, octaves=(16, 8, 4)) for s in (5, 6))
    lvl0 = _late_set(real, stale)
    levels = [_zeros((HI >> l, WI >> l), torch.uint8) for l in (1, 2)]
    other_levels = [_zeros((HI >> l, WI >> l), torch.uint8) for l in (1, 2)]  # where the overwritten pointer array points
    ptrs = lambda ts: np.array([lvl0[0].data_ptr()] + [t.data_ptr() for t in ts], np.uint64)
    ray = _late_set(pairs_cases.raw_depth(1, 1, HI, WI, seed=11, beyond=80.0)[0], pairs_cases.raw_depth(1, 1, HI, WI, seed=12, beyond=80.0)[0])
    u16 = _late_set(pairs_cases.raw_depth(2, 1, HI, WI, seed=13)[0], pairs_cases.raw_depth(2, 1, HI, WI, seed=14)[0])
    z1, z2 = _zeros((HI, WI), torch.float32), _zeros((HI, WI), torch.float32)
    intr = (np.array([WI / 2.0, WI / 2.0, WI / 2.0, HI / 2.0]), np.array([WI / 1.7, WI / 1.9, WI / 2.2, HI / 1.8]))
    c = pairs_cases.undistort_case("crop", "outside")
    cam = lambda dist, to: workloads.pairs_camera(pairs_cases.undistort_camera(c, dist), to)
    to2 = tuple(v * 1.05 for v in c["intr"])
    set_a = (capi.PairsCamera * 2)(cam("outside", c["intr"]), cam("inside", to2))
    set_b = (capi.PairsCamera * 2)(cam("inside", c["intr"]), cam("none", to2))
    maps = [_zeros((2, c["H"], c["W"], 2), torch.float32) for _ in range(2)]
    rng = np.random.default_rng(21)
    raw_points = lambda: np.ascontiguousarray(np.stack([rng.uniform(0, c["Ws"] - 1, 12), rng.uniform(0, c["Hs"] - 1, 12)], 1))
    uv = _late_set(raw_points(), raw_points())
    offsets = (np.array([0, 5, 12], np.int32), np.array([0, 7, 12], np.int32))
    xy, ok = [_zeros((12, 2), torch.float64) for _ in range(2)], [_zeros((12,), torch.uint8) for _ in range(2)]

    def seq(run):
        run.place([lvl0, ray, u16, uv], outputs=levels + other_levels + [z1, z2] + maps + xy + ok)
        p, over = run.host(ptrs(levels), ptrs(other_levels))
        run.call("pyramid_levels", lambda: _ok(lib.mbavo_pyramid_levels_u8(ctx.handle, p.ctypes.data_as(C.POINTER(C.c_void_p)), HI, WI, 3)), after=over)
        k1, over = run.host(*intr)
        run.call("depth_to_z 1", lambda: _ok(lib.mbavo_depth_to_z(ctx.handle, 1, ray[0].data_ptr(), HI, WI, capi.dp(k1), 0.0, 50.0, z1.data_ptr())),
                 after=over, asserted=True)
        k2, over = run.host(*intr)
        run.call("depth_to_z 2", lambda: _ok(lib.mbavo_depth_to_z(ctx.handle, 2, u16[0].data_ptr(), HI, WI, capi.dp(k2), 0.0002, 0.0, z2.data_ptr())),
                 after=over, asserted=True)
        ca, over = run.host(set_a, set_b)
        run.call("map_batch first", lambda: _ok(lib.mbavo_undistort_map_batch(ctx.handle, 2, ca, c["H"], c["W"], maps[0].data_ptr())), after=over)
        run.regate()  # (a pageable array: the runtime may have waited; the second call must still find a backlog)
        cb, over = run.host(set_b, set_a)
        run.call("map_batch second", lambda: _ok(lib.mbavo_undistort_map_batch(ctx.handle, 2, cb, c["H"], c["W"], maps[1].data_ptr())), after=over)
        for i, (cams, offs) in enumerate((((set_a, set_b), offsets), ((set_b, set_a), offsets[::-1]))):
            run.regate()
            cp, over_c = run.host(*cams)
            of, over_o = run.host(*offs)
            run.call("points_batch %d" % i, lambda: _ok(lib.mbavo_undistort_points_batch(ctx.handle, 2, cp, capi.ip(of), uv[0].data_ptr(), xy[i].data_ptr(),
                                                                                         ok[i].data_ptr())), after=lambda: (over_c(), over_o()))
        run.finish()
        lv = other_levels if run.which == "stale" else levels
        return dict(level1=lv[0], level2=lv[1], z1=z1, z2=z2, maps=torch.stack(maps), points=torch.stack(xy))

    got = sb.run_case("b per-image entries, context's stream", S, seq)
    pyr = synth.pyramid(real, 3)
    assert got["level1"] == pyr[1].tobytes() and got["level2"] == pyr[2].tobytes()


# ---------------------------------------------------------------------------------------------------------------- c: object set-up
def _pairs_inputs(seed):
    sharp, depth, blur = pairs_cases.inputs(B, H, W, seed=seed, special=False)
    return dict(sharp=sharp, depth=depth, blur=blur)


def _object(ctx, k, N, **kw):
    from mba_vo_amd import workloads
    return workloads.PairBatch(ctx, B, L=L, H=H, W=W, k=k, N=N, cell=ps.CELL, thresh=ps.THR, border=4, **kw)


def test_c_prepare_and_update_with_late_images(mbavo, own):
    """Case c (the object without cameras or masks): prepare with images and depth maps late, then update with a key list and new
    frames late; the key list is overwritten after the return.  What the object holds is the idle run's."""
    S, ctx = own
    a, b = _pairs_inputs(1), _pairs_inputs(2)
    first = {key: _late_set(a[key], b[key]) for key in ("sharp", "depth", "blur")}
    n_key = 2
    nxt = dict(blur=_late_set(b["blur"], a["blur"]), sharp=_late_set(b["sharp"][:n_key], a["sharp"][:n_key]),
               depth=_late_set(b["depth"][:n_key], a["depth"][:n_key]))
    keys = (np.array([0, 2], np.int32), np.array([1, 2], np.int32))
    pb = _object(ctx, 4, 4)
    try:
        def seq(run):
            run.place(list(first.values()))
            counts = np.zeros((B, L), np.int32)
            run.call("prepare", lambda: _ok(ctx.lib.mbavo_pairs_prepare(pb.handle, first["sharp"][0].data_ptr(), first["depth"][0].data_ptr(),
                                                                       first["blur"][0].data_ptr(), mbavo.capi.ip(counts))))
            after_prepare = counts.copy()
            run.place(list(nxt.values()))  # (prepare reads its counts back: the update gets a backlog and late inputs of its own)
            kl, over = run.host(*keys)
            run.call("update", lambda: _ok(ctx.lib.mbavo_pairs_update(pb.handle, nxt["blur"][0].data_ptr(), n_key, mbavo.capi.ip(kl), nxt["sharp"][0].data_ptr(),
                                                                     nxt["depth"][0].data_ptr(), mbavo.capi.ip(counts))), after=over)
            run.finish()
            got = dv.read_batch(pb, counts)
            return dict(counts=after_prepare.tobytes() + counts.tobytes(), **{key: b"".join(g[key].tobytes() for g in got) for key in ("ref", "cur", "grad", "xy", "z")})

        sb.run_case("c prepare, update with a key list", S, seq)
    finally:
        pb.close()


# ---------------------------------------------------------------------------------------------------------------- d, e: frame step, LM
def _track_object(mbavo, ctx, k):
    case = ps.assess_inputs(B, H, W, k)
    pb = _object(ctx, k, ps.N_KNOTS)
    pb.prepare(*dv.dev(case["sharp"], case["depth"], case["blur"]))
    return pb, case, pt.make_states(mbavo.capi, case)


def _times(case):
    """(cap, exp) of the real and of the other valid set: both on the knots (predict starts the spline at cap - exp / 2)."""
    return (case["cap"].copy(), case["cap"] + 0.03), (case["exp"].copy(), case["exp"] * 1.5)


@pytest.mark.parametrize("k", [2, 4])
def test_d_predict_then_commit(mbavo, own, k):
    """Case d: after set_states, predict and commit under one gate; cap and exp are overwritten once predict has returned."""
    S, ctx = own
    pb, case, states = _track_object(mbavo, ctx, k)
    caps, exps = _times(case)
    try:
        def seq(run):
            assert pb.set_states(states) == 0
            run.place()
            cap, over_c = run.host(*caps)
            exp, over_e = run.host(*exps)
            run.call("predict", lambda: _ok(pb.predict(cap, exp)), after=lambda: (over_c(), over_e()), asserted=True)
            frames = run.call("commit", lambda: pb.commit(*THRESHOLDS), about=False)
            run.finish()
            return dict(frames=bytes(frames), states=bytes(pb.get_states()))

        sb.run_case("d predict, commit (k = %d)" % k, S, seq)
    finally:
        pb.close()


def test_d_hypotheses_without_records_then_commit(mbavo, own):
    """Case d: predict_hypotheses with a NULL out, times and options overwritten after its return, then commit."""
    S, ctx = own
    pb, case, states = _track_object(mbavo, ctx, 4)
    caps, exps = _times(case)
    tw = [None, (0.02, -0.01, 0.015, 0.004, -0.003, 0.002)]
    opts = (pb.hyp_opts([0.5, 1.0], tw, level=L - 1), pb.hyp_opts([1.7, 0.3], tw[::-1], level=L - 2))
    try:
        def seq(run):
            assert pb.set_states(states) == 0
            run.place()
            cap, over_c = run.host(*caps)
            exp, over_e = run.host(*exps)
            o, over_o = run.host(*opts)
            run.call("hypotheses", lambda: _ok(ctx.lib.mbavo_pairs_predict_hypotheses(pb.handle, mbavo.capi.dp(cap), mbavo.capi.dp(exp), C.byref(o), None)),
                     after=lambda: (over_c(), over_e(), over_o()), asserted=True)
            frames = run.call("commit", lambda: pb.commit(*THRESHOLDS), about=False)
            run.finish()
            return dict(frames=bytes(frames), states=bytes(pb.get_states()))

        sb.run_case("d hypotheses (NULL), commit", S, seq)
    finally:
        pb.close()


def test_d_track_three_frames_with_late_images(mbavo, own):
    """Case d: mbavo_pairs_track_frame for three frames, each frame's blurred images late behind a gate of its own (the call reads
    its records back, so every frame finds the stream drained)."""
    S, ctx = own
    capi = mbavo.capi
    k = 4
    pb, case, states = _track_object(mbavo, ctx, k)
    rolled = lambda im, f: np.ascontiguousarray(np.roll(im, (f + 1, 2 * f + 1), (1, 2)))
    other = ps.assess_inputs(B, H, W, k, seed=77)["blur"]
    frames_in = [_late_set(rolled(case["blur"], f), rolled(other, f)) for f in range(3)]
    lm = lm_batch_opts(capi, k, 3)
    try:
        def seq(run):
            assert pb.set_states(states) == 0
            out = []
            for f, blur in enumerate(frames_in):
                run.place([blur])
                cap, over_c = run.host(case["cap"] + 0.1 * f, case["cap"] + 0.1 * f + 0.03)
                exp, over_e = run.host(case["exp"], case["exp"] * 1.5)
                fr, counts, res, _ = run.call("frame %d" % f, lambda: pb.track_frame(blur[0], cap, exp, lm, THRESHOLDS), after=lambda: (over_c(), over_e()))
                out.append(bytes(fr) + bytes(res))
            run.finish()
            return dict(frames=b"".join(out), states=bytes(pb.get_states()))

        sb.run_case("d track_frame x 3", S, seq)
    finally:
        pb.close()


def test_d_assess_after_set_motion(mbavo, own):
    """Case d: set_motion and assess under one gate, every array of the motion overwritten once set_motion has returned."""
    S, ctx = own
    k = 4
    case = ps.assess_inputs(B, H, W, k)
    pb = _object(ctx, k, ps.N_KNOTS)
    pb.prepare(*dv.dev(case["sharp"], case["depth"], case["blur"]))
    sets = ((case["cap"], case["cap"] + 0.01), (case["exp"], case["exp"] * 1.5), (case["t0"], case["t0"].copy()),
            (case["kt"], case["kt"] * 0.5), (case["kR"], np.ascontiguousarray(case["kR"][::-1])))
    try:
        def seq(run):
            run.place()
            args, overs = zip(*[run.host(np.ascontiguousarray(r, np.float64), np.ascontiguousarray(s, np.float64)) for r, s in sets])
            cap, exp, t0, kt, kR = args
            run.call("set_motion", lambda: _ok(pb.set_motion(cap, exp, t0, case["dt"], kt, kR)), after=lambda: [o() for o in overs])
            out = run.call("assess", lambda: pb.assess(*THRESHOLDS), about=False)
            run.finish()
            kt_now, kR_now = pb.knots()
            return dict(assessment=bytes(out), knots=kt_now.tobytes() + kR_now.tobytes())

        sb.run_case("d set_motion, assess", S, seq)
    finally:
        pb.close()


@pytest.mark.parametrize("levels", [False, True])
def test_e_lm_behind_a_predict(mbavo, own, levels):
    """Case e: predict, then the batched LM in two groups on the object's problems under one gate: the predicted knots the LM
    starts from are still queued when the groups fork.  mbavo_lm_batch on the level-0 problems, mbavo_lm_batch_levels on all."""
    S, ctx = own
    capi = mbavo.capi
    k = 4
    pb, case, states = _track_object(mbavo, ctx, k)
    caps, exps = _times(case)
    lm = lm_batch_opts(capi, k, 6, groups=2)
    level0 = (capi.Problem * B)()
    try:
        def seq(run):
            assert pb.set_states(states) == 0
            run.place()
            cap, over_c = run.host(*caps)
            exp, over_e = run.host(*exps)
            res = (capi.LmBatchResult * B)()
            run.call("predict", lambda: _ok(pb.predict(cap, exp)), after=lambda: (over_c(), over_e()), asserted=True, about=False)
            if levels:
                run.call("lm_batch_levels", lambda: _ok(ctx.lib.mbavo_lm_batch_levels(ctx.handle, B, L, pb.array, C.byref(lm), res, None, 0)))
            else:
                for b in range(B):  # (the problems as they are after the predict's host side: t0 and the start index)
                    level0[b] = pb.array[b * L]
                run.call("lm_batch", lambda: _ok(ctx.lib.mbavo_lm_batch(ctx.handle, B, level0, C.byref(lm), res, None, 0)))
            run.finish()
            kt, kR = pb.knots()
            return dict(results=bytes(res), knots=kt.tobytes() + kR.tobytes())

        sb.run_case("e predict, %s in two groups" % ("lm_batch_levels" if levels else "lm_batch"), S, seq)
    finally:
        pb.close()


# ---------------------------------------------------------------------------------------------------------------- f: depth stages
def _both(real, **changes):
    return real, dict(real, **changes)


@pytest.mark.parametrize("k", [2, 4])
def test_f_depth_stages_without_records(mbavo, own, k):
    """Case f: refine, filter, search and smooth, each twice in a row with other options or level, carry save and adopt and a prune
    without apply under one gate, every call with h_out_or_null == NULL; options structs, pair lists and poses are overwritten after
    each return.  Then one synchronising read: depths, filter state, the prune's keep bytes, a report."""
    import torch
    S, ctx = own
    capi, lib = mbavo.capi, ctx.lib
    N = 4
    inp = _pairs_inputs(3)
    inp["depth"] = np.where(inp["depth"] < 0.01, inp["depth"], np.float32(1.0) + inp["depth"] * np.float32(0.5))  # (1.25 .. 2.5 beside the holes)
    m = dc.harness_motion(B, N)
    pb = _object(ctx, k, N, S=3)
    dev = dv.dev(inp["sharp"], inp["depth"], inp["blur"])
    keep = _zeros((B, sum(pb.capacities())), torch.uint8)

    def opts(cls, **kw):
        o = cls()
        for key, v in kw.items():
            setattr(o, key, v)
        return o

    O = capi
    refine = [_both(dict(level=0, apply=1, min_info=150.0, max_rel_step=0.25), apply=0, min_info=0.0, max_rel_step=0.01),
              _both(dict(level=1, apply=1, max_rel_step=0.1), apply=0)]
    filt = [_both(dict(level=-1, apply=1, prior_rel_sigma=0.1, sigma_i=2.0, gate_chi2=9.0), apply=0, sigma_i=6.0, prior_rel_sigma=0.3),
            _both(dict(level=-1, apply=1, prior_rel_sigma=0.1, sigma_i=3.0, gate_chi2=4.0), sigma_i=1.0, gate_chi2=0.0)]
    search = [_both(dict(level=0, apply=1, num_candidates=6, relative=0, rho_lo=0.3, rho_hi=1.1), apply=0, rho_lo=0.5, rho_hi=0.7),
              _both(dict(level=1, apply=1, num_candidates=5, relative=1, rho_lo=0.6, rho_hi=1.5, min_ratio=1.02), relative=0, rho_lo=0.2, rho_hi=0.9)]
    smooth = [_both(dict(level=0, apply=1, fill=1, radius=3, min_support=2, max_rel_diff=0.1, strength=0.7), apply=0, radius=5, strength=0.2),
              _both(dict(level=-1, apply=1, fill=0, radius=2, min_support=1, max_rel_diff=0.2, strength=0.5), radius=6, strength=1.0, fill=1)]
    save = _both(dict(radius=2, deflate=0.8), radius=4, deflate=0.5)
    adopt = _both(dict(apply=1, min_support=1, max_rel_diff=0.1), apply=0, max_rel_diff=0.5)
    prune = _both(dict(level=-1, apply=0, check_depth=1, z_min=1.3, z_max=2.2), z_min=1.6, z_max=1.9)
    pairs = (np.array([0, 2], np.int32), np.array([0, 1], np.int32))
    poses = (np.stack([dc.TILT, dc.rounds_poses()[1]]), np.stack([dc.rounds_poses()[1], dc.TILT]))
    null = None
    try:
        def seq(run):
            pb.prepare(*dev)  # (the object as new: depths, keypoints, the filter seeded anew)
            assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
            with torch.cuda.stream(S):
                keep.zero_()
            run.place()

            def stage(label, entry, cls, pair, extra=(), asserted=True):
                o, over = run.host(opts(cls, **pair[0]), opts(cls, **pair[1]))
                run.call(label, lambda: _ok(entry(pb.handle, C.byref(o), null, *extra)), after=over, asserted=asserted)

            # the first call of a stage must leave the backlog in place; the second waits until the first one's options have left the
            # stage's mirror, which takes the gate away (the first call's kernel may still be queued): every stage gets its own gate
            for name, entry, cls, two, extra in (("refine", lib.mbavo_pairs_refine_depths, O.PairsRefineOpts, refine, (null,) * 4),
                                                 ("filter", lib.mbavo_pairs_filter_depths, O.PairsFilterOpts, filt, ()),
                                                 ("search", lib.mbavo_pairs_search_depths, O.PairsSearchOpts, search, (null,) * 7),
                                                 ("smooth", lib.mbavo_pairs_smooth_depths, O.PairsSmoothOpts, smooth, (null,) * 4)):
                if name != "refine":
                    run.regate(always=True)
                stage(name + " first", entry, cls, two[0], extra, asserted=True)
                stage(name + " second", entry, cls, two[1], extra, asserted=False)
            run.regate(always=True)
            pl, over_p = run.host(*pairs)
            T, over_T = run.host(*poses)
            o, over_o = run.host(opts(O.PairsCarrySaveOpts, **save[0]), opts(O.PairsCarrySaveOpts, **save[1]))
            run.call("carry_save", lambda: _ok(lib.mbavo_pairs_carry_save(pb.handle, 2, capi.ip(pl), capi.dp(T), C.byref(o), null)),
                     after=lambda: (over_p(), over_T(), over_o()), asserted=True)
            pl2, over_p = run.host(*pairs)
            o2, over_o2 = run.host(opts(O.PairsCarryAdoptOpts, **adopt[0]), opts(O.PairsCarryAdoptOpts, **adopt[1]))
            run.call("carry_adopt", lambda: _ok(lib.mbavo_pairs_carry_adopt(pb.handle, 2, capi.ip(pl2), C.byref(o2), null, null, null, null, null)),
                     after=lambda: (over_p(), over_o2()))  # (save's mirror: the call waits until save's options and list have left it)
            run.regate(always=True)
            pl3, over_p3 = run.host(*pairs)
            o3, over_o3 = run.host(opts(O.PairsPruneOpts, **prune[0]), opts(O.PairsPruneOpts, **prune[1]))
            run.call("prune", lambda: _ok(lib.mbavo_pairs_prune_keypoints(pb.handle, 2, capi.ip(pl3), C.byref(o3), null, null, keep.data_ptr())),
                     after=lambda: (over_p3(), over_o3()), asserted=True)
            run.finish()
            st, _ = ds.filter_state(pb)
            return dict(depths=b"".join(z.tobytes() for z in ds.depths(pb)), filter=b"".join(st[key].tobytes() for key in ("mu", "info", "n_obs", "n_rej")),
                        keep=keep, report=bytes(pb.report(3.0)))

        sb.run_case("f depth stages with NULL records (k = %d)" % k, S, seq)
    finally:
        pb.close()


# ---------------------------------------------------------------------------------------------------------------- h: brightness match
@pytest.mark.parametrize("k", [2, 4])
def test_h_match_brightness_then_lm(mbavo, own, k):
    """Case h: the blurred frames of an update late; then match_brightness(apply = 1) and match_brightness(report only, other level,
    rounds and Huber threshold), both with h_out_or_null == NULL and their options struct overwritten the moment the call has
    returned (the options travel through a pinned mirror; R + 1 + 1 + ceil((L - 1) / 3) launches follow the first call); then the
    batched LM in two groups, which forks streams behind the corrected frames, and a report.  Then one synchronising read: a
    brightness fit of what is left with records, the report, the knots and every level of the current frames.  (On these inputs,
    random depths, six LM iterations move most patches out of view: the fit behind the LM is degenerate on most pairs.  What the
    two matching calls did shows in the current frames and in everything the LM and the report made of them.)"""
    import pairs_photo_ref as phref
    S, ctx = own
    capi, lib = mbavo.capi, ctx.lib
    N = 4
    inp, other = _pairs_inputs(3), _pairs_inputs(4)
    inp["depth"] = np.where(inp["depth"] < 0.01, inp["depth"], np.float32(1.0) + inp["depth"] * np.float32(0.5))
    m = dc.harness_motion(B, N)
    pb = _object(ctx, k, N, S=3)
    dev = dv.dev(inp["sharp"], inp["depth"], inp["blur"])
    exposure = [(1.3, -20.0), (0.7, 15.0), (1.0, 0.0)]
    frames = _late_set(np.stack([phref.exposed(inp["blur"][b], *exposure[b]) for b in range(B)]),
                       np.stack([phref.exposed(other["blur"][b], *exposure[(b + 1) % B]) for b in range(B)]))
    first = (phref.opts_struct(capi, level=1, apply=1, rounds=2, min_pixels=8), phref.opts_struct(capi, level=0, apply=1, rounds=4, min_pixels=8, gain_max=1.1))
    second = (phref.opts_struct(capi, level=0, apply=0, rounds=3, min_pixels=8, huber=6.0), phref.opts_struct(capi, level=2, apply=1, rounds=1, min_pixels=8))
    lm = lm_batch_opts(capi, k, 6, groups=2)
    try:
        def seq(run):
            counts = pb.prepare(*dev)  # (the object as new)
            assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
            run.place([frames])
            again = np.zeros((B, L), np.int32)
            run.call("update", lambda: _ok(lib.mbavo_pairs_update(pb.handle, frames[0].data_ptr(), 0, None, None, None, capi.ip(again))), about=False)
            run.regate()  # (where the update has waited for its counts, the calls this case is about get a backlog of their own)
            o1, over1 = run.host(*first)
            run.call("match apply", lambda: _ok(lib.mbavo_pairs_match_brightness(pb.handle, C.byref(o1), None)), after=over1, asserted=True)
            o2, over2 = run.host(*second)
            # (the second call waits until the first one's options have left the stage's mirror, which may take the gate away)
            run.call("match report", lambda: _ok(lib.mbavo_pairs_match_brightness(pb.handle, C.byref(o2), None)), after=over2, asserted=False)
            run.regate(always=True)
            res = (capi.LmBatchResult * B)()
            run.call("lm_batch_levels", lambda: _ok(lib.mbavo_lm_batch_levels(ctx.handle, B, L, pb.array, C.byref(lm), res, None, 0)))
            rep = run.call("report", lambda: pb.report(3.0), about=False)
            run.finish()
            rc, rec = pb.match_brightness(level=0, rounds=1, min_pixels=8)
            assert rc == 0 and np.array_equal(again, counts)
            kt, kR = pb.knots()
            got = dv.read_batch(pb, counts)
            print("h %s %s: what is left at level 0 after the LM: %s" % (run.mode, run.which, [(r.status, r.num_full, round(r.gain, 4), round(r.offset, 2)) for r in rec]))
            # (the fit behind the LM and the report in one entry: where the LM has moved a pair's patches out of view, its fit is degenerate for any frame)
            return dict(records=bytes(rec) + bytes(rep), results=bytes(res), knots=kt.tobytes() + kR.tobytes(), frames=b"".join(g["cur"].tobytes() for g in got))

        real = sb.run_case("h update, match_brightness apply and report with NULL records, LM, report (k = %d)" % k, S, seq)
        assert real["frames"] != b"".join(synth.pyramid(f, L)[l].tobytes() for f in frames[1].numpy() for l in range(L))  # (some pair was corrected)
    finally:
        pb.close()


# ---------------------------------------------------------------------------------------------------------------- g: evaluation
@pytest.mark.parametrize("k", [2, 4])
def test_g_evaluation_with_late_inputs(mbavo, own, k):
    """Case g: mbavo_eval_batch and mbavo_eval_batch_merged at K = 60 with images, keypoints, depths and knots late.  The keypoints
    lie over the whole image and past its border, so that the two sets' counts of in-bounds pixels differ as well."""
    import torch
    S, ctx = own
    capi = mbavo.capi
    mk = lambda seed: [scenes.Scene(H=H, W=W, S=3, F=2, k=k, N=5, P=8, K=60, seed=seed + 10 * b, kp="border", z_range=(2.0, 4.0)) for b in range(2)]
    real, stale = mk(1), mk(2)
    dsc = [scenes.DeviceScene(sc) for sc in real]
    buffers = []
    for d, r, s in zip(dsc, real, stale):
        assert r.N == s.N and np.array_equal(r.start_idx, s.start_idx)
        buffers += [(d.ref, r.ref, s.ref), (d.grad, r.grad, s.grad), (d.kp_xy, r.kp_xy, s.kp_xy), (d.kp_z, r.kp_z, s.kp_z),
                    (d.knots_t, r.knots_t, s.knots_t), (d.knots_R, r.knots_R, s.knots_R)] + [(d.cur[f], r.cur[f], s.cur[f]) for f in range(2)]
    buffers = [(t, sb.pinned(r), sb.pinned(s)) for t, r, s in buffers]
    arr = (capi.Problem * 2)(*[d.problem() for d in dsc])
    E, nbf = synth.packed_len(k), 4
    fb, fb2 = _zeros(nbf * E, torch.float64), _zeros(nbf * E, torch.float64)
    pc, valid = _zeros(nbf * 60, torch.float64), _zeros(nbf, torch.float64)
    systems = _zeros(2 * ctx.lib.mbavo_system_len(5), torch.float64)

    def seq(run):
        run.place(buffers, outputs=[fb, fb2, pc, valid, systems])
        run.call("eval_batch", lambda: _ok(ctx.lib.mbavo_eval_batch(ctx.handle, 2, arr, k, 1, fb.data_ptr(), pc.data_ptr(), valid.data_ptr())), asserted=True)
        run.call("eval_batch_merged", lambda: _ok(ctx.lib.mbavo_eval_batch_merged(ctx.handle, 2, arr, k, fb2.data_ptr(), systems.data_ptr(), None, None)))
        run.finish()
        return dict(blocks=fb, patch_cost=pc, valid=valid, blocks_merged=fb2, systems=systems)

    sb.run_case("g eval_batch, eval_batch_merged (k = %d)" % k, S, seq)


# ---------------------------------------------------------------------------------------------------------------- b: maps, remaps, clearance, masks
def test_b_undistort_entries_on_the_context_stream(mbavo, own):
    """Case b, the camera entries at 75 x 101: mbavo_undistort_map and _map_unified with the camera and the intrinsics overwritten after
    the return; mbavo_undistort_u8, _u8_batch, _clearance_batch, _mask_batch and mbavo_mask_clearance_batch, which take no host array,
    with raw images, maps and masks late and the backlog asserted after each."""
    import torch
    from mba_vo_amd import workloads
    S, ctx = own
    lib, capi = ctx.lib, mbavo.capi
    K = uref.intrinsics(HI, WI)
    to = (np.array(K, np.float64), np.array([K[0] * 1.03, K[1] * 1.03, K[2], K[3]], np.float64))
    radtan = tuple(workloads.camera_radtan(HI, WI, K, d) for d in (uref.DIST_OUTSIDE, uref.DIST_INSIDE))
    uni = lambda name: workloads.camera_unified(HI, WI, nref.from_intrinsics(name, "same", HI, WI), nref.SETS[name]["xi"], nref.SETS[name]["dist"])
    unified = (uni("inside"), uni("pinhole"))
    host_maps = [uref.undistort_map(K, d, K, HI, WI) for d in (uref.DIST_OUTSIDE, uref.DIST_INSIDE)]
    maps = _late_set(np.stack(host_maps), np.stack(host_maps[::-1]))
    tex = lambda seed: np.stack([synth.texture_image(HI, WI, seed=seed + i, octaves=(16, 8, 4)) for i in range(2)])
    imgs = _late_set(tex(30), tex(40))
    rng = np.random.default_rng(8)
    blocks = lambda: np.ascontiguousarray(np.kron((rng.uniform(size=(2, 15, 21)) > 0.2).astype(np.uint8) * 200, np.ones((5, 5), np.uint8))[:, :HI, :WI])
    raw_masks, und_masks = _late_set(blocks(), blocks()), _late_set(blocks(), blocks())
    nbytes = int(lib.mbavo_undistort_clearance_bytes(HI, WI, L))
    out = dict(map=_zeros((HI, WI, 2), torch.float32), map_unified=_zeros((HI, WI, 2), torch.float32), u8=_zeros((HI, WI), torch.uint8),
               u8_batch=_zeros((2, HI, WI), torch.uint8), clearance=_zeros((2, nbytes), torch.uint8), mask=_zeros((2, HI, WI), torch.uint8),
               mask_clearance=_zeros((2, nbytes), torch.uint8))
    ptr = lambda t: t.data_ptr()

    def seq(run):
        run.place([maps, imgs, raw_masks, und_masks], outputs=out.values())
        cam, over_c = run.host(*radtan)
        k, over_k = run.host(*to)
        run.call("map", lambda: _ok(lib.mbavo_undistort_map(ctx.handle, C.byref(cam), capi.dp(k), HI, WI, ptr(out["map"]))), after=lambda: (over_c(), over_k()))
        run.regate()
        ucam, over_u = run.host(*unified)
        k2, over_k2 = run.host(*to)
        run.call("map_unified", lambda: _ok(lib.mbavo_undistort_map_unified(ctx.handle, C.byref(ucam), capi.dp(k2), HI, WI, ptr(out["map_unified"]))),
                 after=lambda: (over_u(), over_k2()))
        run.regate()
        m, im = ptr(maps[0]), ptr(imgs[0])
        run.call("u8", lambda: _ok(lib.mbavo_undistort_u8(ctx.handle, im, HI, WI, m, HI, WI, ptr(out["u8"]))), asserted=True)
        run.call("u8_batch", lambda: _ok(lib.mbavo_undistort_u8_batch(ctx.handle, im, 2, HI, WI, m, HI, WI, ptr(out["u8_batch"]))), asserted=True)
        run.call("clearance_batch", lambda: _ok(lib.mbavo_undistort_clearance_batch(ctx.handle, 2, m, HI, WI, HI, WI, L, 2, ptr(out["clearance"]))), asserted=True)
        run.call("mask_batch", lambda: _ok(lib.mbavo_undistort_mask_batch(ctx.handle, 2, ptr(raw_masks[0]), HI, WI, m, HI, WI, ptr(out["mask"]))), asserted=True)
        run.call("mask_clearance_batch", lambda: _ok(lib.mbavo_mask_clearance_batch(ctx.handle, 2, m, ptr(und_masks[0]), HI, WI, HI, WI, L, 1,
                                                                                    ptr(out["mask_clearance"]))), asserted=True)
        run.finish()
        return dict(out)

    got = sb.run_case("b maps, remaps, clearance and masks", S, seq)
    real_imgs = tex(30)
    assert got["u8"] == uref.remap_u8(real_imgs[0], host_maps[0]).tobytes()
    assert got["u8_batch"] == np.stack([uref.remap_u8(im, host_maps[0]) for im in real_imgs]).tobytes()


# ---------------------------------------------------------------------------------------------------------------- c: cameras, masks, points
def test_c_cameras_masks_then_prepare(mbavo, own):
    """Case c on an object with G = 2 cameras and masks (48 x 64 from 52 x 76 raw images): set_cameras(A), set_cameras(B), set_masks,
    prepare under gates, with raw images, depth maps and masks late and the camera and index arrays overwritten after each return.
    What the object holds is the idle run's for B."""
    from mba_vo_amd import workloads
    S, ctx = own
    lib, capi = ctx.lib, mbavo.capi
    c = pairs_cases.undistort_case("crop", "outside")
    cam = lambda dist: workloads.pairs_camera(pairs_cases.undistort_camera(c, dist), c["intr"])
    set_a, set_b = (capi.PairsCamera * 2)(cam("outside"), cam("inside")), (capi.PairsCamera * 2)(cam("inside"), cam("none"))
    idx_a, idx_b = np.array([0, 1, 0], np.int32), np.array([1, 0, 1], np.int32)
    bufs = dict(sharp=_late_set(c["raw"]["sharp"], c["raw"]["new_sharp"]), z=_late_set(c["z"], c["new_z"]), blur=_late_set(c["raw"]["blur"], c["raw"]["new_blur"]))
    rng = np.random.default_rng(17)
    blocks = lambda: np.ascontiguousarray(np.kron((rng.uniform(size=(2, 12, 16)) > 0.25).astype(np.uint8) * 7, np.ones((4, 4), np.uint8)))
    masks = _late_set(blocks(), blocks())
    pb = pairs_cases.undistort_batch(ctx, c, 1, num_cameras=2, valid_radius=1, mask=1)
    try:
        def seq(run):
            run.place(list(bufs.values()) + [masks])
            ca, over_c = run.host(set_a, set_b)
            ia, over_i = run.host(idx_a, idx_b)
            run.call("set_cameras A", lambda: _ok(lib.mbavo_pairs_set_cameras(pb.handle, 2, ca, capi.ip(ia))), after=lambda: (over_c(), over_i()), asserted=True)
            cb, over_c2 = run.host(set_b, set_a)
            ib, over_i2 = run.host(idx_b, idx_a)
            run.call("set_cameras B", lambda: _ok(lib.mbavo_pairs_set_cameras(pb.handle, 2, cb, capi.ip(ib))), after=lambda: (over_c2(), over_i2()))
            run.regate(always=True)  # (the second set_cameras has waited for the first one's copy out of the mirror)
            run.call("set_masks", lambda: _ok(lib.mbavo_pairs_set_masks(pb.handle, 0, 2, masks[0].data_ptr())), asserted=True)
            counts = np.zeros((c["B"], c["L"]), np.int32)
            run.call("prepare", lambda: _ok(lib.mbavo_pairs_prepare(pb.handle, bufs["sharp"][0].data_ptr(), bufs["z"][0].data_ptr(), bufs["blur"][0].data_ptr(),
                                                                   capi.ip(counts))))
            run.finish()
            got = dv.read_batch(pb, counts)
            return dict(counts=counts.tobytes(), **{key: b"".join(g[key].tobytes() for g in got) for key in ("ref", "cur", "grad", "xy", "z")})

        sb.run_case("c set_cameras A, B, set_masks, prepare (G = 2)", S, seq)
    finally:
        pb.close()


def _point_lists(rng, lengths):
    """(xy total x 2, z total, offsets) of level-0 points over the image and a little past it, a third on whole pixels."""
    n = int(sum(lengths))
    xy = np.stack([rng.uniform(-2, W + 2, n), rng.uniform(-2, H + 2, n)], 1)
    xy[::3] = np.floor(xy[::3])
    return np.ascontiguousarray(xy), rng.uniform(1.0, 3.0, n), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def test_c_prepare_points_and_update_points(mbavo, own):
    """Case c with the caller's keypoints: prepare_points, then update_points with a key list, points and depths late, the offsets
    and the key list overwritten after each return.  The real run's lists equal the numpy restatement."""
    from mba_vo_amd import workloads
    S, ctx = own
    lib, capi = ctx.lib, mbavo.capi
    a, b = _pairs_inputs(1), _pairs_inputs(2)
    rng = np.random.default_rng(44)
    (xy_r, z_r, off_r), (xy_s, z_s, off_s) = _point_lists(rng, (40, 50, 60)), _point_lists(rng, (55, 45, 50))
    (xy2_r, z2_r, off2_r), (xy2_s, z2_s, off2_s) = _point_lists(rng, (30, 40)), _point_lists(rng, (45, 25))
    first = dict(sharp=_late_set(a["sharp"], b["sharp"]), blur=_late_set(a["blur"], b["blur"]), xy=_late_set(xy_r, xy_s), z=_late_set(z_r, z_s))
    nxt = dict(sharp=_late_set(b["sharp"][:2], a["sharp"][:2]), blur=_late_set(b["blur"], a["blur"]), xy=_late_set(xy2_r, xy2_s), z=_late_set(z2_r, z2_s))
    keys = (np.array([0, 2], np.int32), np.array([1, 2], np.int32))
    pb = workloads.PairBatch(ctx, B, L=L, H=H, W=W, k=4, N=4, cell=0, every_candidate=True, thresh=ps.THR, border=4)
    p = lambda d, key: d[key][0].data_ptr()
    try:
        def seq(run):
            run.place(list(first.values()))
            counts = np.zeros((B, L), np.int32)
            of, over = run.host(off_r, off_s)
            run.call("prepare_points", lambda: _ok(lib.mbavo_pairs_prepare_points(pb.handle, p(first, "sharp"), p(first, "blur"), capi.ip(of), p(first, "xy"),
                                                                                 p(first, "z"), capi.ip(counts))), after=over)
            run.place(list(nxt.values()))  # (prepare_points reads its counts back: the update gets a backlog and late inputs of its own)
            kl, over_k = run.host(*keys)
            of2, over_o = run.host(off2_r, off2_s)
            run.call("update_points", lambda: _ok(lib.mbavo_pairs_update_points(pb.handle, p(nxt, "blur"), 2, capi.ip(kl), p(nxt, "sharp"), capi.ip(of2),
                                                                               p(nxt, "xy"), p(nxt, "z"), capi.ip(counts))), after=lambda: (over_k(), over_o()))
            run.finish()
            got = dv.read_batch(pb, counts)
            return dict(counts=counts.tobytes(), **{key: b"".join(g[key].tobytes() for g in got) for key in ("ref", "cur", "grad", "xy", "z")})

        got = sb.run_case("c prepare_points, update_points", S, seq)
        rows = lambda xy, z, off, i: (xy[off[i]:off[i + 1]], z[off[i]:off[i + 1]])
        final = [rows(xy2_r, z2_r, off2_r, 0), rows(xy_r, z_r, off_r, 1), rows(xy2_r, z2_r, off2_r, 1)]
        want, want_counts = pref.keypoints(final, L, H, W, [4] * L)
        assert got["counts"] == want_counts.tobytes()
        assert got["xy"] == b"".join(w["xy"].tobytes() for w in want) and got["z"] == b"".join(w["z"].tobytes() for w in want)
    finally:
        pb.close()
