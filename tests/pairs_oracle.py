"""The oracle on what a pairs object hands to the engine (helper, no test in it).

oracle_problem rebuilds one entry of a PairBatch's problem array on the host from the entry's own fields and the device arrays it
points at -- nothing comes from the constructor arguments of the Python object -- and oracle_lm_levels runs the oracle's
coarse-to-fine LM loop (orc_optimize_trajectory, blur_aware_direct_tracker.cpp:544-924, restated call by call on the oracle's own
evaluation, solver, LM and trust-region functions) on the L rebuilt problems of one pair, every level with the intrinsics and the
start index ITS entry states.  tests/test_gpu_pairs_oracle.py holds the device to both.

The four option-laden objects of that file (OBJECTS) are described here once: `inputs` makes their numpy inputs, `make_object`
the device object, and `host_levels` the arrays every (pair, level) must hold from the numpy restatements that are byte-exact to
the device (pairs_ref, pairs_cameras_ref, pairs_unified_ref, pairs_valid_ref, pairs_mask_ref, pairs_depth_ref, pairs_dense_ref,
pairs_points_ref), so that tests/test_pairs_oracle_inputs.py can assert on the CPU what the GPU tests rest on."""
import ctypes as C

import numpy as np

import pairs_cameras_ref as cref
import pairs_dense_ref as dref
import pairs_depth_ref as zref
import pairs_device as dv
import pairs_mask_ref as mref
import pairs_points_ref as pref
import pairs_ref
import pairs_undistort_ref as uref
import pairs_valid_ref as vref
from lm_support import lm_batch_opts
from mba_vo_amd import synth

LM = dict(max_num_iterations=20, max_nonmono=5, solver_type=0, min_step_quality=0.5, min_abs_cost_decrease=1e-3, max_chi_square_error=3.0)
HUBER = 10.0


def lm_opts(capi, k):
    """LM's numbers for lm_support.lm_batch_opts."""
    return lm_batch_opts(capi, k, LM["max_num_iterations"], LM["max_nonmono"], LM["solver_type"], 0, LM["min_step_quality"], LM["min_abs_cost_decrease"],
                         LM["max_chi_square_error"])


# ---------------------------------------------------------------------------------------------------------------- gradient formats
def decode_half(raw, H, W):
    """Format 1: H * W * 2 IEEE half words (uint16) -> the H x W x 2 float32 [dx, dy] image; the conversion is exact."""
    raw = np.ascontiguousarray(raw, dtype=np.uint16)
    assert raw.size == H * W * 2
    return np.ascontiguousarray(raw.view(np.float16).astype(np.float32).reshape(H, W, 2))


def decode_packed(words, H, W):
    """Format 2: H * W words of 8 + 9 + 9 bits -> (intensity H x W uint8, gradient H x W x 2 float32): bits 0-7 the intensity,
    bits 8-16 and 23-31 the doubled central differences as 9-bit two's complement (tests/test_host_logic.py states the same)."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(H, W)
    kx = ((w.astype(np.int64) << 47) >> 55).astype(np.int32)
    ky = w.view(np.int32) >> 23
    g = np.stack([kx.astype(np.float32) * np.float32(0.5), ky.astype(np.float32) * np.float32(0.5)], 2)
    return (w & 0xff).astype(np.uint8), np.ascontiguousarray(g)


def encode_half(grad):
    """The half words of a float gradient image, as mbavo_image_gradients_u8_half stores them."""
    return np.ascontiguousarray(grad, dtype=np.float32).astype(np.float16).view(np.uint16).ravel()


# ---------------------------------------------------------------------------------------------------------------- one entry
def read_entry(capi, q, k):
    """Everything one mbavo_problem points at, copied back: a dict of numpy arrays and numbers."""
    H, W, K, P, N, F = q.H, q.W, q.K, q.P, q.N, q.F
    n = H * W
    fmt = int(q.grad_fp16)
    ref = dv.peek(q.d_ref_img, n, np.uint8).reshape(H, W)
    if fmt == 0:
        grad = dv.peek(q.d_ref_dIxy, 2 * n, np.float32).reshape(H, W, 2)
        word_I = None
    elif fmt == 1:
        grad, word_I = decode_half(dv.peek(q.d_ref_dIxy, 2 * n, np.uint16), H, W), None
    else:
        assert fmt == 2, fmt
        word_I, grad = decode_packed(dv.peek(q.d_ref_dIxy, n, np.uint32), H, W)
    ptrs = dv.peek(q.d_cur_imgs, F, np.uint64)
    curs = [dv.peek(int(p), n, np.uint8).reshape(H, W) for p in ptrs]
    stride = int(q.kp_stride)
    assert stride >= 2
    xy = np.ascontiguousarray(dv.peek(q.d_kp_xy, K * stride, np.float64).reshape(K, stride)[:, :2])
    z = dv.peek(q.d_kp_z, K, np.float64)
    outlier = dv.peek(q.d_outlier, K, np.uint8) if q.d_outlier else None
    return dict(S=int(q.S), F=F, K=K, P=P, k=k, N=N, H=H, W=W, fmt=fmt, ref=ref, word_I=word_I, grad=np.ascontiguousarray(grad), curs=curs,
                xy=xy, z=z, stride=stride, pattern=dv.peek(q.d_pattern, 2 * P, np.int32), intr=np.array(list(q.intrinsics)),
                cap=dv.peek(q.d_cap_time, F, np.float64), exp=dv.peek(q.d_exp_time, F, np.float64), t0=float(q.t0), dt=float(q.dt),
                kt=dv.peek(q.d_knots_t, 3 * N, np.float64), kR=dv.peek(q.d_knots_R, 4 * N, np.float64),
                start=np.array([q.h_start_idx[f] for f in range(F)], np.int32), huber=float(q.huber_a), outlier=outlier, num_bad=int(q.num_bad))


def problem_of(orc, e):
    """orc.make_problem of a read_entry / host_levels dict: (OrcProblem, keep-alive list whose last item is the dict).  A packed
    keyframe's intensity is the word's (what the kernel reads)."""
    ref = e["ref"] if e.get("word_I") is None else e["word_I"]
    p, keep = orc.make_problem(e["S"], e["F"], e["K"], e["P"], e["k"], e["N"], e["H"], e["W"], np.ascontiguousarray(ref), e["grad"], e["curs"],
                               e["xy"], e["z"], e["pattern"], e["intr"], e["cap"], e["exp"], e["t0"], e["dt"], e["kt"], e["kR"], e["start"],
                               e["huber"], outlier=e["outlier"], num_bad=e["num_bad"])
    return p, keep + [e]


def oracle_problem(orc, capi, entry, k):
    """(OrcProblem, keep-alive) of exactly what the entry says; keep[-1] is the read_entry dict."""
    return problem_of(orc, read_entry(capi, entry, k))


# ---------------------------------------------------------------------------------------------------------------- the LM loop
def _evaluate(L, p, patch_blocks, frame_blocks, H, g):
    cost = np.zeros(1)
    L.orc_evaluate(C.byref(p), patch_blocks.ctypes.data_as(C.POINTER(C.c_double)), frame_blocks.ctypes.data_as(C.POINTER(C.c_double)),
                   cost.ctypes.data_as(C.POINTER(C.c_double)), None if H is None else H.ctypes.data_as(C.POINTER(C.c_double)),
                   None if g is None else g.ctypes.data_as(C.POINTER(C.c_double)))
    return float(cost[0])


def detect_outliers(costs, chi, flags):
    """detectOutliersAndUploadToGpu (:639-699) as the oracle restates it: flags are only ever set; returns (number flagged by this
    call, the smallest relative distance of a |cost - mu| from the bound)."""
    c = np.asarray(costs, np.float64)
    keep = ~(c < 1e-8)
    cnt = int(keep.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = (np.cumsum(c[keep])[-1] if cnt else 0.0) / np.float64(cnt)         # (cumsum: the sequential sum of the C loop)
        var = (np.cumsum((c[keep] - mu) * (c[keep] - mu))[-1] if cnt else 0.0) / np.float64(cnt)
        thr = chi * float(np.sqrt(np.float32(var)))
        hit = np.abs(c - mu) > thr
        margin = np.abs(np.abs(c - mu) - thr) / (thr if thr > 0 else 1.0)
    flags[hit] = 1
    return int(hit.sum()), (float(np.nanmin(margin)) if len(c) and cnt else float("inf"))


def oracle_lm_levels(orc, problems_of_pair, lm_opts=LM):
    """The oracle's optimizeTrajectory on one pair: problems_of_pair[l] is the (OrcProblem, keep) of level l, all levels with the
    same times and the same initial knots.  Every level is evaluated with ITS problem's intrinsics and start index.  Returns
    dict(trace [(level, iter, kind, outliers, radius, eval cost, candidate cost, model change, quality)], kt, kR, cost, margin:
    the smallest relative distance of any patch cost from its chi bound in any detection, quality_margin: the smallest
    |quality - min_step_quality| of an evaluated step)."""
    L = orc.lib()
    probs = [p for p, _ in problems_of_pair]
    ents = [keep[-1] for _, keep in problems_of_pair]
    k, N, F = probs[0].k, probs[0].N, probs[0].F
    n, E = 6 * N, orc.packed_len(probs[0].k)
    for e in ents[1:]:
        assert np.array_equal(e["kt"], ents[0]["kt"]) and np.array_equal(e["kR"], ents[0]["kR"]) and e["N"] == N and e["F"] == F
    kt, kR = ents[0]["kt"].copy(), ents[0]["kR"].copy()
    cand_t, cand_R = np.zeros(3 * N), np.zeros(4 * N)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    H, g, step = np.zeros(n * n), np.zeros(n), np.zeros(n)
    lm, tr = orc.OrcLm(), orc.OrcTr()
    L.orc_lm_init(C.byref(lm))
    L.orc_tr_init(C.byref(tr), int(lm_opts["max_nonmono"]))
    trace, margin, qmargin, eval_cost = [], float("inf"), float("inf"), 0.0
    for lv in range(len(probs) - 1, -1, -1):
        p = probs[lv]
        K = p.K
        flags = np.zeros(max(K, 1), np.uint8)
        patch_blocks, frame_blocks = np.zeros(max(F * K * E, 1)), np.zeros(F * E)
        p.outlier, p.num_bad = flags.ctypes.data_as(orc.c_u8p), 0
        p.knots_t, p.knots_R = dp(kt), dp(kR)
        cand_cost = model = quality = 0.0
        eval_cost = _evaluate(L, p, patch_blocks, frame_blocks, H, g)
        L.orc_lm_reset(C.byref(lm))
        L.orc_tr_reset(C.byref(tr), eval_cost)
        trace.append((lv, 0, 0, 0, lm.radius, eval_cost, 0.0, 0.0, 0.0))
        it, abs_dec = 0, 1e10
        while True:
            it += 1
            if it > lm_opts["max_num_iterations"] or abs_dec < lm_opts["min_abs_cost_decrease"]:
                break
            iradius = 1.0 / lm.radius
            for i in range(n):
                H[i * n + i] += H[i * n + i] * iradius
            L.orc_solve_normal_equation(dp(H), dp(g), n, int(lm_opts["solver_type"]), dp(step))
            Hl, gl, sl = H.tolist(), g.tolist(), step.tolist()
            gx = 0.0
            for i in range(n):
                gx += gl[i] * sl[i]
            xHx = 0.0
            for r in range(n):
                a = 0.0
                for c in range(n):
                    a += Hl[c * n + r] * sl[c]
                xHx += sl[r] * a
            model = -(gx + 0.5 * xHx)
            if model < 0:
                L.orc_lm_rejected(C.byref(lm))
                trace.append((lv, it, 3, p.num_bad, lm.radius, eval_cost, 0.0, model, 0.0))
                continue
            L.orc_plus_t(dp(kt), dp(step), N, dp(cand_t))
            L.orc_plus_R(dp(kR), dp(step[3 * N:]), N, dp(cand_R))
            p.knots_t, p.knots_R = dp(cand_t), dp(cand_R)
            cand_cost = _evaluate(L, p, patch_blocks, frame_blocks, None, None)
            p.knots_t, p.knots_R = dp(kt), dp(kR)
            abs_dec = eval_cost - cand_cost
            quality = L.orc_tr_quality(C.byref(tr), cand_cost, model)
            if quality == quality:
                qmargin = min(qmargin, abs(quality - lm_opts["min_step_quality"]))
            if quality > lm_opts["min_step_quality"] and cand_cost < eval_cost:
                p.num_bad, m = detect_outliers(patch_blocks[:K * E:E], lm_opts["max_chi_square_error"], flags)
                margin = min(margin, m)
                kt[:], kR[:] = cand_t, cand_R
                eval_cost = _evaluate(L, p, patch_blocks, frame_blocks, H, g)
                L.orc_lm_accepted(C.byref(lm), quality)
                L.orc_tr_accepted(C.byref(tr), eval_cost, model)
                trace.append((lv, it, 1, p.num_bad, lm.radius, eval_cost, cand_cost, model, quality))
                continue
            L.orc_lm_rejected(C.byref(lm))
            trace.append((lv, it, 2, p.num_bad, lm.radius, eval_cost, cand_cost, model, quality))
        p.outlier, p.num_bad = None, 0
    return dict(trace=trace, kt=kt.reshape(N, 3).copy(), kR=kR.reshape(N, 4).copy(), cost=eval_cost, margin=margin, quality_margin=qmargin)


def evaluate0(orc, p):
    """One evaluation with the Hessian through the variant's own library: (packed frame blocks F x E, patch costs F x K)."""
    E = orc.packed_len(p.k)
    pb, fb = np.zeros(max(p.F * p.K * E, 1)), np.zeros(p.F * E)
    n = 6 * p.N
    _evaluate(orc.lib(), p, pb, fb, np.zeros(n * n), np.zeros(n))
    return fb.reshape(p.F, E), pb[:p.F * p.K * E].reshape(p.F, p.K, E)[:, :, 0].copy()


# ---------------------------------------------------------------------------------------------------------------- the four objects
def _cam3():
    """The three cameras of object D: the two of the clearance tests and the radial-tangential one again under another pinhole."""
    a, b = vref.CAMERAS["radtan"], vref.CAMERAS["unified"]
    t = a["to_intr"]
    return [a, b, dict(a, dist=uref.DIST_INSIDE, to_intr=(1.04 * t[0], 0.97 * t[1], t[2] - 0.6, t[3] + 0.4))]


_C_HS, _C_WS = 80, 112
_C_CAM = dict(model=2, Hs=_C_HS, Ws=_C_WS, xi=0.8, dist=(0.035, -0.006, -2e-4, 1e-4),
              from_intr=tuple(1.6 * v if i < 2 else v for i, v in enumerate(uref.intrinsics(_C_HS, _C_WS))), to_intr=uref.intrinsics(72, 100))

OBJECTS = {
    # Seeds: chosen on the CPU (tests/test_pairs_oracle_inputs.py) so that the oracle and its contracted build take the same
    # decisions, no pair of A .. D loses every pixel, and the two builds end close to each other -- a k = 4 spline held by one
    # exposure is weakly constrained, and most seeds send even the reference's two roundings to different places.
    # pinhole, packed keyframe, grid picks, ray-distance depth maps with a cut-off, k = 4 on the second segment of five knots (a
    # long exposure, so that the samples span the segment)
    "A": dict(B=3, L=2, H=75, W=101, S=3, k=4, N=5, start=1, P=8, fmt=2, dense=False, cell=6, thr=3.0, border=(3, 2), intr=(90.0, 90.0, 50.0, 37.0),
              depth=dict(depth_format=1, depth_unit=0.0, depth_max=100.0), undistort=0, cams=None, cam_of=None, radius=0, masks=None, points=False, seed=2, exp=0.35, knot_noise=0.02),
    # raw images AND raw 16-bit depth maps of two cameras (radtan, unified), clearance radius 2, raw-geometry masks (a low bonnet, a
    # thin scatter of single pixels: with radius 2 anything denser leaves level 1 without keypoints), half gradients
    "B": dict(B=4, L=2, H=vref.H, W=vref.W, S=3, k=2, N=2, start=0, P=8, fmt=1, dense=False, cell=4, thr=3.0, border=(3, 2), intr=None,
              depth=dict(depth_format=2, depth_unit=5000.0, depth_max=0.0), undistort=2, cams=[vref.CAMERAS["radtan"], vref.CAMERAS["unified"]],
              cam_of=(0, 1, 1, 0), radius=2, masks=(lambda: mref.bonnet(height=0.3), lambda: mref.scatter(share=0.004)), points=False, seed=12),
    # one unified camera, every candidate a one-pixel keypoint (level-0 K beyond 4096), float gradients
    "C": dict(B=3, L=2, H=72, W=100, S=3, k=2, N=2, start=0, P=1, fmt=0, dense=True, cell=0, thr=1.0, border=(3, 2), intr=_C_CAM["to_intr"],
              depth=dict(depth_format=0, depth_unit=0.0, depth_max=0.0), undistort=1, cams=[_C_CAM], cam_of=None, radius=0, masks=None, points=False, seed=2),
    # the caller's points, one camera per pair, clearance radius 1, packed keyframe
    "D": dict(B=3, L=3, H=vref.H, W=vref.W, S=5, k=4, N=4, start=0, P=8, fmt=2, dense=True, cell=0, thr=3.0, border=(3, 2, 1), intr=None,
              depth=None, undistort=1, cams=_cam3(), cam_of=(0, 1, 2), radius=1, masks=None, points=True, lengths=(190, 50, 130), seed=4),
}
_INPUTS = {}


def _noised_shift(img, rng):
    return np.clip(np.roll(img, (1, -1), (0, 1)).astype(np.int32) + rng.integers(-4, 5, img.shape), 0, 255).astype(np.uint8)


def motion(o, seed=0):
    """Times and knots with every blur sample and the capture time on segment o["start"]; the knots of synth.trajectory("harness")."""
    rng = np.random.default_rng(700 + 10 * o["seed"] + seed)
    B, N = o["B"], o["N"]
    kt, kR = np.zeros((B, N, 3)), np.zeros((B, N, 4))
    for b in range(B):
        kt[b], kR[b] = synth.trajectory("harness", N, 0.004 * (b + 1), 0.01 * (b + 1))
        kt[b] += rng.normal(0, o.get("knot_noise", 0.05), 3)
    cap = (o["start"] + 0.4 + 0.05 * np.arange(B)) * 0.5
    return dict(cap=cap, exp=np.full(B, o.get("exp", 0.04)), t0=np.zeros(B), dt=0.5, kt=np.ascontiguousarray(kt), kR=np.ascontiguousarray(kR))


def inputs(name):
    """The numpy inputs of an object, made once and left unchanged: sharp / blur (raw geometry where the object undistorts), depth
    maps in the object's format and geometry or point lists, raw masks, the motion; and for object B a second frame (`new_*`)."""
    if name in _INPUTS:
        return _INPUTS[name]
    o = OBJECTS[name]
    rng = np.random.default_rng(9000 + o["seed"])
    B, H, W = o["B"], o["H"], o["W"]
    Hi, Wi = (o["cams"][0]["Hs"], o["cams"][0]["Ws"]) if o["undistort"] else (H, W)
    octaves = (8, 4) if o["dense"] and not o["points"] else (16, 8, 4)
    tex = lambda seed: np.ascontiguousarray(np.stack([synth.texture_image(Hi, Wi, seed=seed + 3 * b, octaves=octaves) for b in range(B)]))
    sharp = tex(50 + 100 * o["seed"])
    blur = np.ascontiguousarray(np.stack([_noised_shift(s, rng) for s in sharp]))
    c = dict(sharp=sharp, blur=blur, motion=motion(o))
    if o["points"]:
        pts = []
        for n in o["lengths"]:
            xy = np.stack([rng.uniform(-2, W + 2, n), rng.uniform(-2, H + 2, n)], 1)
            xy[::3] = np.floor(xy[::3])
            z = rng.uniform(1.0, 3.0, n)
            z[rng.uniform(0, 1, n) < 0.05] = 0.005
            pts.append((np.ascontiguousarray(xy), np.ascontiguousarray(z)))
        c["points"] = pts
    else:
        Hd, Wd = (Hi, Wi) if o["undistort"] == 2 else (H, W)

        def depth_maps():
            holes = rng.uniform(0, 1, (B, Hd, Wd))
            if o["depth"]["depth_format"] == 2:
                d = rng.integers(5000, 15000, (B, Hd, Wd)).astype(np.uint16)
                d[holes < 0.1] = 0
            else:
                d = rng.uniform(1.0, 3.0, (B, Hd, Wd)).astype(np.float32)
                d[holes < 0.1] = 0.0
                if o["depth"]["depth_format"] == 1:
                    d[(holes >= 0.1) & (holes < 0.14)] = 150.0  # beyond depth_max
            return d
        c["depth"] = depth_maps()
    if o["masks"]:
        c["raw_masks"] = np.ascontiguousarray(np.stack([m() for m in o["masks"]]))
    if name == "B":  # the second frame: new blurred frames for all pairs, a new keyframe for pair 2
        c["new_sharp"] = np.ascontiguousarray(np.stack([synth.texture_image(Hi, Wi, seed=977, octaves=octaves)]))
        both = sharp.copy()
        both[2] = c["new_sharp"][0]
        c["new_blur"] = np.ascontiguousarray(np.stack([np.clip(np.roll(s, (-1, 1), (0, 1)).astype(np.int32) + rng.integers(-4, 5, s.shape), 0, 255).astype(np.uint8)
                                                       for s in both]))
        c["new_depth"] = depth_maps()[2:3].copy()
        c["new_motion"] = motion(o, seed=1)
    _INPUTS[name] = c
    return c


def second_frame(name):
    """The composite inputs after object B's update with key pair 2."""
    c = dict(inputs(name))
    sharp, depth = c["sharp"].copy(), c["depth"].copy()
    sharp[2], depth[2] = c["new_sharp"][0], c["new_depth"][0]
    c.update(sharp=sharp, depth=depth, blur=c["new_blur"], motion=c["new_motion"])
    return c


def pattern(o):
    return synth.PATTERN8 if o["P"] == 8 else np.zeros(2, np.int32)


def camera_of(o, b):
    if not o["undistort"]:
        return None
    return o["cams"][o["cam_of"][b]] if o["cam_of"] is not None else o["cams"][0]


def to_intr(o, b):
    cam = camera_of(o, b)
    return tuple(float(v) for v in (o["intr"] if o["cam_of"] is None else cam["to_intr"]))


def plain_intake(pair, g, image, map_xy):
    """How an uncalibrated object takes an image in: through its camera's map, or as it is where the object has none."""
    return image if map_xy is None else uref.remap_u8(image, map_xy)


def host_levels(name, c=None, intake=None):
    """Per pair a list over the levels of read_entry-shaped dicts, from the numpy restatements alone.  intake(pair, camera index,
    image, map or None) -> level 0 of one arriving image (None: plain_intake; tests/pairs_photocal_support.py has the calibrated one)."""
    o = OBJECTS[name]
    c = inputs(name) if c is None else c
    intake = plain_intake if intake is None else intake
    B, L, H, W, m = o["B"], o["L"], o["H"], o["W"], c["motion"]
    maps = {}
    out = []
    for b in range(B):
        cam, K4 = camera_of(o, b), to_intr(o, b)
        mp, clear = None, None
        g = o["cam_of"][b] if o["cam_of"] is not None else 0
        if cam is not None:
            if g not in maps:
                maps[g] = cref.camera_map(cam, H, W)
            mp = maps[g]
        sharp, blur = intake(b, g, c["sharp"][b], mp), intake(b, g, c["blur"][b], mp)
        if o["radius"] > 0 or o["masks"]:
            mask = mref.warp_mask(c["raw_masks"][o["cam_of"][b]], mp) if o["masks"] else None
            clear = mref.clearance(mp, mask, L, o["radius"], cam["Hs"], cam["Ws"])
        if not o["points"]:
            d = o["depth"]
            if o["undistort"] == 2:
                z0 = uref.depth_through_map(d["depth_format"], c["depth"][b], mp, K4, d["depth_unit"], d["depth_max"])
            else:
                z0 = zref.to_z(d["depth_format"], c["depth"][b], K4, d["depth_unit"], d["depth_max"])
            z0 = np.ascontiguousarray(z0, dtype=np.float32)
        refs, curs = synth.pyramid(np.ascontiguousarray(sharp), L), synth.pyramid(np.ascontiguousarray(blur), L)
        levels = []
        for l in range(L):
            Hl, Wl = H >> l, W >> l
            assert refs[l].shape == (Hl, Wl)
            if o["points"]:
                xy, z = pref.level_keypoints(c["points"][b][0], c["points"][b][1], l, Hl, Wl, o["border"][l], None if clear is None else clear[l])
            else:
                if o["dense"]:
                    xy, z = dref.keypoints(refs[l], l, o["thr"], z0, o["border"][l])
                else:
                    xy, z = pairs_ref.keypoints(refs[l], l, H, W, o["cell"], o["cell"], o["thr"], z0, o["border"][l])
                if clear is not None:
                    keep = clear[l][xy[:, 1].astype(np.int64), xy[:, 0].astype(np.int64)] == 1
                    xy, z = xy[keep], z[keep]
            grad = synth.image_gradients(refs[l])
            if o["fmt"] == 1:
                grad = decode_half(encode_half(grad), Hl, Wl)
            elif o["fmt"] == 2:
                I, grad = decode_packed(synth.pack_keyframe(refs[l]), Hl, Wl)
                assert np.array_equal(I, refs[l])
            levels.append(dict(S=o["S"], F=1, K=len(z), P=o["P"], k=o["k"], N=o["N"], H=Hl, W=Wl, fmt=o["fmt"], ref=refs[l], word_I=None,
                               grad=np.ascontiguousarray(grad), curs=[curs[l]], xy=np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2),
                               z=np.ascontiguousarray(z, dtype=np.float64), stride=2, pattern=np.ascontiguousarray(pattern(o), dtype=np.int32),
                               intr=np.array([v / float(1 << l) for v in K4]), cap=m["cap"][b:b + 1].copy(), exp=m["exp"][b:b + 1].copy(),
                               t0=float(m["t0"][b]), dt=float(m["dt"]), kt=m["kt"][b].ravel().copy(), kR=m["kR"][b].ravel().copy(),
                               start=np.array([synth.segment_start_index(m["cap"][b], m["t0"][b], m["dt"])], np.int32), huber=HUBER,
                               outlier=None, num_bad=0))
        out.append(levels)
    return out


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to("cuda:0")


def _pairs_camera(cam):
    from mba_vo_amd import workloads
    raw = (workloads.camera_unified(cam["Hs"], cam["Ws"], cam["from_intr"], cam["xi"], cam["dist"]) if cam["model"] == 2
           else workloads.camera_radtan(cam["Hs"], cam["Ws"], cam["from_intr"], cam["dist"]))
    return raw, workloads.pairs_camera(raw, cam["to_intr"])


def prepare_object(pb, name, c=None):
    """The object's prepare on the inputs c (default: its own): counts B x L."""
    o = OBJECTS[name]
    c = inputs(name) if c is None else c
    if o["points"]:
        return pb.prepare_points(_t(c["sharp"]), _t(c["blur"]), c["points"])
    return pb.prepare(_t(c["sharp"]), _t(c["depth"]), _t(c["blur"]))


def make_object(ctx, name, before_prepare=None):
    """The prepared device object with its motion set: (PairBatch, counts B x L).  before_prepare(pb): called after the camera and
    mask calls and before the prepare."""
    from mba_vo_amd import workloads
    o, c = OBJECTS[name], inputs(name)
    G = len(o["cams"]) if o["cam_of"] is not None else 0
    pb = workloads.PairBatch(ctx, o["B"], L=o["L"], H=o["H"], W=o["W"], S=o["S"], k=o["k"], N=o["N"], intr=o["intr"], huber=HUBER, cell=o["cell"],
                             thresh=o["thr"], border=list(o["border"]), keyframe_format=o["fmt"], pattern=pattern(o), every_candidate=o["dense"],
                             undistort=o["undistort"], num_cameras=G, valid_radius=o["radius"], mask=1 if o["masks"] else 0, **(o["depth"] or {}))
    try:
        if G:
            assert pb.set_cameras([_pairs_camera(cam)[1] for cam in o["cams"]], list(o["cam_of"])) == 0
        elif o["undistort"]:
            assert pb.set_camera(_pairs_camera(o["cams"][0])[0]) == 0
        if o["masks"]:
            assert pb.set_masks(_t(c["raw_masks"]), 1) == 0
        if before_prepare is not None:
            before_prepare(pb)
        counts = prepare_object(pb, name, c)
        set_motion(pb, c["motion"])
    except Exception:
        pb.close()
        raise
    return pb, counts


def set_motion(pb, m):
    assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
