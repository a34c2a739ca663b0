"""BASELINE.json workloads as lists of alignment problems (numpy), plus device upload.

A workload is a list of `Prob` (one per pyramid level or per keyframe pair).  bench.py
times `mbavo_eval_batch` over the whole list (one GN iteration = one H/g evaluation of
every problem in it); tests use the same builders at reduced size.  Pure numpy + torch
plumbing; no oracle code.

The GPU-rendered workloads (RenderedPairBatch: level 0, the benchmark's; RenderedPairPyramids: L levels) stand on one
RenderedScene (the sequence and `render`, the one pair renderer), one detector step (detect_level) and one `fill_problem`,
which DeviceWorkload uses too; both expose their pairs as `pair(b)` (RenderedPair, its levels as RenderedLevel).
"""
import ctypes as C

import numpy as np

from . import capi, synth


class Prob:
    """One alignment problem on the host (numpy arrays; layout of include/mbavo.h:mbavo_problem)."""

    def __init__(self, ref, cur, kp_xy, kp_z, pattern, intr, S, k, N, cap, exp, t0, dt, knots_t, knots_R, huber,
                 grad=None):
        self.ref = np.ascontiguousarray(ref)
        self.grad = synth.image_gradients(self.ref) if grad is None else grad
        self.cur = [np.ascontiguousarray(c) for c in cur]
        self.H, self.W = self.ref.shape
        self.kp_xy, self.kp_z = np.ascontiguousarray(kp_xy), np.ascontiguousarray(kp_z)
        self.pattern = np.ascontiguousarray(pattern, np.int32)
        self.intr = np.ascontiguousarray(intr, np.float64)
        self.S, self.k, self.N, self.F = S, k, N, len(self.cur)
        self.K, self.P = self.kp_xy.shape[0], self.pattern.size // 2
        self.cap, self.exp = np.ascontiguousarray(cap, np.float64), np.ascontiguousarray(exp, np.float64)
        self.t0, self.dt, self.huber = float(t0), float(dt), float(huber)
        self.knots_t, self.knots_R = np.ascontiguousarray(knots_t, np.float64).ravel(), np.ascontiguousarray(knots_R, np.float64).ravel()
        self.start_idx = np.array([synth.segment_start_index(c, t0, dt) for c in self.cap], np.int32)
        self.outlier, self.num_bad = None, 0
        self.grad_fp16 = False  # True / 1: upload the gradient image as IEEE half pairs (BASELINE configs[4]); 2: the packed keyframe

    @property
    def pixel_samples(self):
        return self.F * self.K * self.P * self.S


def _current_image(ref, rng, shift=(1, -2), noise=6):
    sh = np.roll(ref, shift, (0, 1)).astype(np.int32)
    return np.ascontiguousarray(np.clip(sh + rng.integers(-noise, noise + 1, ref.shape), 0, 255).astype(np.uint8))


def pyramid_pair(H=480, W=640, levels=4, S=8, k=4, N=4, mode="dense", seed=1, huber=10.0, margin=0,
                 trans_scale=0.004, rot_scale=0.05, frames=1):
    """Config 1/2 of BASELINE.json: one keyframe pair, `levels` pyramid levels, `S` blur samples,
    `N` control poses.  mode 'dense': every pixel a P=1 patch with its own depth;
    'semidense': grid-selected keypoints (30-px cells) with the harness' 8-pixel pattern.
    frames > 1: a joint problem of `frames` blurred frames against the same keyframe on one spline segment (the
    multi-GPU workload: one frame per rank); frame 0 is exactly the frames == 1 problem."""
    rng = np.random.default_rng(seed)
    ref0 = synth.noise_image(H, W, seed=seed)
    refs = synth.pyramid(ref0, levels)
    curs = [synth.pyramid(_current_image(ref0, rng, shift=(1 + f % 3, -2 - f % 2)), levels) for f in range(frames)]
    kt, kR = synth.harness_spline(trans_scale, rot_scale, N)
    t0, dt = 0.0, 0.5
    cap, exp = [0.25 + 0.01 * f for f in range(frames)], [0.1] * frames
    assert all(synth.segment_start_index(c - 0.05, t0, dt) == 0 and synth.segment_start_index(c + 0.05, t0, dt) + k <= N for c in cap)
    probs = []
    for l in range(levels):
        sc = 2 ** l
        Hl, Wl = refs[l].shape
        intr = np.array([W / 2.0, W / 2.0, W / 2.0, H / 2.0]) / sc
        if mode == "dense":
            xy, z = synth.dense_keypoints(Hl, Wl, margin=margin, seed=seed + 10 + l)
            pat = np.zeros(2, np.int32)
        else:
            xy, z = synth.semi_dense_keypoints(refs[l], cell=30, thresh=4.0, margin=max(4, 20 // sc), seed=seed + 10 + l)
            pat = synth.PATTERN8
        probs.append(Prob(refs[l], [c[l] for c in curs], xy, z, pat, intr, S, k, N, cap, exp, t0, dt, kt, kR, huber))
    return probs


def pair_batch(B, H=480, W=640, S=8, k=4, N=4, mode="semidense", seed=1, huber=10.0):
    """Config 2/3 of BASELINE.json: B independent keyframe pairs (consecutive frames of one
    synthetic sequence, each with its own knots), level 0 only."""
    rng = np.random.default_rng(seed)
    ref0 = synth.noise_image(H, W, seed=seed)
    grad0 = synth.image_gradients(ref0)
    if mode == "dense":
        xy, z = synth.dense_keypoints(H, W, seed=seed + 10)
        pat = np.zeros(2, np.int32)
    else:
        xy, z = synth.semi_dense_keypoints(ref0, cell=30, thresh=4.0, margin=20, seed=seed + 10)
        pat = synth.PATTERN8
    intr = np.array([W / 2.0, W / 2.0, W / 2.0, H / 2.0])
    probs = []
    for b in range(B):
        kt, kR = synth.harness_spline(0.004, 0.05, N)
        kt = kt + rng.normal(0, 2e-3, kt.shape)
        cur = _current_image(ref0, rng, shift=(1 + b % 3, -(1 + b % 2)))
        probs.append(Prob(ref0, [cur], xy, z, pat, intr, S, k, N, [0.25], [0.1], 0.0, 0.5, kt, kR, huber, grad=grad0))
    return probs


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _qrot(q, v):
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R @ v


def loop_spline(n_knots, dt=0.5, amp=(0.5, 0.35, 0.04), period=(2.1, 1.7, 3.3), rot_amp=(0.012, 0.01, 0.006)):
    """Control knots of a bounded ground-truth trajectory (a Lissajous loop in front of the textured plane, small periodic
    roll / pitch / yaw): any number of frames stays on the texture, unlike the harness spline's straight line."""
    kt = np.zeros((n_knots, 3))
    kR = np.zeros((n_knots, 4))
    for i in range(n_knots):
        t = i * dt
        kt[i] = [amp[a] * np.sin(2 * np.pi * t / period[a] + 0.7 * a) for a in range(3)]
        kR[i] = synth.rpy_quat(*[rot_amp[a] * np.sin(2 * np.pi * t / (period[a] * 1.3) + 1.1 * a) for a in range(3)])
    return np.ascontiguousarray(kt), np.ascontiguousarray(kR)


class _PairInfo:
    """What bench.py's accounting needs to know about one device-resident pair (no host copies of the images)."""

    def __init__(self, S, k, N, F, K, P, H, W, fmt=0):
        self.S, self.k, self.N, self.F, self.K, self.P, self.H, self.W = S, k, N, F, K, P, H, W
        # SURVEY.md 8(d), semi-dense: the compulsory bytes are the taps of the distinct tap locations, bounded above by the
        # gather figure 36 B per pixel-sample (2 x 2 u8 + 2 x 2 x 8 B gradient taps) + the current pixel -- and by the
        # whole images (keyframe u8 + gradient 2 x f32 + current u8), all of them this pair's own
        # (keyframe formats 1 / 2: half pairs 1 + 4 bytes per pixel, 20 per tap; packed words 4 and 16)
        img, tap = {0: (9, 36), 1: (5, 20), 2: (4, 16)}[int(fmt)]
        self.fmt = int(fmt)
        self.image_bytes_upper = min(H * W * img + F * H * W, F * K * P * (S * tap + 1))  # the gather bound: no reuse at all
        # until distinct_tap_bytes() has counted the pair's distinct tap locations the upper bound stands in
        self.image_bytes = self.image_bytes_upper
        self.distinct = None  # (distinct keyframe pixels tapped, distinct current pixels read, 128-byte lines touched)

    @property
    def pixel_samples(self):
        return self.F * self.K * self.P * self.S


def fill_problem(q, S, F, K, P, N, H, W, ref, grad, cur_ptrs, xy, kz, pat, intr, cap, exp, t0, dt, kt, kR, start, huber, level=0,
                 grad_fp16=0, outlier=None, num_bad=0):
    """One mbavo_problem `q` from device tensors (it takes their pointers: the caller keeps them alive).  cur_ptrs: the int64 tensor
    of the F current images' pointers; intr: the level-0 (fx, fy, cx, cy), written divided by 2^level; start: the host int32
    array of the frames' start indices (h_start_idx points into it); outlier: the uint8 flags of num_bad keypoints, or None."""
    q.S, q.F, q.K, q.P, q.N, q.H, q.W = S, F, K, P, N, H, W
    q.d_ref_img, q.d_ref_dIxy, q.d_cur_imgs = ref.data_ptr(), grad.data_ptr(), cur_ptrs.data_ptr()
    q.d_kp_xy, q.kp_stride, q.d_kp_z, q.d_pattern = xy.data_ptr(), 2, kz.data_ptr(), pat.data_ptr()
    q.d_outlier, q.num_bad = (outlier.data_ptr() if outlier is not None else None), num_bad
    for i in range(4):
        q.intrinsics[i] = float(intr[i]) / (1 << level)
    q.d_cap_time, q.d_exp_time, q.t0, q.dt = cap.data_ptr(), exp.data_ptr(), t0, dt
    q.d_knots_t, q.d_knots_R = kt.data_ptr(), kR.data_ptr()
    q.h_start_idx = start.ctypes.data_as(C.POINTER(C.c_int))
    q.huber_a, q.grad_fp16 = huber, int(grad_fp16)


def detect_level(ctx, img, Hl, Wl, l, H0, W0, cell, thresh, depth, cap_kp, margin):
    """mbavo_detect_semidense on one pyramid level (img: Hl x Wl uint8, level l of an H0 x W0 image; depth: the level-0 float32
    z-map; room for cap_kp keypoints), then the filter of the semi-dense builder: the keypoints whose patch stays `margin`
    pixels inside the level, order kept.  Returns (xy 2K doubles, kz K doubles, K)."""
    import torch
    xy = torch.empty(cap_kp * 2, dtype=torch.float64, device=img.device)
    kz = torch.empty(cap_kp, dtype=torch.float64, device=img.device)
    cnt = C.c_int(0)
    capi.check(ctx.lib.mbavo_detect_semidense(ctx.handle, img.data_ptr(), Hl, Wl, l, H0, W0, cell, cell, float(thresh), depth.data_ptr(),
                                              xy.data_ptr(), kz.data_ptr(), cap_kp, C.byref(cnt)), "mbavo_detect_semidense")
    # (the clamp never binds for the rendered classes: the detector keeps at most one keypoint per grid cell, keyframe_ops.hip
    # cell_grid, and they pass the number of cells of the level, (Hl // cl + 1) * (Wl // cl + 1) with cl = int(cell / 1.414^l))
    K = min(cnt.value, cap_kp)
    xyv = xy[:2 * K].view(K, 2)
    ok = (xyv[:, 0] >= margin) & (xyv[:, 0] < Wl - margin) & (xyv[:, 1] >= margin) & (xyv[:, 1] < Hl - margin)
    kz = kz[:K][ok].contiguous()
    return xyv[ok].contiguous().view(-1), kz, int(kz.shape[0])


class RenderedLevel:
    """One pyramid level of a rendered pair, as its mbavo_problem entry points at it: device tensors (ref, cur uint8 H * W; grad
    in the keyframe format; xy 2K and kz K doubles, margin-filtered; cur_ptrs the one-element int64 tensor d_cur_imgs is)."""

    def __init__(self, H, W, K, ref, cur, grad, xy, kz, cur_ptrs):
        self.H, self.W, self.K, self.ref, self.cur, self.grad, self.xy, self.kz, self.cur_ptrs = H, W, K, ref, cur, grad, xy, kz, cur_ptrs


class RenderedPair:
    """What RenderedScene.render gives for one pair, all of it independent of pyramid levels: the keyframe's world pose (pk, qk);
    the level-0 keyframe `ref`, current image `cur` (uint8, H * W) and float32 z-map `depth` (H x W) on the device; the initial
    knots in the keyframe's camera on the host (kt perturbed, kt_gt not, kR) and their device buffers dkt, dkR that the LM
    updates in place; t0 of the knots' segment, capture and exposure time (cap, exp; capt, expt on the device) and the host
    start-index array.  `levels`: the RenderedLevel list the class holding the pair adds (RenderedPairBatch: level 0 alone)."""

    def __init__(self, pk, qk, ref, cur, depth, kt, kR, kt_gt, t0, cap, exp, capt, expt, dkt, dkR, start):
        self.pk, self.qk, self.ref, self.cur, self.depth = pk, qk, ref, cur, depth
        self.kt, self.kR, self.kt_gt, self.t0, self.cap, self.exp = kt, kR, kt_gt, t0, cap, exp
        self.capt, self.expt, self.dkt, self.dkR, self.start, self.levels = capt, expt, dkt, dkR, start, []


class RenderedScene:
    """What is per SEQUENCE in the rendered workloads (RenderedPairBatch, RenderedPairPyramids): a textured plane at z = D, a camera
    on a ground-truth world spline (loop_spline, knots every 0.5), B + 1 frames frame_dt apart of which frame b is pair b's
    keyframe and frame b + 1 its blurred current image, and one perturbation of the initial knots per pair.  The B perturbations
    are drawn up front in pair order: pair b's is the b-th draw whoever renders it and whichever pairs are rendered (a rank
    that builds only its own pairs, or a checker that re-renders single pairs, sees the pairs the whole batch holds).
    `render(b, ref, cur)` is the one pair renderer.  The host part (timing, knots, perturbations) needs no GPU: with
    device = "cpu" and ctx = None everything but `render` works."""

    def __init__(self, ctx, B, H, W, device, seed, D, frame_dt, exp, perturb):
        import torch
        self.ctx, self.B, self.H, self.W, self.device, self.D, self.frame_dt, self.exp = ctx, B, H, W, device, D, frame_dt, exp
        self.dtk, self.t0w, self.t_first = 0.5, 0.0, 0.55  # frame times t_first + i * frame_dt never straddle a knot (multiples of 0.5 +- exp)
        self.n_world = int((self.t_first + (B + 2) * frame_dt + exp) / self.dtk) + 5
        self.kt_w, self.kR_w = loop_spline(self.n_world, self.dtk)
        self.ktw, self.kRw = np.ascontiguousarray(self.kt_w.ravel()), np.ascontiguousarray(self.kR_w.ravel())
        self.intr = np.array([W / 2.0, W / 2.0, W / 2.0, H / 2.0])
        self.base = torch.from_numpy(synth.texture_image(H, W, seed=seed, octaves=(32, 16, 8, 4))).to(device)
        self.xs = torch.arange(W, dtype=torch.float64, device=device)[None, :].expand(H, W)
        self.ys = torch.arange(H, dtype=torch.float64, device=device)[:, None].expand(H, W)
        self.pat = torch.from_numpy(synth.PATTERN8).to(device)
        rng = np.random.default_rng(seed)
        self.perts = [rng.normal(0, perturb, (4, 3)) for _ in range(B)]

    def times(self, b):
        """(time of pair b's keyframe, capture time of its current frame)."""
        return self.t_first + b * self.frame_dt, self.t_first + (b + 1) * self.frame_dt

    def segment(self, b):
        """Index of the world-spline segment that holds the whole exposure of pair b's current frame."""
        tc = self.times(b)[1]
        idx = int((tc - self.exp * 0.5 - self.t0w) / self.dtk)
        assert int((tc + self.exp * 0.5 - self.t0w) / self.dtk) == idx and idx + 4 <= self.n_world
        return idx

    def render(self, b, ref, cur):
        """Pair b as a RenderedPair.  The sharp keyframe and the blurred current frame are rendered INTO ref and cur (uint8 device
        tensors of H * W: the caller allocates them where it needs them, e.g. as level 0 of a pyramid).  Waits for the device once the
        images and the torch-computed z-map are queued: both are complete before a detector reads them on the context's stream."""
        import torch
        L, H, W, D, intr, exp, dtk, device = self.ctx.lib, self.H, self.W, self.D, self.intr, self.exp, self.dtk, self.device
        tk, tc = self.times(b)
        pk, qk = np.zeros(3), np.zeros(4)
        capi.check(L.mbavo_spline_get_pose(4, self.t0w, dtk, capi.dp(self.ktw), capi.dp(self.kRw), self.n_world, float(tk), capi.dp(pk),
                                           capi.dp(qk), None, None), "mbavo_spline_get_pose")
        for (t, e, ns, dst) in ((tk, 0.0, 2, ref), (tc, exp, 8, cur)):
            capi.check(L.mbavo_synthesize_blur(self.base.data_ptr(), H, W, float(D), capi.dp(intr), 4, self.t0w, dtk, capi.dp(self.ktw),
                                               capi.dp(self.kRw), self.n_world, float(t), float(e), ns, dst.data_ptr(), None),
                       "mbavo_synthesize_blur")
        # z-depth of the plane z = D (plane frame) in the keyframe camera (camera -> plane pose (qk, pk))
        x, y, z, w = qk
        r2 = (2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y))
        rz = (self.xs - intr[2]) / intr[0] * r2[0] + (self.ys - intr[3]) / intr[1] * r2[1] + r2[2]
        depth = ((D - pk[2]) / rz).to(torch.float32).contiguous()
        torch.cuda.synchronize()
        # knots of the segment that holds the current frame's exposure, in the keyframe's camera
        idx = self.segment(b)
        qk_inv = np.array([-qk[0], -qk[1], -qk[2], qk[3]])
        kt_gt = np.stack([_qrot(qk_inv, self.kt_w[idx + i] - pk) for i in range(4)])
        kR = np.stack([_qmul(qk_inv, self.kR_w[idx + i]) for i in range(4)])
        kR /= np.linalg.norm(kR, axis=1, keepdims=True)
        kt = kt_gt + self.perts[b]
        t0 = self.t0w + idx * dtk
        start = np.array([synth.segment_start_index(tc, t0, dtk)], np.int32)
        assert start[0] == 0
        return RenderedPair(pk=pk, qk=qk, ref=ref, cur=cur, depth=depth, kt=kt, kR=kR, kt_gt=kt_gt, t0=t0, cap=tc, exp=exp,
                            capt=torch.tensor([tc], dtype=torch.float64, device=device),
                            expt=torch.tensor([exp], dtype=torch.float64, device=device),
                            dkt=torch.from_numpy(kt.ravel().copy()).to(device), dkR=torch.from_numpy(kR.ravel().copy()).to(device),
                            start=start)


# keyframe formats (mbavo_problem.grad_fp16): dtype and elements per pixel of the image d_ref_dIxy points at, the entry that fills it
_KEYFRAME_FORMATS = {0: ("float32", 2, "mbavo_image_gradients_u8"),       # float gradient pairs
                     1: ("float16", 2, "mbavo_image_gradients_u8_half"),  # IEEE half pairs (lossless for central differences of an 8-bit image)
                     2: ("int32", 1, "mbavo_pack_keyframe_u8")}           # packed keyframe: intensity + both differences in one word per pixel


class _RenderedPairs:
    """What RenderedPairBatch and RenderedPairPyramids share: ONE RenderedScene (`scene`), whose `render` gives every pair's
    images, z-map, times and knots, so pair b of either class is the same pair bit for bit; `_add_level` for one pyramid level
    of a pair (keyframe image in its format, detect_level, fill_problem); and the access to the pairs: `pair(b)`, the RenderedPair
    of pair b with its `levels` (None for a pair the object did not render), `knots(b)` and `reset_knots()`."""

    def _add_level(self, ctx, q, p, l, ref, cur, S, cell, thresh, cap_kp, margin, grad_fp16=0):
        """Level l of pair p from that level's images: appended to p.levels, its problem entry q filled."""
        import torch
        sc = self.scene
        Hl, Wl = sc.H >> l, sc.W >> l
        dtype, per_px, entry = _KEYFRAME_FORMATS[int(grad_fp16)]
        grad = torch.empty(Hl * Wl * per_px, dtype=getattr(torch, dtype), device=ref.device)
        capi.check(getattr(ctx.lib, entry)(ref.data_ptr(), Hl, Wl, grad.data_ptr(), None), entry)
        xy, kz, K = detect_level(ctx, ref, Hl, Wl, l, sc.H, sc.W, cell, thresh, p.depth, cap_kp, margin)
        cur_ptrs = torch.tensor([cur.data_ptr()], dtype=torch.int64, device=ref.device)
        p.levels.append(RenderedLevel(H=Hl, W=Wl, K=K, ref=ref, cur=cur, grad=grad, xy=xy, kz=kz, cur_ptrs=cur_ptrs))
        fill_problem(q, S, 1, K, 8, 4, Hl, Wl, ref, grad, cur_ptrs, xy, kz, sc.pat, sc.intr, p.capt, p.expt, p.t0, sc.dtk, p.dkt, p.dkR,
                     p.start, self.huber, level=l, grad_fp16=grad_fp16)

    def pair(self, b):
        """The RenderedPair of pair b, or None where the object did not render it."""
        return self._rendered[b]

    def knots(self, b):
        """(knots_t, knots_R) device tensors of pair b."""
        return self._rendered[b].dkt, self._rendered[b].dkR

    def reset_knots(self):
        """Initial control knots back into the device buffers (the LM calls update them in place)."""
        import torch
        for p in self._rendered:
            if p is not None:
                p.dkt.copy_(torch.from_numpy(p.kt.ravel().copy()))
                p.dkR.copy_(torch.from_numpy(p.kR.ravel().copy()))
        torch.cuda.synchronize()


class RenderedPairBatch(_RenderedPairs):
    """BASELINE configs[2]/[3] as the configs describe them: B independent keyframe pairs = B consecutive frames of ONE
    synthetic blurred sequence (a textured plane, a camera on a ground-truth spline; generate_synthetic_data.cpp:127-214),
    every pair with its OWN keyframe image (the sharp rendering at the keyframe's time), its own gradient image, its own
    grid-selected keypoints with depths read from its own z-depth map, its own current image (the motion-blurred
    rendering one frame later, mbavo_synthesize_blur) and its own control knots (the ground-truth spline expressed in the
    keyframe's camera by left-multiplication -- the cumulative B-spline is left-invariant -- plus a small perturbation).
    Everything is rendered and detected on the GPU and stays there; `host_problem(b)` downloads one pair for the parity
    tests.  Same interface as DeviceWorkload (array, step, frame_blocks, valid, probs).  The sequence and the pairs come from
    RenderedScene, shared with RenderedPairPyramids: pair b here is level 0 of pair b there.  Level 0 alone, a border of 20
    pixels, the keyframe in any of the three formats (grad_fp16); `pairs`: the pairs to render (a rank may build only its own;
    the entries of the others stay zero-filled, their `pair(b)` is None)."""

    def __init__(self, ctx, B, H=480, W=640, S=8, k=4, device="cuda:0", seed=1, huber=10.0, D=7.5, frame_dt=0.1, exp=0.04,
                 cell=30, thresh=4.0, perturb=2e-3, pairs=None, grad_fp16=False):
        import torch
        self.B, self.k, self.S, self.H, self.W, self.device, self.huber = B, k, S, H, W, device, huber
        self.E = synth.packed_len(k)
        self.scene = sc = RenderedScene(ctx, B, H, W, device, seed, D, frame_dt, exp, perturb)
        self.intr, self.D, self.kt_w, self.kR_w = sc.intr, D, sc.kt_w, sc.kR_w
        self.array = (capi.Problem * B)()
        self.probs, self._rendered = [], []
        own = set(range(B) if pairs is None else pairs)
        cap_kp = (H // cell + 1) * (W // cell + 1)
        for b in range(B):
            p = None
            if b in own:
                p = sc.render(b, torch.empty(H * W, dtype=torch.uint8, device=device), torch.empty(H * W, dtype=torch.uint8, device=device))
                self._add_level(ctx, self.array[b], p, 0, p.ref, p.cur, S, cell, thresh, cap_kp, 20, grad_fp16)
            self.probs.append(_PairInfo(S, k, 4, 1, p.levels[0].K if p else 0, 8, H, W, grad_fp16))
            self._rendered.append(p)
        self.nbf = B
        self.frame_blocks = torch.zeros(self.nbf * self.E, dtype=torch.float64, device=device)
        self.valid = torch.zeros(self.nbf, dtype=torch.float64, device=device)
        torch.cuda.synchronize()

    def count_distinct_taps(self, ctx, pairs=None):
        """the COMPULSORY bytes of a semi-dense pair are the bytes of its DISTINCT tap locations (36 B per
        pixel-sample is the no-reuse upper bound).  Counts them on the host for the pairs' actual keypoints and knots: patch
        centre at blur sample S/2 (compute_local_patches_xy.cu:19-49), the truncated pixel (A3), for every blur sample the warp
        through its pose (compute_pixel_intensity.h:117-144) and the 2 x 2 tap window anchored at min(floor, size - 2) -- plain
        numpy (the figure is a count of locations; a last-place difference in a coordinate moves no window).  Sets, per pair,
        probs[b].distinct = (keyframe pixels, current pixels, 128-byte lines of the row-major images) and
        probs[b].image_bytes = the distinct-tap bytes in the pair's keyframe format."""
        L = ctx.lib
        H, W, S = self.H, self.W, self.S
        fx, fy, cx, cy = [float(v) for v in self.intr]
        pat = synth.PATTERN8.reshape(-1, 2).astype(np.int64)
        per_px = {0: (1, 8), 1: (1, 4), 2: (0, 4)}  # keyframe bytes per distinct pixel: (u8 image, gradient / packed image)
        for b in (range(self.B) if pairs is None else pairs):
            h = self.pair(b)
            if h is None:
                continue
            xy = h.levels[0].xy.cpu().numpy().reshape(-1, 2)
            kz = h.levels[0].kz.cpu().numpy()
            kt, kR = np.ascontiguousarray(h.kt.ravel()), np.ascontiguousarray(h.kR.ravel())
            poses = []
            for i in range(S):
                t = h.cap - h.exp * 0.5 + i * h.exp / (S - 1 + 1e-8)
                pp, qq = np.zeros(3), np.zeros(4)
                capi.check(L.mbavo_spline_get_pose(self.k, h.t0, 0.5, capi.dp(kt), capi.dp(kR), 4, float(t), capi.dp(pp), capi.dp(qq),
                                                   None, None), "mbavo_spline_get_pose")
                x, y, z, w = qq
                R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                              [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                              [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
                poses.append((R, pp))
            Rm, tm = poses[S // 2]
            P3r = np.stack([kz * (xy[:, 0] - cx) / fx, kz * (xy[:, 1] - cy) / fy, kz], 1)
            P3c = (P3r - tm) @ Rm                       # R^T (P - t)
            cen = np.stack([P3c[:, 0] / P3c[:, 2] * fx + cx, P3c[:, 1] / P3c[:, 2] * fy + cy], 1)
            px = (cen[:, None, 0] + pat[None, :, 0]).astype(np.int64)   # truncation toward zero, as (int)
            py = (cen[:, None, 1] + pat[None, :, 1]).astype(np.int64)
            inb = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
            d = np.broadcast_to(kz[:, None], px.shape)[inb]
            px, py = px[inb], py[inb]
            cur_ids = np.unique(py * W + px)
            rx, ry = (px - cx) / fx, (py - cy) / fy
            zh = 1.0 / np.sqrt(1.0 + rx * rx + ry * ry)
            ray = np.stack([rx * zh, ry * zh, zh], 1)
            ids = []
            for R, t in poses:
                rr = ray @ R.T
                lam = (d - t[2]) / rr[:, 2]
                Pr = rr * lam[:, None] + t
                u, v = Pr[:, 0] / Pr[:, 2] * fx + cx, Pr[:, 1] / Pr[:, 2] * fy + cy
                ok = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
                x0 = np.minimum(np.floor(u[ok]).astype(np.int64), W - 2)
                y0 = np.minimum(np.floor(v[ok]).astype(np.int64), H - 2)
                for dy in (0, 1):
                    for dx in (0, 1):
                        ids.append((y0 + dy) * W + (x0 + dx))
            ref_ids = np.unique(np.concatenate(ids)) if ids else np.zeros(0, np.int64)
            fmt = self.probs[b].fmt
            b_img, b_grad = per_px[fmt]
            lines = len(np.unique(cur_ids // 128)) + (len(np.unique(ref_ids // 128)) if b_img else 0) + len(np.unique(ref_ids * b_grad // 128))
            self.probs[b].distinct = (int(len(ref_ids)), int(len(cur_ids)), int(lines))
            self.probs[b].image_bytes = int(len(ref_ids) * (b_img + b_grad) + len(cur_ids))
        return self

    def host_problem(self, b):
        """Pair b as a numpy Prob (images downloaded): what the oracle is given in the parity tests."""
        h = self.pair(b)
        lv = h.levels[0]
        H, W = self.H, self.W
        return Prob(h.ref.cpu().numpy().reshape(H, W), [h.cur.cpu().numpy().reshape(H, W)],
                    lv.xy.cpu().numpy().reshape(-1, 2), lv.kz.cpu().numpy(), synth.PATTERN8, self.intr, self.S, self.k, 4,
                    [h.cap], [h.exp], h.t0, 0.5, h.kt, h.kR, self.huber,
                    grad=lv.grad.float().cpu().numpy().reshape(H, W, 2))

    def step(self, ctx, with_hessian=True, out=None, merged=True):
        _step(self, ctx, with_hessian, out, merged)


class RenderedPairPyramids(_RenderedPairs):
    """The B rendered keyframe pairs of RenderedPairBatch (the same RenderedScene and pair renderer: own keyframe, depth map,
    current image and perturbed knots per pair), each with an L-level pyramid: per level the keyframe and current image reduced
    on the device (mbavo_pyramid_levels_u8), the level's gradient image (mbavo_image_gradients_u8) and its semi-dense keypoints
    detected against the pair's own depth map (mbavo_detect_semidense: grid cells of cell / 1.414^l, as the front end's; a border
    of max(4, 20 >> l) pixels).  Intrinsics are scaled per level (1 / 2^l), S blur samples on every level.  `array`: B x L
    mbavo_problem, pair-major (entry b*L + l = pair b at level l), the levels of a pair sharing its times, start index and knot
    buffers -- what mbavo_lm_batch_levels takes.  `pair(b)` names the level-0 inputs (ref = sharp, depth, cur = blur) and the
    levels; `levels_of(b)` gives pair b as mbavo_optimize_trajectory takes it."""

    def __init__(self, ctx, B, L=4, H=480, W=640, S=8, k=4, device="cuda:0", seed=1, huber=10.0, D=7.5, frame_dt=0.1, exp=0.04,
                 cell=30, thresh=4.0, perturb=2e-3):
        import torch
        assert 1 <= L <= 8 and (H >> (L - 1)) >= 8 and (W >> (L - 1)) >= 8
        self.B, self.L, self.k, self.S, self.H, self.W, self.device, self.huber = B, L, k, S, H, W, device, huber
        self.scene = sc = RenderedScene(ctx, B, H, W, device, seed, D, frame_dt, exp, perturb)
        self.intr, self.pat = sc.intr, sc.pat
        self.array = (capi.Problem * (B * L))()
        self._rendered = []
        for b in range(B):
            refs = [torch.empty((H >> l) * (W >> l), dtype=torch.uint8, device=device) for l in range(L)]
            curs = [torch.empty((H >> l) * (W >> l), dtype=torch.uint8, device=device) for l in range(L)]
            p = sc.render(b, refs[0], curs[0])
            for lv in (refs, curs):
                ptrs = (C.c_void_p * L)(*[a.data_ptr() for a in lv])
                capi.check(ctx.lib.mbavo_pyramid_levels_u8(ctx.handle, ptrs, H, W, L), "mbavo_pyramid_levels_u8")
            for l in range(L):
                cl = int(cell / 1.414 ** l)  # (the detector scales the level-0 cell itself, FeatureDetectorBase.cpp:56-64)
                cap_kp = ((H >> l) // cl + 1) * ((W >> l) // cl + 1)
                self._add_level(ctx, self.array[b * L + l], p, l, refs[l], curs[l], S, cell, thresh, cap_kp, max(4, 20 >> l))
            self._rendered.append(p)
        torch.cuda.synchronize()

    def levels_of(self, b):
        """Pair b for mbavo_optimize_trajectory: (mbavo_level array, level-0 intrinsics, cap, exp, t0, dt, initial knots_t, knots_R)."""
        h = self.pair(b)
        lv = (capi.Level * self.L)()
        for q, d in zip(lv, h.levels):
            q.H, q.W, q.K, q.P, q.S = d.H, d.W, d.K, 8, self.S
            q.d_ref_img, q.d_ref_dIxy, q.d_cur_imgs = d.ref.data_ptr(), d.grad.data_ptr(), d.cur_ptrs.data_ptr()
            q.d_kp_xy, q.d_kp_z, q.d_pattern = d.xy.data_ptr(), d.kz.data_ptr(), self.pat.data_ptr()
        return (lv, self.intr, np.array([h.cap]), np.array([h.exp]), h.t0, 0.5, h.kt.ravel().copy(), h.kR.ravel().copy(), self.huber)


def rendered_inputs(rpp):
    """The level-0 inputs of a RenderedPairPyramids as mbavo_pairs_prepare takes them: (sharp, depth, blur), B x H x W device tensors
    (uint8, float32, uint8), stacked from what every pair holds by name (ref, depth, cur)."""
    import torch
    H, W = rpp.H, rpp.W
    pairs = [rpp.pair(b) for b in range(rpp.B)]
    return (torch.stack([p.ref.view(H, W) for p in pairs]).contiguous(), torch.stack([p.depth for p in pairs]).contiguous(),
            torch.stack([p.cur.view(H, W) for p in pairs]).contiguous())


def depth_dtypes(depth_format):
    """The tensor dtypes a depth map of that format (mbavo_pairs_opts.depth_format) may have: float32 for z (0) and ray distance
    (1); for format 2 uint16, or int16 holding the same 16 bits."""
    import torch
    return (torch.float32,) if depth_format in (0, 1) else tuple(getattr(torch, n) for n in ("uint16", "int16") if hasattr(torch, n))


def depth_to_z(ctx, depth_format, depth, intr, depth_unit=0.0, depth_max=0.0):
    """mbavo_depth_to_z on every map of a device tensor ([B x] H x W, contiguous, of the format's dtype): a float32 z tensor of
    the same shape, one launch per map on the context's stream, nothing waited for.  intr: level-0 (fx, fy, cx, cy)."""
    import torch
    assert depth.is_cuda and depth.is_contiguous() and depth.dim() in (2, 3) and depth.dtype in depth_dtypes(depth_format), (depth.dtype, depth_format)
    H, W = depth.shape[-2:]
    maps = depth.view(-1, H, W)
    out = torch.empty(maps.shape, dtype=torch.float32, device=depth.device)
    K = np.ascontiguousarray(intr, dtype=np.float64)
    assert K.size == 4
    for b in range(maps.shape[0]):
        capi.check(ctx.lib.mbavo_depth_to_z(ctx.handle, int(depth_format), maps[b].data_ptr(), H, W, capi.dp(K), float(depth_unit), float(depth_max),
                                            out[b].data_ptr()), "mbavo_depth_to_z")
    return out.view(depth.shape)


def camera_radtan(H, W, intr, dist):
    """An mbavo_camera_radtan: the raw H x W camera (fx, fy, cx, cy) with distortion (k1, k2, p1, p2)."""
    cam = capi.CameraRadTan()
    cam.H, cam.W = int(H), int(W)
    for i in range(4):
        cam.intrinsics[i], cam.dist[i] = float(intr[i]), float(dist[i])
    return cam


def camera_unified(H, W, intr, xi, dist=(0.0, 0.0, 0.0, 0.0)):
    """An mbavo_camera_unified: the raw H x W unified camera (fx, fy, cx, cy; mirror parameter xi) with distortion (k1, k2, p1, p2)."""
    cam = capi.CameraUnified()
    cam.H, cam.W, cam.xi = int(H), int(W), float(xi)
    for i in range(4):
        cam.intrinsics[i], cam.dist[i] = float(intr[i]), float(dist[i])
    return cam


def pairs_camera(cam, to_intr):
    """An mbavo_pairs_camera: one camera of a batch's set -- the raw camera `cam` (a camera_radtan or a camera_unified) and the
    pinhole camera to_intr (fx, fy, cx, cy at level 0) its pairs' undistorted images have."""
    out = capi.PairsCamera()
    unified = isinstance(cam, capi.CameraUnified)
    out.model, out.H, out.W, out.xi = (2 if unified else 1), cam.H, cam.W, (cam.xi if unified else 0.0)
    for i in range(4):
        out.intrinsics[i], out.dist[i], out.to_intrinsics[i] = cam.intrinsics[i], cam.dist[i], float(to_intr[i])
    return out


def undistort_map_batch(ctx, cams, H, W):
    """mbavo_undistort_map_batch: the n x H x W x 2 float32 maps of a sequence of pairs_camera in ONE launch on the context's
    stream, nothing waited for; map i is what undistort_map gives for camera i and its to_intrinsics."""
    import torch
    arr = (capi.PairsCamera * len(cams))(*cams)
    out = torch.empty((len(cams), H, W, 2), dtype=torch.float32, device="cuda:%d" % ctx.device_id)
    capi.check(ctx.lib.mbavo_undistort_map_batch(ctx.handle, len(cams), arr, int(H), int(W), out.data_ptr()), "mbavo_undistort_map_batch")
    return out


def undistort_points_batch(ctx, cams, points, want_ok=True):
    """mbavo_undistort_points_batch: raw points into the undistorted images of a sequence of pairs_camera in ONE launch on the
    context's stream, nothing waited for.  `points`: one n_i x 2 array of raw (u, v) per camera.  Returns (xy total x 2 float64,
    ok total uint8 or None) as device tensors, the rows one behind the other, and the host offsets; a point without a solution
    is (NaN, NaN) with ok 0."""
    import torch
    arr = (capi.PairsCamera * len(cams))(*cams)
    uv = [np.asarray(q, np.float64).reshape(-1, 2) for q in points]
    assert len(uv) == len(cams)
    offsets = np.zeros(len(cams) + 1, np.int32)
    offsets[1:] = np.cumsum([len(a) for a in uv])
    dev = "cuda:%d" % ctx.device_id
    d_uv = torch.from_numpy(np.ascontiguousarray(np.concatenate(uv) if uv else np.zeros((0, 2)))).to(dev)
    xy = torch.empty_like(d_uv)
    ok = torch.empty((int(offsets[-1]),), dtype=torch.uint8, device=dev) if want_ok else None
    capi.check(ctx.lib.mbavo_undistort_points_batch(ctx.handle, len(cams), arr, capi.ip(offsets), d_uv.data_ptr(), xy.data_ptr(),
                                                    ok.data_ptr() if want_ok else None), "mbavo_undistort_points_batch")
    return xy, ok, offsets


def undistort_map(ctx, cam, to_intr, H, W):
    """mbavo_undistort_map (or, for a camera_unified, mbavo_undistort_map_unified): the H x W x 2 float32 map [sx, sy] of the pinhole
    camera to_intr into the raw camera `cam`, a device tensor; one launch on the context's stream, nothing waited for."""
    import torch
    out = torch.empty((H, W, 2), dtype=torch.float32, device="cuda:%d" % ctx.device_id)
    K = np.ascontiguousarray(to_intr, dtype=np.float64)
    name = "mbavo_undistort_map_unified" if isinstance(cam, capi.CameraUnified) else "mbavo_undistort_map"
    capi.check(getattr(ctx.lib, name)(ctx.handle, C.byref(cam), capi.dp(K), int(H), int(W), out.data_ptr()), name)
    return out


def undistort_clearance(ctx, maps, Hs, Ws, L, radius):
    """mbavo_undistort_clearance_batch: the clearance pyramids of the maps of a device tensor ([n x] H x W x 2 float32, contiguous)
    into the Hs x Ws raw image -- an n x mbavo_undistort_clearance_bytes(H, W, L) uint8 device tensor, per map the levels 0 .. L-1
    one behind the other (`clearance_levels` splits a row); 1 or 3 launches (L > 4: one more) on the context's stream, nothing
    waited for.  radius 0: the plain valid pyramid."""
    import torch
    assert maps.is_cuda and maps.is_contiguous() and maps.dtype == torch.float32 and maps.dim() in (3, 4) and maps.shape[-1] == 2
    H, W = maps.shape[-3:-1]
    n = maps.numel() // (2 * H * W)
    nbytes = int(ctx.lib.mbavo_undistort_clearance_bytes(int(H), int(W), int(L)))
    if nbytes < 0:
        raise ValueError("mbavo_undistort_clearance_bytes(%d, %d, %d) = %d" % (H, W, L, nbytes))
    out = torch.empty((n, nbytes), dtype=torch.uint8, device=maps.device)
    capi.check(ctx.lib.mbavo_undistort_clearance_batch(ctx.handle, n, maps.data_ptr(), int(H), int(W), int(Hs), int(Ws), int(L), int(radius),
                                                       out.data_ptr()), "mbavo_undistort_clearance_batch")
    return out


def undistort_mask(ctx, raw_masks, maps):
    """mbavo_undistort_mask_batch: n raw-geometry masks ([n x] Hs x Ws uint8, a byte != 0 is usable) through n maps ([n x] H x W x 2
    float32), mask i through map i -- an n x H x W uint8 device tensor of 0 / 1; ONE launch on the context's stream, nothing waited
    for."""
    import torch
    assert raw_masks.is_cuda and raw_masks.is_contiguous() and raw_masks.dtype == torch.uint8 and raw_masks.dim() in (2, 3)
    assert maps.is_cuda and maps.is_contiguous() and maps.dtype == torch.float32 and maps.dim() in (3, 4) and maps.shape[-1] == 2
    Hs, Ws = raw_masks.shape[-2:]
    H, W = maps.shape[-3:-1]
    n = maps.numel() // (2 * H * W)
    assert raw_masks.numel() == n * Hs * Ws
    out = torch.empty((n, H, W), dtype=torch.uint8, device=maps.device)
    capi.check(ctx.lib.mbavo_undistort_mask_batch(ctx.handle, n, raw_masks.data_ptr(), int(Hs), int(Ws), maps.data_ptr(), int(H), int(W),
                                                  out.data_ptr()), "mbavo_undistort_mask_batch")
    return out


def mask_clearance(ctx, maps, masks, Hs, Ws, L, radius):
    """mbavo_mask_clearance_batch: undistort_clearance with caller-supplied masks ([n x] H x W uint8 in the undistorted geometry, a
    byte != 0 is usable) beside the maps, or -- maps None; Hs, Ws are then not read -- in their place.  masks None: the bytes of
    undistort_clearance.  The same packed n x bytes uint8 tensor, the same launches."""
    import torch
    assert maps is not None or masks is not None
    if maps is not None:
        assert maps.is_cuda and maps.is_contiguous() and maps.dtype == torch.float32 and maps.dim() in (3, 4) and maps.shape[-1] == 2
        H, W = maps.shape[-3:-1]
    if masks is not None:
        assert masks.is_cuda and masks.is_contiguous() and masks.dtype == torch.uint8 and masks.dim() in (2, 3)
        assert maps is None or tuple(masks.shape[-2:]) == (H, W)
        H, W = masks.shape[-2:]
    n = (maps.numel() // (2 * H * W)) if maps is not None else masks.numel() // (H * W)
    assert masks is None or masks.numel() == n * H * W
    nbytes = int(ctx.lib.mbavo_undistort_clearance_bytes(int(H), int(W), int(L)))
    if nbytes < 0:
        raise ValueError("mbavo_undistort_clearance_bytes(%d, %d, %d) = %d" % (H, W, L, nbytes))
    out = torch.empty((n, nbytes), dtype=torch.uint8, device=(maps if maps is not None else masks).device)
    capi.check(ctx.lib.mbavo_mask_clearance_batch(ctx.handle, n, maps.data_ptr() if maps is not None else None,
                                                  masks.data_ptr() if masks is not None else None, int(H), int(W), int(Hs), int(Ws), int(L),
                                                  int(radius), out.data_ptr()), "mbavo_mask_clearance_batch")
    return out


def clearance_levels(row, H, W, L):
    """One map's packed clearance pyramid (a row of undistort_clearance, tensor or array) as L views of (H >> l) x (W >> l)."""
    out, at = [], 0
    for l in range(L):
        h, w = H >> l, W >> l
        out.append(row[at:at + h * w].reshape(h, w))
        at += h * w
    return out


def undistort_u8(ctx, raw, map_xy):
    """mbavo_undistort_u8 on every image of a device tensor ([B x] Hs x Ws uint8, contiguous) through an H x W x 2 map: [B x] H x W
    uint8, one launch per image on the context's stream, nothing waited for."""
    import torch
    assert raw.is_cuda and raw.is_contiguous() and raw.dtype == torch.uint8 and raw.dim() in (2, 3)
    assert map_xy.is_cuda and map_xy.is_contiguous() and map_xy.dtype == torch.float32 and map_xy.dim() == 3 and map_xy.shape[2] == 2
    Hs, Ws = raw.shape[-2:]
    H, W = map_xy.shape[:2]
    imgs = raw.view(-1, Hs, Ws)
    out = torch.empty((imgs.shape[0], H, W), dtype=torch.uint8, device=raw.device)
    for b in range(imgs.shape[0]):
        capi.check(ctx.lib.mbavo_undistort_u8(ctx.handle, imgs[b].data_ptr(), Hs, Ws, map_xy.data_ptr(), H, W, out[b].data_ptr()), "mbavo_undistort_u8")
    return out.view(raw.shape[:-2] + (H, W))


def undistort_u8_batch(ctx, raw, map_xy):
    """mbavo_undistort_u8_batch: what undistort_u8 returns, in ONE launch for all images of `raw` (at most 65535)."""
    import torch
    assert raw.is_cuda and raw.is_contiguous() and raw.dtype == torch.uint8 and raw.dim() in (2, 3)
    assert map_xy.is_cuda and map_xy.is_contiguous() and map_xy.dtype == torch.float32 and map_xy.dim() == 3 and map_xy.shape[2] == 2
    Hs, Ws = raw.shape[-2:]
    H, W = map_xy.shape[:2]
    n = raw.numel() // (Hs * Ws)
    out = torch.empty(raw.shape[:-2] + (H, W), dtype=torch.uint8, device=raw.device)
    capi.check(ctx.lib.mbavo_undistort_u8_batch(ctx.handle, raw.data_ptr(), n, Hs, Ws, map_xy.data_ptr(), H, W, out.data_ptr()), "mbavo_undistort_u8_batch")
    return out


def photometric_table(G=None, scale=1.0):
    """mbavo_photometric_table (pure host): (return code, the 256 float32 entries) of the inverse response G (256 float64, None:
    the identity) under `scale`; the entries are as they were on a rejection (here: zeros)."""
    lut = np.zeros(256, np.float32)
    g = None if G is None else np.ascontiguousarray(G, dtype=np.float64)
    assert g is None or g.size == 256
    rc = capi.load().mbavo_photometric_table(None if g is None else g.ctypes.data_as(capi.c_dp), float(scale), lut.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, lut


def photometric_u8_batch(ctx, src, luts, inv=None, cal_of_image=None, out=None):
    """mbavo_photometric_u8_batch: the n_img images of `src` (device uint8, .. x H x W) through the tables `luts` (host, n_cal x 256
    float32) and the INVERSE vignettes `inv` (device float32 n_cal x H x W, or None), image i under calibration cal_of_image[i]
    (None: the one calibration, or image i's own), in ONE launch.  out: the destination (None: a new tensor; `src` itself: in place)."""
    import torch
    assert src.is_cuda and src.is_contiguous() and src.dtype == torch.uint8 and src.dim() >= 2
    H, W = src.shape[-2:]
    n_img = src.numel() // (H * W)
    luts = np.ascontiguousarray(luts, dtype=np.float32).reshape(-1, 256)
    n_cal = luts.shape[0]
    assert inv is None or (inv.is_cuda and inv.is_contiguous() and inv.dtype == torch.float32 and inv.numel() == n_cal * H * W)
    idx = None if cal_of_image is None else np.ascontiguousarray(cal_of_image, dtype=np.int32)
    assert idx is None or idx.size == n_img
    out = torch.empty_like(src) if out is None else out
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.numel() == src.numel()
    capi.check(ctx.lib.mbavo_photometric_u8_batch(ctx.handle, n_img, src.data_ptr(), H, W, n_cal, luts.ctypes.data_as(C.POINTER(C.c_float)),
                                                  None if inv is None else inv.data_ptr(), None if idx is None else capi.ip(idx), out.data_ptr()),
               "mbavo_photometric_u8_batch")
    return out


class PairBatch:
    """The library's batched input side (mbavo_pairs_*): B pairs x L levels prepared on the device in a constant number of
    launches.  `prepare` takes device tensors (sharp and blurred images B x H x W uint8, depth maps B x H x W: float32 z, or
    with depth_format 1 float32 ray distances, with 2 uint16 values of 1 / depth_unit metres),
    `set_motion` host arrays; `array` is the library-owned B x L mbavo_problem array, pair-major, that mbavo_lm_batch_levels
    takes as is.  Same defaults as RenderedPairPyramids (cell 30, threshold 4, border max(4, 20 >> l), the 8-pixel pattern).
    With undistort = 1 the images are raw Hs x Ws images of the camera given to `set_camera`, with 2 the depth maps too.
    With num_cameras = G the batch holds a set of G cameras (`set_cameras`: a list of pairs_camera and every pair's index) in
    place of the one camera; `intr` is then not used.  With valid_radius = r > 0 (needs undistort != 0) a keypoint is kept only
    where no pixel within r of it, on its level, has taken anything from outside the raw image.  With mask = 1 the batch holds
    one caller-supplied mask per camera (`set_masks`) beside that test; valid_radius may then be 0 .. 64 under any undistort.
    `prepare_points`, `update_points` and `track_frame_points` take, in place of the depth maps, one (xy, z) list of level-0
    keypoints per keyframe: the detector is not run (mbavo_pairs_prepare_points).  After `set_points_geometry(1)` those points are
    raw pixel coordinates of the pair's camera, inverted on the device."""

    def __init__(self, ctx, B, L=4, H=480, W=640, S=8, k=4, N=4, intr=None, huber=10.0, cell=30, thresh=4.0, border=None,
                 keyframe_format=0, pattern=None, every_candidate=False, depth_format=0, depth_unit=0.0, depth_max=0.0, undistort=0,
                 num_cameras=0, valid_radius=0, mask=0):
        self.ctx, self.B, self.L, self.H, self.W, self.k, self.N = ctx, B, L, H, W, k, N
        self.depth_format, self.undistort = int(depth_format), int(undistort)
        self.image_px = self.depth_px = H * W  # pixels of one image / one depth map as the caller passes them
        # (S and pattern: one value for every level, or a sequence with one per level)
        pats = pattern if isinstance(pattern, (list, tuple)) else [synth.PATTERN8 if pattern is None else pattern] * 8
        pats = [np.ascontiguousarray(q, dtype=np.int32) for q in pats]
        pat = pats
        o = capi.PairsOpts()
        o.B, o.L, o.H, o.W, o.spline_deg_k, o.N = B, L, H, W, k, N
        intr = np.array([W / 2.0, W / 2.0, W / 2.0, H / 2.0]) if intr is None else np.asarray(intr, np.float64)
        self.intr = intr
        for l in range(min(L, 8)):
            o.S[l], o.P[l] = (S[l] if hasattr(S, "__len__") else S), pats[l].size // 2
            o.pattern_xy[l] = pats[l].ctypes.data_as(capi.c_ip)
            o.border[l] = max(4, 20 >> l) if border is None else int(border[l] if hasattr(border, "__len__") else border)
        for i in range(4):
            o.intrinsics[i] = float(intr[i])
        o.huber_a, o.score_threshold, o.cell_H, o.cell_W, o.keyframe_format = huber, thresh, cell, cell, keyframe_format
        o.every_candidate = 1 if every_candidate else 0  # (no grid: every pixel above the threshold with a depth, `cell` is not read)
        o.depth_format, o.depth_unit, o.depth_max = int(depth_format), float(depth_unit), float(depth_max)
        o.undistort, o.num_cameras, o.valid_radius, o.mask = int(undistort), int(num_cameras), int(valid_radius), int(mask)
        self.opts, self.handle, self._pattern = o, capi.vp(), pat  # (the options point at the pattern)
        capi.check(ctx.lib.mbavo_pairs_create(ctx.handle, C.byref(o), C.byref(self.handle)), "mbavo_pairs_create")
        arr, n = C.POINTER(capi.Problem)(), C.c_int(0)
        capi.check(ctx.lib.mbavo_pairs_problems(self.handle, C.byref(arr), C.byref(n)), "mbavo_pairs_problems")
        assert n.value == B * L
        self.array = arr

    def set_camera(self, cam):
        """mbavo_pairs_set_camera / _set_camera_unified: the raw camera (camera_radtan or camera_unified) of an object made with
        undistort != 0; the return code."""
        entry = self.ctx.lib.mbavo_pairs_set_camera_unified if isinstance(cam, capi.CameraUnified) else self.ctx.lib.mbavo_pairs_set_camera
        rc = entry(self.handle, C.byref(cam))
        if rc == 0:
            self.image_px = cam.H * cam.W
            self.depth_px = cam.H * cam.W if self.undistort == 2 else self.H * self.W
        return rc

    def set_cameras(self, cams, camera_of_pair):
        """mbavo_pairs_set_cameras: the G cameras (a sequence of pairs_camera) of an object made with num_cameras = G and the
        camera index of every pair; the return code."""
        arr = (capi.PairsCamera * max(len(cams), 1))(*cams)
        idx = np.ascontiguousarray(camera_of_pair, dtype=np.int32)
        assert idx.size == self.B
        rc = self.ctx.lib.mbavo_pairs_set_cameras(self.handle, len(cams), arr, capi.ip(idx))
        if rc == 0 and self.undistort != 0:
            self.image_px = cams[0].H * cams[0].W
            self.depth_px = cams[0].H * cams[0].W if self.undistort == 2 else self.H * self.W
        return rc

    def set_masks(self, masks, geometry=0):
        """mbavo_pairs_set_masks on an object made with mask = 1: one uint8 mask per camera (max(num_cameras, 1) of them; a byte
        != 0 is usable), a contiguous device tensor -- geometry 0: H x W each, in the undistorted geometry; 1: Hs x Ws each, in the
        raw geometry, warped through the object's maps.  The return code."""
        import torch
        assert masks.is_cuda and masks.is_contiguous() and masks.dtype == torch.uint8
        px = self.H * self.W if geometry == 0 else self.image_px
        n = masks.numel() // px
        assert masks.numel() == n * px
        return self.ctx.lib.mbavo_pairs_set_masks(self.handle, int(geometry), int(n), masks.data_ptr())

    def set_photometric(self, G=None, vignette=None, scale=0.0, v_min=0.0):
        """mbavo_pairs_set_photometric: the inverse response curves G (n x 256 float64, None: the identity) and the vignettes
        (device float32, n maps in the geometry the images arrive in, None: none) of the n = max(1, num_cameras) cameras; scale and
        v_min 0: the defaults (1.0, 0.0625).  Later prepares, updates and track_frames take their images in through them.  The
        return code."""
        n = max(1, int(self.opts.num_cameras))
        g = None if G is None else np.ascontiguousarray(G, dtype=np.float64)
        assert g is None or g.size == n * 256
        if vignette is not None:
            import torch
            assert vignette.is_cuda and vignette.is_contiguous() and vignette.dtype == torch.float32 and vignette.numel() == n * self.image_px
        o = capi.PairsPhotocalOpts()
        o.scale, o.v_min = float(scale), float(v_min)
        return self.ctx.lib.mbavo_pairs_set_photometric(self.handle, n, None if g is None else g.ctypes.data_as(capi.c_dp),
                                                        None if vignette is None else vignette.data_ptr(), C.byref(o))

    def clear_photometric(self):
        """mbavo_pairs_clear_photometric: back to the uncalibrated intake; the return code."""
        return self.ctx.lib.mbavo_pairs_clear_photometric(self.handle)

    def photocal_stats(self):
        """(launches, synchronisations, D2H bytes) of the last set_photometric."""
        o = (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_photocal_stats(self.handle, o), "mbavo_pairs_photocal_stats")
        return tuple(int(v) for v in o)

    def set_detector(self, score=0, radius=0, threshold=0.0, reserved=None):
        """mbavo_pairs_set_detector: score 0 -- gradient magnitude, the object as created (also `score=None`: a NULL options
        pointer); 1 -- the corner score of a (2 radius + 1)^2 window with its own threshold.  Later prepares, updates and
        track_frames select by it.  The return code."""
        if score is None:
            return self.ctx.lib.mbavo_pairs_set_detector(self.handle, None)
        o = capi.PairsDetectorOpts()
        o.score, o.radius, o.score_threshold = int(score), int(radius), float(threshold)
        for i, v in enumerate(reserved or ()):
            o.reserved[i] = int(v)
        return self.ctx.lib.mbavo_pairs_set_detector(self.handle, C.byref(o))

    def detector_stats(self):
        """(score mode, radius, bytes of score slices held) of mbavo_pairs_detector_stats."""
        o = (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_detector_stats(self.handle, o), "mbavo_pairs_detector_stats")
        return tuple(int(v) for v in o)

    def set_points_geometry(self, geometry):
        """mbavo_pairs_set_points_geometry: 0 -- the points of later prepare_points / update_points / track_frame_points calls
        are in the undistorted geometry (the state at creation); 1 -- in the raw camera's (needs undistort != 0).  The return
        code."""
        return self.ctx.lib.mbavo_pairs_set_points_geometry(self.handle, int(geometry))

    def prepare(self, sharp, depth, blur):
        """Keypoint counts, B x L."""
        import torch
        for t, dt, px in ((sharp, (torch.uint8,), self.image_px), (depth, depth_dtypes(self.depth_format), self.depth_px), (blur, (torch.uint8,), self.image_px)):
            assert t.is_cuda and t.is_contiguous() and t.dtype in dt and t.numel() == self.B * px, (t.dtype, dt)
        counts = np.zeros((self.B, self.L), np.int32)
        capi.check(self.ctx.lib.mbavo_pairs_prepare(self.handle, sharp.data_ptr(), depth.data_ptr(), blur.data_ptr(), capi.ip(counts)),
                   "mbavo_pairs_prepare")
        return counts

    def _point_lists(self, points, rows):
        """`points`: one (xy n x 2, z n) pair of arrays per row -- level-0 pixel coordinates of the undistorted geometry (after
        set_points_geometry(1): of the raw camera's) and depths along the optical axis.  Returns (host offsets rows + 1, flat xy and z device tensors): the lists as mbavo_pairs_*_points
        take them."""
        import torch
        assert len(points) == rows
        xy = [np.asarray(q[0], np.float64).reshape(-1, 2) for q in points]
        z = [np.asarray(q[1], np.float64).reshape(-1) for q in points]
        assert all(len(a) == len(b) for a, b in zip(xy, z))
        offsets = np.zeros(rows + 1, np.int32)
        offsets[1:] = np.cumsum([len(a) for a in z])
        dev = self.ctx.device_id
        flat = lambda parts, shape: torch.from_numpy(np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(shape))).to("cuda:%d" % dev)
        return offsets, flat(xy, (0, 2)), flat(z, (0,))

    def prepare_points(self, sharp, blur, points):
        """mbavo_pairs_prepare_points: the caller's keypoints in place of the detector and the depth maps.  `points`: B pairs of
        arrays (xy n_b x 2, z n_b).  Keypoint counts, B x L."""
        import torch
        for t in (sharp, blur):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.numel() == self.B * self.image_px
        offsets, xy, z = self._point_lists(points, self.B)
        counts = np.zeros((self.B, self.L), np.int32)
        capi.check(self.ctx.lib.mbavo_pairs_prepare_points(self.handle, sharp.data_ptr(), blur.data_ptr(), capi.ip(offsets), xy.data_ptr(),
                                                           z.data_ptr(), capi.ip(counts)), "mbavo_pairs_prepare_points")
        return counts

    def update_points(self, blur, key_pairs=(), sharp=None, points=()):
        """mbavo_pairs_update_points: `update` with one (xy, z) list per listed pair in place of the depth maps.  Counts, B x L."""
        import torch
        keys = np.ascontiguousarray(key_pairs, dtype=np.int32)
        n = int(keys.size)
        for t, cnt in ([(blur, self.B * self.image_px)] if blur is not None else []) + ([(sharp, n * self.image_px)] if n else []):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.numel() == cnt
        offsets, xy, z = self._point_lists(points, n)
        counts = np.zeros((self.B, self.L), np.int32)
        capi.check(self.ctx.lib.mbavo_pairs_update_points(self.handle, blur.data_ptr() if blur is not None else None, n, capi.ip(keys) if n else None,
                                                          sharp.data_ptr() if n else None, capi.ip(offsets), xy.data_ptr(), z.data_ptr(),
                                                          capi.ip(counts)), "mbavo_pairs_update_points")
        return counts

    def track_frame_points(self, blur, cap, exp, lm_opts, thresholds, key_pairs=(), sharp=None, points=(), trace_cap=0):
        """mbavo_pairs_track_frame_points: `track_frame` with one (xy, z) list per listed pair in place of the depth maps."""
        import torch
        keys = np.ascontiguousarray(key_pairs, dtype=np.int32)
        n = int(keys.size)
        for t, cnt in [(blur, self.B * self.image_px)] + ([(sharp, n * self.image_px)] if n else []):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.numel() == cnt
        offsets, xy, z = self._point_lists(points, n)
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap, exp)]
        assert a[0].size == a[1].size == self.B
        counts = np.zeros((self.B, self.L), np.int32)
        out, res = (capi.PairsFrame * self.B)(), (capi.LmBatchResult * self.B)()
        trace = (capi.TraceRec * (self.B * trace_cap))() if trace_cap else None
        capi.check(self.ctx.lib.mbavo_pairs_track_frame_points(
            self.handle, blur.data_ptr(), n, capi.ip(keys) if n else None, sharp.data_ptr() if n else None, capi.ip(offsets), xy.data_ptr(),
            z.data_ptr(), capi.dp(a[0]), capi.dp(a[1]), C.byref(lm_opts), res, trace, int(trace_cap), float(thresholds[0]), float(thresholds[1]),
            float(thresholds[2]), out, capi.ip(counts)), "mbavo_pairs_track_frame_points")
        return out, counts, res, trace

    def set_motion(self, cap, exp, t0, dt, knots_t, knots_R):
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap, exp, t0, knots_t, knots_R)]
        assert a[0].size == a[1].size == a[2].size == self.B and a[3].size == self.B * 3 * self.N and a[4].size == self.B * 4 * self.N
        return self.ctx.lib.mbavo_pairs_set_motion(self.handle, capi.dp(a[0]), capi.dp(a[1]), capi.dp(a[2]), float(dt), capi.dp(a[3]), capi.dp(a[4]))

    def knots(self):
        """(knots_t B x N x 3, knots_R B x N x 4) as the device holds them now."""
        kt, kR = np.zeros((self.B, self.N, 3)), np.zeros((self.B, self.N, 4))
        capi.check(self.ctx.lib.mbavo_pairs_get_knots(self.handle, capi.dp(kt), capi.dp(kR)), "mbavo_pairs_get_knots")
        return kt, kR

    def update(self, blur, key_pairs=(), sharp=None, depth=None):
        """mbavo_pairs_update: new blurred frames for all pairs (B x H x W uint8 device tensor, or None: they stay) and new
        keyframes for the pairs listed (ascending; sharp n x H x W uint8, depth n x H x W in the object's depth format, in the
        order of the list).  Keypoint counts of all pairs, B x L."""
        import torch
        keys = np.ascontiguousarray(key_pairs, dtype=np.int32)
        n = int(keys.size)
        checks = [(blur, (torch.uint8,), self.B * self.image_px)] if blur is not None else []
        if n:
            checks += [(sharp, (torch.uint8,), n * self.image_px), (depth, depth_dtypes(self.depth_format), n * self.depth_px)]
        for t, dt, cnt in checks:
            assert t.is_cuda and t.is_contiguous() and t.dtype in dt and t.numel() == cnt, (t.dtype, dt)
        counts = np.zeros((self.B, self.L), np.int32)
        capi.check(self.ctx.lib.mbavo_pairs_update(self.handle, blur.data_ptr() if blur is not None else None, n, capi.ip(keys) if n else None,
                                                   sharp.data_ptr() if n else None, depth.data_ptr() if n else None, capi.ip(counts)),
                   "mbavo_pairs_update")
        return counts

    def assess(self, flow_mag0, flow_mag1, max_blur_kernel_mag):
        """mbavo_pairs_assess: a ctypes array of B PairsAssessment (keyframe verdict, averages, pose at the capture time)."""
        out = (capi.PairsAssessment * self.B)()
        capi.check(self.ctx.lib.mbavo_pairs_assess(self.handle, float(flow_mag0), float(flow_mag1), float(max_blur_kernel_mag), out),
                   "mbavo_pairs_assess")
        return out

    def initial_states(self, cap0, dt_frame):
        """The state trackFrame has after its first frame (blur_aware_direct_tracker.cpp:94-110), per pair: two identity knots
        starting at the first capture time, identity poses, zero velocity.  cap0: one time or B of them.  Needs N == 2."""
        assert self.N == 2
        cap0 = np.broadcast_to(np.asarray(cap0, np.float64), (self.B,))
        states = (capi.VoState * self.B)()
        for b, st in enumerate(states):
            st.t0, st.dt, st.N, st.is_first, st.prev_timestamp = float(cap0[b]), float(dt_frame), 2, 0, float(cap0[b])
            st.knots_R[3] = st.knots_R[7] = st.T_keyframe[6] = st.T_prev_b2w[6] = 1.0
        return states

    def set_states(self, states):
        """mbavo_pairs_set_states: a ctypes array (or sequence) of B VoState; the return code."""
        if not isinstance(states, C.Array):
            states = (capi.VoState * self.B)(*states)
        assert len(states) == self.B
        return self.ctx.lib.mbavo_pairs_set_states(self.handle, states)

    def get_states(self):
        states = (capi.VoState * self.B)()
        capi.check(self.ctx.lib.mbavo_pairs_get_states(self.handle, states), "mbavo_pairs_get_states")
        return states

    def predict(self, cap, exp):
        """mbavo_pairs_predict: the constant-velocity prediction of every pair on the device; the return code."""
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap, exp)]
        assert a[0].size == a[1].size == self.B
        return self.ctx.lib.mbavo_pairs_predict(self.handle, capi.dp(a[0]), capi.dp(a[1]))

    def hyp_opts(self, scales, twists, level=None, min_valid_frac=0, min_gain=0):
        """The mbavo_pairs_hyp_opts of `predict_hypotheses`: hypothesis m = 1 .. has scale scales[m - 1] and twist twists[m - 1]
        (6 numbers (v, w), or None for zero); hypothesis 0 is the predict's own.  level None: the coarsest, L - 1."""
        scales = [float(s) for s in scales]
        twists = [None] * len(scales) if twists is None else list(twists)
        assert len(twists) == len(scales) <= 15
        o = capi.PairsHypOpts()
        o.M, o.level = 1 + len(scales), self.L - 1 if level is None else int(level)
        o.min_valid_frac, o.min_gain = float(min_valid_frac), float(min_gain)
        for m, (s, tw) in enumerate(zip(scales, twists), start=1):
            o.scale[m] = s
            for j in range(6):
                o.twist[m][j] = 0.0 if tw is None else float(tw[j])
        return o

    def predict_hypotheses(self, cap, exp, scales, twists, level=None, min_valid_frac=0, min_gain=0, want_records=True):
        """mbavo_pairs_predict_hypotheses in predict's place: every pair starts from the cheapest of 1 + len(scales) motion
        hypotheses, costs taken at `level`.  Returns (return code, ctypes array of B PairsHyp or None); without records nothing
        is waited for."""
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap, exp)]
        assert a[0].size == a[1].size == self.B
        o = self.hyp_opts(scales, twists, level, min_valid_frac, min_gain)
        out = (capi.PairsHyp * self.B)() if want_records else None
        rc = self.ctx.lib.mbavo_pairs_predict_hypotheses(self.handle, capi.dp(a[0]), capi.dp(a[1]), C.byref(o), out)
        return rc, out

    def hyp_stats(self):
        """(launches, synchronisations, D2H bytes) of the last predict_hypotheses."""
        o = (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_hyp_stats(self.handle, o), "mbavo_pairs_hyp_stats")
        return tuple(int(v) for v in o)

    def commit(self, flow_mag0, flow_mag1, max_blur_kernel_mag):
        """mbavo_pairs_commit: a ctypes array of B PairsFrame (the assessment and the pose in the world)."""
        out = (capi.PairsFrame * self.B)()
        capi.check(self.ctx.lib.mbavo_pairs_commit(self.handle, float(flow_mag0), float(flow_mag1), float(max_blur_kernel_mag), out),
                   "mbavo_pairs_commit")
        return out

    def track_frame(self, blur, cap, exp, lm_opts, thresholds, key_pairs=(), sharp=None, depth=None, trace_cap=0):
        """mbavo_pairs_track_frame: update, predict, mbavo_lm_batch_levels and commit in one call.  thresholds: (flow_mag0,
        flow_mag1, max_blur_kernel_mag).  Returns (frames B PairsFrame, counts B x L, results B LmBatchResult, trace or None)."""
        import torch
        keys = np.ascontiguousarray(key_pairs, dtype=np.int32)
        n = int(keys.size)
        checks = [(blur, (torch.uint8,), self.B * self.image_px)] + (
            [(sharp, (torch.uint8,), n * self.image_px), (depth, depth_dtypes(self.depth_format), n * self.depth_px)] if n else [])
        for t, dt, cnt in checks:
            assert t.is_cuda and t.is_contiguous() and t.dtype in dt and t.numel() == cnt, (t.dtype, dt)
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap, exp)]
        assert a[0].size == a[1].size == self.B
        counts = np.zeros((self.B, self.L), np.int32)
        out, res = (capi.PairsFrame * self.B)(), (capi.LmBatchResult * self.B)()
        trace = (capi.TraceRec * (self.B * trace_cap))() if trace_cap else None
        capi.check(self.ctx.lib.mbavo_pairs_track_frame(
            self.handle, blur.data_ptr(), n, capi.ip(keys) if n else None, sharp.data_ptr() if n else None, depth.data_ptr() if n else None,
            capi.dp(a[0]), capi.dp(a[1]), C.byref(lm_opts), res, trace, int(trace_cap), float(thresholds[0]), float(thresholds[1]),
            float(thresholds[2]), out, capi.ip(counts)), "mbavo_pairs_track_frame")
        return out, counts, res, trace

    def report(self, max_chi_square_error, patch_cost=None, flags=None):
        """mbavo_pairs_report: a ctypes array of B PairsReport (pose information, covariance, flag counts at the knots as they
        are).  patch_cost / flags: optional contiguous device tensors of B x cap0 float64 / uint8 (cap0: level 0's keypoint
        capacity) that receive every pair's level-0 patch costs and chi-test flags."""
        import torch
        for t, dt in ((patch_cost, torch.float64), (flags, torch.uint8)):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == dt)
        out = (capi.PairsReport * self.B)()
        capi.check(self.ctx.lib.mbavo_pairs_report(self.handle, float(max_chi_square_error), out,
                                                   None if patch_cost is None else patch_cost.data_ptr(),
                                                   None if flags is None else flags.data_ptr()), "mbavo_pairs_report")
        return out

    def report_stats(self):
        """(launches, synchronisations, D2H bytes) of the last report."""
        o = (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_report_stats(self.handle, o), "mbavo_pairs_report_stats")
        return tuple(int(v) for v in o)

    def capacities(self):
        """Keypoint capacity of every level (h_cells_per_level of mbavo_pairs_plan): the row length of per-keypoint arrays."""
        nbytes, cells = C.c_longlong(0), (C.c_int * 8)()
        capi.check(self.ctx.lib.mbavo_pairs_plan(C.byref(self.opts), C.byref(nbytes), cells), "mbavo_pairs_plan")
        return [int(cells[l]) for l in range(self.L)]

    def refine_depths(self, level=0, apply=False, min_info=0.0, max_rel_step=0.0, z_min=0.0, z_max=0.0, g=None, h=None, cost=None, valid=None,
                      want_records=True):
        """mbavo_pairs_refine_depths at the knots as they are: per keypoint the gradient g and curvature h of its patch cost with
        respect to its depth and, with apply, the damped inverse-depth step written into the object's keypoint depths.  level -1:
        every level.  g / h / cost (float64) and valid (int32): optional contiguous device tensors of B x cap[level] entries (level
        -1: B x sum(cap)), cap = `capacities()`.  Returns (return code, ctypes array of B (level -1: B x L) PairsRefine or None);
        without records nothing is waited for."""
        import torch
        cap = self.capacities()
        need = self.B * (sum(cap) if int(level) < 0 else cap[min(max(int(level), 0), self.L - 1)])
        for t, dt in ((g, torch.float64), (h, torch.float64), (cost, torch.float64), (valid, torch.int32)):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.numel() >= need)  # (the kernel writes up to row b's K)
        o = capi.PairsRefineOpts()
        o.level, o.apply = int(level), int(apply)
        o.min_info, o.max_rel_step, o.z_min, o.z_max = float(min_info), float(max_rel_step), float(z_min), float(z_max)
        n = self.B * (self.L if int(level) < 0 else 1)
        out = (capi.PairsRefine * n)() if want_records else None
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self.ctx.lib.mbavo_pairs_refine_depths(self.handle, C.byref(o), out, ptr(g), ptr(h), ptr(cost), ptr(valid))
        return rc, out

    def refine_stats(self):
        """(launches, synchronisations, D2H bytes) of the last refine_depths."""
        o = (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_refine_stats(self.handle, o), "mbavo_pairs_refine_stats")
        return tuple(int(v) for v in o)

    def match_brightness(self, level=0, apply=False, want_records=True, **opts):
        """mbavo_pairs_match_brightness at the knots as they are: every pair's gain and offset I_cur = gain I_key + offset fitted on
        the aligned patches of `level` and, with apply, removed from the pair's current-frame pyramid inside the object.  opts:
        rounds, min_pixels, huber, min_var, gain_min, gain_max (0: the defaults).  Returns (return code, ctypes array of B
        PairsPhoto or None); without records nothing is waited for."""
        o = capi.PairsPhotoOpts()
        o.level, o.apply = int(level), int(apply)
        for key, v in opts.items():
            if key not in ("rounds", "min_pixels", "huber", "min_var", "gain_min", "gain_max"):
                raise TypeError("match_brightness: unknown option %r" % key)
            setattr(o, key, int(v) if key in ("rounds", "min_pixels") else float(v))
        out = (capi.PairsPhoto * self.B)() if want_records else None
        rc = self.ctx.lib.mbavo_pairs_match_brightness(self.handle, C.byref(o), out)
        return rc, out

    def photo_stats(self):
        """(launches, synchronisations, D2H bytes) of the last match_brightness."""
        o = (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_photo_stats(self.handle, o), "mbavo_pairs_photo_stats")
        return tuple(int(v) for v in o)

    def filter_depths(self, level=-1, apply=False, want_records=True, **opts):
        """mbavo_pairs_filter_depths at the knots as they are: every keypoint's depth evidence from the aligned frame fused into its
        filter state on the device (seeded anew where the pair's keypoints were rewritten) and, with apply, the fused depth written
        into the object's keypoint depths.  level -1: every level.  opts: min_info, max_rel_step, z_min, z_max, sigma_i,
        prior_rel_sigma, gate_chi2, reset.  Returns (return code, ctypes array of B (level -1: B x L) PairsFilter or None); without
        records nothing is waited for."""
        o = capi.PairsFilterOpts()
        o.level, o.apply = int(level), int(apply)
        for key, v in opts.items():
            if key not in ("min_info", "max_rel_step", "z_min", "z_max", "sigma_i", "prior_rel_sigma", "gate_chi2", "reset"):
                raise TypeError("filter_depths: unknown option %r" % key)
            setattr(o, key, int(v) if key == "reset" else float(v))
        n = self.B * (self.L if int(level) < 0 else 1)
        out = (capi.PairsFilter * n)() if want_records else None
        rc = self.ctx.lib.mbavo_pairs_filter_depths(self.handle, C.byref(o), out)
        return rc, out

    def filter_state(self):
        """The filter's state on the device as torch views, not copies: dict(mu, info (float64), n_obs, n_rej (int32), each B x
        sum(capacities()); offset: the first column of every level; ptr: the four raw device pointers).  Writable; raises before the first filter_depths."""
        import torch
        ptr = [C.c_void_p() for _ in range(4)]
        stride, off = C.c_longlong(0), (C.c_longlong * 8)()
        capi.check(self.ctx.lib.mbavo_pairs_filter_state(self.handle, *[C.byref(p) for p in ptr], C.byref(stride), off), "mbavo_pairs_filter_state")
        n = self.B * int(stride.value)

        def view(p, dt):
            iface = {"shape": (n,), "typestr": dt, "data": (int(p.value), False), "version": 2, "strides": None}
            holder = type("_DeviceSpan", (), {"__cuda_array_interface__": iface})()
            return torch.as_tensor(holder, device="cuda:%d" % self.ctx.device_id).view(self.B, int(stride.value))
        return dict(mu=view(ptr[0], "<f8"), info=view(ptr[1], "<f8"), n_obs=view(ptr[2], "<i4"), n_rej=view(ptr[3], "<i4"),
                    offset=[int(off[l]) for l in range(self.L)], ptr=tuple(int(p.value) for p in ptr))

    def filter_stats(self):
        """(launches, synchronisations, D2H bytes) of the last filter_depths."""
        o = (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_filter_stats(self.handle, o), "mbavo_pairs_filter_stats")
        return tuple(int(v) for v in o)

    def search_depths(self, num_candidates, rho_lo, rho_hi, level=-1, apply=False, relative=False, min_ratio=0.0, min_curv=0.0, z_min=0.0, z_max=0.0,
                      rho=None, cost_best=None, cost_second=None, curv=None, best=None, num_full=None, volume=None, want_records=True):
        """mbavo_pairs_search_depths at the knots as they are: every keypoint's patch cost at num_candidates inverse depths from
        rho_lo to rho_hi (relative: both times the keypoint's own inverse depth), the best one refined by a parabola and, with
        apply, the accepted depths written into the object's keypoint depths.  level -1: every level.  rho / cost_best /
        cost_second / curv (float64), best / num_full (int32): optional contiguous device tensors in refine_depths' layout; volume
        (float64): that layout times num_candidates.  Returns (return code, ctypes array of B (level -1: B x L) PairsSearch or
        None); without records nothing is waited for.  The filter is not told: pass reset=1 to the next filter_depths."""
        import torch
        cap = self.capacities()
        need = self.B * (sum(cap) if int(level) < 0 else cap[min(max(int(level), 0), self.L - 1)])
        f8, i4 = torch.float64, torch.int32
        for t, dt, n in ((rho, f8, 1), (cost_best, f8, 1), (cost_second, f8, 1), (curv, f8, 1), (best, i4, 1), (num_full, i4, 1),
                         (volume, f8, max(int(num_candidates), 0))):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.numel() >= need * n)
        o = capi.PairsSearchOpts()
        o.level, o.apply, o.num_candidates, o.relative = int(level), int(apply), int(num_candidates), int(relative)
        o.rho_lo, o.rho_hi, o.min_ratio, o.min_curv, o.z_min, o.z_max = float(rho_lo), float(rho_hi), float(min_ratio), float(min_curv), float(z_min), float(z_max)
        n = self.B * (self.L if int(level) < 0 else 1)
        out = (capi.PairsSearch * n)() if want_records else None
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self.ctx.lib.mbavo_pairs_search_depths(self.handle, C.byref(o), out, ptr(rho), ptr(cost_best), ptr(cost_second), ptr(curv), ptr(best),
                                                    ptr(num_full), ptr(volume))
        return rc, out

    def search_stats(self):
        """(launches, synchronisations, D2H bytes) of the last search_depths."""
        o = (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_search_stats(self.handle, o), "mbavo_pairs_search_stats")
        return tuple(int(v) for v in o)

    def smooth_depths(self, radius, min_support=1, max_rel_diff=0.1, strength=1.0, level=-1, apply=False, fill=False, sync_filter=False,
                      weights=0, max_intensity_diff=0, z_min=0.0, z_max=0.0, weight=None, rho=None, flags=None, support=None, want_records=True):
        """mbavo_pairs_smooth_depths: every keypoint's inverse depth replaced by a weighted mean over itself and the neighbours
        within `radius` pixels that agree with it (within max_rel_diff), filled from all neighbours where none agrees (fill), flagged
        where neither can be done; with apply the depths that stand are written into the object's keypoint depths.  No pose is read.
        level -1: every level.  weights: 0 ones, 1 the filter's info, 2 `weight` (float64).  rho (float64), flags (uint8), support
        (int32): optional contiguous device tensors in refine_depths' layout.  Returns (return code, ctypes array of B (level -1:
        B x L) PairsSmooth or None); without records nothing is waited for."""
        import torch
        cap = self.capacities()
        need = self.B * (sum(cap) if int(level) < 0 else cap[min(max(int(level), 0), self.L - 1)])
        for t, dt in ((weight, torch.float64), (rho, torch.float64), (flags, torch.uint8), (support, torch.int32)):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.numel() >= need)
        o = capi.PairsSmoothOpts()
        o.level, o.apply, o.fill, o.sync_filter, o.weights = int(level), int(apply), int(fill), int(sync_filter), int(weights)
        o.radius, o.min_support, o.max_intensity_diff = int(radius), int(min_support), int(max_intensity_diff)
        o.max_rel_diff, o.strength, o.z_min, o.z_max = float(max_rel_diff), float(strength), float(z_min), float(z_max)
        n = self.B * (self.L if int(level) < 0 else 1)
        out = (capi.PairsSmooth * n)() if want_records else None
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self.ctx.lib.mbavo_pairs_smooth_depths(self.handle, C.byref(o), out, ptr(weight), ptr(rho), ptr(flags), ptr(support))
        return rc, out

    def smooth_stats(self):
        """(launches, synchronisations, D2H bytes) of the last smooth_depths."""
        o = (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_smooth_stats(self.handle, o), "mbavo_pairs_smooth_stats")
        return tuple(int(v) for v in o)

    def carry_save(self, pairs, T, radius, deflate=1.0, weights=0, z_min=0.0, z_max=0.0, want_records=True):
        """mbavo_pairs_carry_save: the keypoints of the listed pairs (ascending indices) warped into their next keyframe and kept
        as carried points for `carry_adopt`.  T: len(pairs) x 7 (t, q xyzw), the pose of the new keyframe in the old one's frame
        (PairsFrame.a.T of the commit whose verdict was 1).  weights: 0 ones, 1 the filter's info.  Returns (return code, ctypes
        array of len(pairs) x L PairsCarrySave or None); without records nothing is waited for."""
        keys = np.ascontiguousarray(pairs, dtype=np.int32)
        T = np.ascontiguousarray(T, dtype=np.float64)
        assert T.size == 7 * keys.size
        o = capi.PairsCarrySaveOpts()
        o.weights, o.radius, o.deflate, o.z_min, o.z_max = int(weights), int(radius), float(deflate), float(z_min), float(z_max)
        out = (capi.PairsCarrySave * (max(int(keys.size), 1) * self.L))() if want_records else None
        rc = self.ctx.lib.mbavo_pairs_carry_save(self.handle, int(keys.size), capi.ip(keys), capi.dp(T), C.byref(o), out)
        return rc, out

    def carry_adopt(self, pairs, min_support=1, max_rel_diff=0.1, apply=False, seed_filter=False, z_min=0.0, z_max=0.0, prior_rel_sigma=0.0,
                    max_info=0.0, rho=None, info=None, count=None, flags=None, want_records=True):
        """mbavo_pairs_carry_adopt after the update that gave the listed pairs their new keypoints: every keypoint gathers a depth
        from the carried points within the save's radius (the foreground within max_rel_diff of the nearest); with apply the
        adopted depths are written, with seed_filter the filter's state as well.  rho, info (float64), count (int32), flags
        (uint8): optional contiguous device tensors of B x sum(capacities()).  Returns (return code, ctypes array of len(pairs) x L
        PairsCarryAdopt or None); without records nothing is waited for.  The listed pairs' carried sets are disarmed."""
        import torch
        keys = np.ascontiguousarray(pairs, dtype=np.int32)
        need = self.B * sum(self.capacities())
        for t, dt in ((rho, torch.float64), (info, torch.float64), (count, torch.int32), (flags, torch.uint8)):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.numel() >= need)
        o = capi.PairsCarryAdoptOpts()
        o.apply, o.seed_filter, o.min_support = int(apply), int(seed_filter), int(min_support)
        o.max_rel_diff, o.z_min, o.z_max, o.prior_rel_sigma, o.max_info = float(max_rel_diff), float(z_min), float(z_max), float(prior_rel_sigma), float(max_info)
        out = (capi.PairsCarryAdopt * (max(int(keys.size), 1) * self.L))() if want_records else None
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self.ctx.lib.mbavo_pairs_carry_adopt(self.handle, int(keys.size), capi.ip(keys), C.byref(o), out, ptr(rho), ptr(info), ptr(count), ptr(flags))
        return rc, out

    def carry_stats(self):
        """((launches, synchronisations, D2H bytes) of the last carry_save, the same of the last carry_adopt)."""
        s, a = (C.c_longlong * 3)(), (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_carry_save_stats(self.handle, s), "mbavo_pairs_carry_save_stats")
        capi.check(self.ctx.lib.mbavo_pairs_carry_adopt_stats(self.handle, a), "mbavo_pairs_carry_adopt_stats")
        return tuple(int(v) for v in s), tuple(int(v) for v in a)

    def prune_keypoints(self, pairs=None, level=-1, apply=False, drop_mask=0, flags=None, use_filter=False, min_info=0.0, min_obs=0, rej_limit=0,
                        check_depth=False, z_min=0.0, z_max=0.0, min_keep=0, keep=None, want_records=True):
        """mbavo_pairs_prune_keypoints: the keypoints of the listed pairs (ascending indices; None: every pair) that a criterion
        drops are removed from the object's own arrays on the device, depths and filter state moved along; `array[e].K` follows.
        flags (read) / keep (written): optional contiguous uint8 device tensors in refine_depths' layout for `level`; a flag byte
        f < 32 whose bit is set in drop_mask drops.  Returns (return code, ctypes array of len(pairs) (level -1: x L) PairsPrune or
        None); with apply the call always waits (it reads the new counts back), without apply and records it waits for nothing."""
        import torch
        cap = self.capacities()
        need = self.B * (sum(cap) if int(level) < 0 else cap[min(max(int(level), 0), self.L - 1)])
        for t in (flags, keep):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.numel() >= need)
        keys = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
        o = capi.PairsPruneOpts()
        o.level, o.apply, o.drop_mask, o.use_filter, o.check_depth = int(level), int(apply), int(drop_mask), int(use_filter), int(check_depth)
        o.min_info, o.min_obs, o.rej_limit, o.z_min, o.z_max, o.min_keep = float(min_info), int(min_obs), int(rej_limit), float(z_min), float(z_max), int(min_keep)
        n = (self.B if keys is None else max(int(keys.size), 1)) * (self.L if int(level) < 0 else 1)
        out = (capi.PairsPrune * n)() if want_records else None
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self.ctx.lib.mbavo_pairs_prune_keypoints(self.handle, 0 if keys is None else int(keys.size), None if keys is None else capi.ip(keys),
                                                      C.byref(o), ptr(flags), out, ptr(keep))
        return rc, out

    def prune_stats(self):
        """(launches, synchronisations, D2H bytes) of the last prune_keypoints."""
        o = (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_prune_stats(self.handle, o), "mbavo_pairs_prune_stats")
        return tuple(int(v) for v in o)

    def track_stats(self):
        """((launches, synchronisations, D2H bytes) of the last predict, the same of the last commit)."""
        o = (C.c_longlong * 6)()
        capi.check(self.ctx.lib.mbavo_pairs_track_stats(self.handle, o), "mbavo_pairs_track_stats")
        return tuple(int(v) for v in o[:3]), tuple(int(v) for v in o[3:])

    def step_stats(self):
        """((launches, synchronisations, D2H bytes) of the last update, the same of the last assess)."""
        u, a = (C.c_longlong * 3)(), (C.c_longlong * 3)()
        capi.check(self.ctx.lib.mbavo_pairs_update_stats(self.handle, u), "mbavo_pairs_update_stats")
        capi.check(self.ctx.lib.mbavo_pairs_assess_stats(self.handle, a), "mbavo_pairs_assess_stats")
        return tuple(int(v) for v in u), tuple(int(v) for v in a)

    def stats(self):
        """(kernel launches, stream synchronisations, D2H bytes) of the last prepare, device bytes held."""
        out = (C.c_longlong * 4)()
        capi.check(self.ctx.lib.mbavo_pairs_last_stats(self.handle, out), "mbavo_pairs_last_stats")
        return tuple(int(v) for v in out)

    def close(self):
        if self.handle and self.ctx.handle:  # (a closed context has freed its pair batches already)
            self.ctx.lib.mbavo_pairs_destroy(self.handle)
        self.handle, self.array = capi.vp(), None


class DeviceWorkload:
    """Uploads a list of Prob once; builds the mbavo_problem array (inputs resident in HBM)."""

    def __init__(self, probs, device="cuda:0"):
        import torch
        self.probs = probs
        self.keep = []
        cache = {}

        def up(a):
            key = (a.__array_interface__["data"][0], a.shape, a.dtype.str)
            if key not in cache:
                cache[key] = torch.from_numpy(a).to(device)
            return cache[key]

        B = len(probs)
        self._knots = []
        self.array = (capi.Problem * B)()
        for b, p in enumerate(probs):
            ref = up(p.ref)
            if int(p.grad_fp16) == 2:
                grad = up(synth.pack_keyframe(p.ref))
            elif p.grad_fp16:
                if not hasattr(p, "_grad_half"):
                    p._grad_half = np.ascontiguousarray(p.grad.astype(np.float16))
                grad = up(p._grad_half)
            else:
                grad = up(p.grad)
            curs = [up(c) for c in p.cur]
            cur_ptrs = torch.tensor([c.data_ptr() for c in curs], dtype=torch.int64, device=device)
            xy, z, pat = up(p.kp_xy), up(p.kp_z), up(p.pattern)
            cap, exp, kt, kR = up(p.cap), up(p.exp), up(p.knots_t), up(p.knots_R)
            out = up(p.outlier) if p.outlier is not None else None
            self.keep += [ref, grad, curs, cur_ptrs, xy, z, pat, cap, exp, kt, kR, out]
            fill_problem(self.array[b], p.S, p.F, p.K, p.P, p.N, p.H, p.W, ref, grad, cur_ptrs, xy, z, pat, p.intr, cap, exp, p.t0, p.dt,
                         kt, kR, p.start_idx, p.huber, grad_fp16=p.grad_fp16, outlier=out, num_bad=p.num_bad)
            self._knots.append((kt, kR))
        self.B = B
        self.k = probs[0].k
        self.E = synth.packed_len(self.k)
        self.nbf = sum(p.F for p in probs)
        self.frame_blocks = torch.zeros(self.nbf * self.E, dtype=torch.float64, device=device)
        self.valid = torch.zeros(self.nbf, dtype=torch.float64, device=device)
        torch.cuda.synchronize()

    def keep_knots(self, b):
        """(knots_t, knots_R) device tensors of problem b (updated in place by mbavo_lm_batch)."""
        return self._knots[b]

    def step(self, ctx, with_hessian=True, out=None, merged=True):
        """One GN-iteration evaluation of every problem (asynchronous on the context's stream); `out` replaces the
        default output tensor (double buffering under an asynchronous all-reduce)."""
        _step(self, ctx, with_hessian, out, merged)


def _step(w, ctx, with_hessian, out, merged):
    """One pass of the hot path over the workload's problem list.  With H / g the pass ends in the reference's unit
    (evaluate_cost_hessian_gradient, spline_update_step.cpp:97-241): every problem's merged system [cost | g (6N) | H (6N x 6N)]
    in `w.systems` on the device (mbavo_eval_batch_merged: the merge of :232-239 is part of the finalize step where every
    problem has one frame and N == k, a kernel behind it otherwise) next to the packed frame blocks; merged=False keeps
    mbavo_eval_batch alone (packed blocks only: what the batched LM and the multi-GPU collectives consume)."""
    import torch
    fb = w.frame_blocks if out is None else out
    if with_hessian and merged:
        if getattr(w, "systems", None) is None:
            w.systems = torch.zeros(sum(1 + 6 * int(w.array[b].N) + 36 * int(w.array[b].N) ** 2 for b in range(w.B)), dtype=torch.float64,
                                    device=fb.device)
        rc = ctx.lib.mbavo_eval_batch_merged(ctx.handle, w.B, w.array, w.k, fb.data_ptr(), w.systems.data_ptr(), None, w.valid.data_ptr())
    else:
        rc = ctx.lib.mbavo_eval_batch(ctx.handle, w.B, w.array, w.k, 1 if with_hessian else 0, fb.data_ptr(), None, w.valid.data_ptr())
    if rc != 0:
        raise RuntimeError("mbavo_eval_batch%s failed: %d" % ("_merged" if with_hessian and merged else "", rc))


def algorithmic_flops(probs, valid_pixels=None):
    """flops_alg(H,g) = PS*(363 + 48k) + PX*(2E + 12k + 13), counted from the
    reference source as written (every add/sub/mul/div/sqrt = 1)."""
    total = 0.0
    for i, p in enumerate(probs):
        px = p.F * p.K * p.P if valid_pixels is None else valid_pixels[i]
        E = synth.packed_len(p.k)
        total += px * p.S * (363 + 48 * p.k) + px * (2 * E + 12 * p.k + 13)
    return total


def algorithmic_bytes(probs, shard=None, upper=False):
    """compulsory HBM bytes: images once (ref u8 + gradient 2 x f32 + current u8 per frame),
    keypoints (xy, z), pose tables, packed output blocks.  shard = (mode, rank, world): the bytes of that rank's share
    of the workload -- 'frames': keyframe images and keypoints in full, its own frames' current images; 'keypoints': a
    1/world band of every image and of the keypoints; 'pairs': the pairs b % world == rank, whole."""
    total = 0.0
    seen = set()
    mode, rank, world = shard if shard is not None else ("none", 0, 1)
    for b, p in enumerate(probs):
        if mode == "pairs" and b % world != rank:
            continue
        E = synth.packed_len(p.k)
        f0, f1 = ((p.F * rank) // world, (p.F * (rank + 1)) // world) if mode == "frames" else (0, p.F)
        band = 1.0 / world if mode == "keypoints" else 1.0
        if hasattr(p, "image_bytes"):  # a device-resident pair with its own images (RenderedPairBatch)
            # (its distinct tap locations once count_distinct_taps() has run -- SURVEY 8(d)'s compulsory figure; `upper`: the
            # gather bound, no reuse at all)
            total += (p.image_bytes_upper if upper else p.image_bytes) * band
        for a in ([] if hasattr(p, "image_bytes") else [p.ref, p.grad] + list(p.cur[f0:f1])):
            key = a.__array_interface__["data"][0]
            if key not in seen:
                seen.add(key)
                total += a.nbytes * band
        total += p.K * band * 24 + (f1 - f0) * p.S * (7 + 21 * p.k) * 8 + (f1 - f0) * E * 8
    return total
