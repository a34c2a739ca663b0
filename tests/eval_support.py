"""Shared by the evaluation tests (mbavo_eval_batch and its kin against the oracle): the tolerances and their reasons, the
oracle's valid-pixel counts, the engine's last layout and kernel, the run through every evaluation entry point, and the seeded
random problems of tests/test_gpu_fuzz.py, which tools/fuzz_more.py runs over more seeds."""
import ctypes as C

import numpy as np

import scenes
from mba_vo_amd import synth

U = np.finfo(np.float64).eps / 2  # unit roundoff


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def tol(sc):
    """1e-9, or what ONE flipped fp32 bilinear weight may do to a SMALL problem: the kernel contracts the warp to FMAs,
    the oracle does not, and once in ~1e5 taps the last fp64 bit moves a fractional coordinate across an fp32 rounding
    boundary -- that pixel's intensity then changes by ~1e-7 of its value, i.e. the normalised sums by up to
    ~2e-6 / (number of residuals)."""
    return max(1e-9, 2e-6 / max(sc.K * sc.F * sc.P, 1))


def _random_scene_kwargs(rng, k, seed, S=None):
    S = int(rng.choice([1, 2, 3, 4, 8, 16])) if S is None else S
    P = int(rng.choice([1, 2, 3, 4, 8, 16]))
    kw = dict(S=S, F=int(rng.choice([1, 1, 2])), k=k, P=P, seed=seed)
    if P == 1 and rng.random() < 0.5:
        kw.update(H=int(rng.integers(12, 50)), W=int(rng.integers(16, 70)), kp="dense", margin=int(rng.integers(0, 3)))
    else:
        kw.update(K=int(rng.integers(1, 400)), kp=str(rng.choice(["random", "border"])))
    if rng.random() < 0.3:
        kw.update(outlier_frac=0.15)
    return kw


def random_problem_matches_oracle(orc, ctx, seed, tol=tol):
    """One seeded random problem through mbavo_eval_batch against the oracle; `tol`: the bound on the packed blocks."""
    rng = np.random.default_rng(1000 + seed)
    k = int(rng.choice([2, 4]))
    S = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 32, 64]))
    P = int(rng.choice([1, 1, 3, 8, 8, 13]))  # seeds fixed: do not reorder (see test_patch_sizes for 2 .. 128)
    F = int(rng.choice([1, 1, 2, 3]))
    dense = P == 1 and rng.random() < 0.6
    kw = dict(S=S, F=F, k=k, P=P, seed=seed + 50)
    if dense:
        H, W = int(rng.integers(12, 60)), int(rng.integers(16, 90))
        kw.update(H=H, W=W, kp="dense", margin=int(rng.integers(0, 3)))
    else:
        kw.update(K=int(rng.integers(1, 700)), kp=str(rng.choice(["random", "border"])))
    if S >= 32:
        kw.update(trans_scale=0.002, rot_scale=0.02)
    if rng.random() < 0.3:
        kw.update(outlier_frac=0.15)
    if rng.random() < 0.3:
        kw.update(huber=float(rng.choice([0.1, 1.0, 30.0])))
    sc = scenes.Scene(**kw)
    p, keep = sc.oracle_problem(orc)
    ro = orc.evaluate(p)
    d = scenes.DeviceScene(sc, vec2d=bool(seed % 2) and not dense)
    fb, pc, valid = scenes.gpu_eval_batch(ctx, [d], k)
    assert rel(fb, ro["frame_blocks"]) < tol(sc), kw
    E = sc.E
    want_pc = ro["patch_blocks"].reshape(-1, E)[:, 0]
    # per-patch costs: exact, except where an fp64 rounding difference of the warp (the kernel contracts to FMAs, the
    # oracle does not) moves a tap coordinate across an fp32 rounding boundary -- one bilinear weight then changes by
    # one ulp (6e-8 of that pixel's intensity); at most a few patches per thousand
    got_pc = pc.ravel()[:want_pc.size]
    mism = got_pc != want_pc
    assert mism.sum() <= max(2, int(0.01 * want_pc.size)), (int(mism.sum()), want_pc.size, kw)
    assert np.abs(got_pc - want_pc).max() <= 1e-5 * max(np.abs(want_pc).max(), 1e-300), kw
    fc, _, _ = scenes.gpu_eval_batch(ctx, [d], k, with_hessian=False)
    assert np.abs(fc[:, 0] - fb[:, 0]).max() <= 1e-11 * max(np.abs(fb[:, 0]).max(), 1e-300), kw


def random_batch_matches_oracle(orc, ctx, seed, tol=tol):
    """Several seeded random problems in ONE mbavo_eval_batch call, each against the oracle's result for it alone."""
    rng = np.random.default_rng(7000 + seed)
    k = int(rng.choice([2, 4]))
    B = int(rng.integers(2, 7))
    same_S = int(rng.choice([4, 8, 16])) if seed % 2 else None
    kws = [_random_scene_kwargs(rng, k, 300 + 10 * seed + b, S=same_S) for b in range(B)]
    scs = [scenes.Scene(**kw) for kw in kws]
    dscs = [scenes.DeviceScene(sc) for sc in scs]
    fb, pc, valid = scenes.gpu_eval_batch(ctx, dscs, k)
    fc, _, _ = scenes.gpu_eval_batch(ctx, dscs, k, with_hessian=False)
    f0 = p0 = 0
    for sc, kw in zip(scs, kws):
        p, keep = sc.oracle_problem(orc)
        ro = orc.evaluate(p)
        want = ro["frame_blocks"].reshape(sc.F, sc.E)
        assert rel(fb[f0:f0 + sc.F], want) < tol(sc), kw
        assert np.abs(fc[f0:f0 + sc.F, 0] - want[:, 0]).max() <= tol(sc) * max(np.abs(want[:, 0]).max(), 1e-300), kw
        want_pc = ro["patch_blocks"].reshape(-1, sc.E)[:, 0]
        got_pc = pc[p0:p0 + want_pc.size]
        assert (got_pc != want_pc).sum() <= max(2, int(0.01 * want_pc.size)), kw
        assert np.abs(got_pc - want_pc).max() <= 1e-5 * max(np.abs(want_pc).max(), 1e-300), kw
        f0 += sc.F
        p0 += want_pc.size


def oracle_valid_counts(orc, sc):
    O = orc.lib()
    k, S, F, K, P = sc.k, sc.S, sc.F, sc.K, sc.P
    poses, Jt, JR = np.zeros(F * S * 7), np.zeros(F * S * 9 * k), np.zeros(F * S * 12 * k)
    O.orc_compute_virtual_camera_poses(S, F, orc.dp(sc.cap), orc.dp(sc.exp), k, sc.t0, sc.dt, orc.dp(sc.knots_t),
                                       orc.dp(sc.knots_R), orc.dp(poses), orc.dp(Jt), orc.dp(JR), None)
    c = np.zeros(F * K * 2)
    O.orc_compute_local_patches_xy(S, F, orc.dp(poses), orc.dp(sc.kp_xy), orc.dp(sc.kp_z), K, orc.dp(sc.intr), orc.dp(c))
    # use an all-255 current image so that a valid pixel can never have residual exactly 0
    cur = np.full((sc.H, sc.W), 255, np.uint8)
    ref = np.minimum(sc.ref, 254)
    curs = (orc.c_u8p * F)(*[orc.u8p(cur)] * F)
    res = np.zeros(F * K * P)
    O.orc_compute_pixel_jacobian_residual(orc.u8p(ref), None, curs, S, F, orc.dp(poses), k, None, None, orc.dp(c),
                                          orc.dp(sc.kp_z), K, orc.ip(sc.pattern), P, orc.dp(sc.intr), sc.H, sc.W,
                                          orc.dp(res), None)
    return (res.reshape(F, K * P) != 0).sum(1).astype(np.float64)


def layout(ctx):
    out = (C.c_int * 8)()
    assert ctx.lib.mbavo_last_layout(ctx.handle, out) == 0
    return dict(zip(("ntiles", "nbf", "max_slot_tiles", "sp_logs", "flat", "empty", "num_cus", "nprob"), list(out)))


def group_tol(n_tiles):
    """Bound on the difference between two sums of the same n tile partials grouped differently, relative to the block's largest
    entry.  A recursive sum of n terms is off by at most (n - 1) u sum_t |p_t|, so two groupings differ by at most 2 (n - 1) u
    sum_t |p_t|.  Every partial is a sum over pixels of w [rho, J r, J J^T] with Huber weights w >= 0: the H partials are positive
    semi-definite, so sum_t |H_t[a, b]| <= sum_t sqrt(H_t[a, a] H_t[b, b]) <= sqrt(H[a, a] H[b, b]) (Cauchy-Schwarz), and
    likewise sum_t |g_t[a]| <= sqrt(2 cost H[a, a]) <= cost + H[a, a]: the absolute sums stay within twice the block's largest
    entry.  Hence 4 (n - 1) u; with n the most tiles in one slot of either run.  1e-13 -- the bound of
    test_many_small_problems_flat_finalize -- holds up to n = 113; beyond it the bound grows with n."""
    return max(1e-13, 4 * max(n_tiles - 1, 0) * U)


def run(mbavo, ctx, k, scs, ds):
    """H/g and cost-only through mbavo_eval_batch, merged systems through both entry points, with the witnesses of each."""
    import torch
    B, E = len(ds), synth.packed_len(k)
    arr = (mbavo.capi.Problem * B)(*[d.problem() for d in ds])
    nbf = sum(sc.F for sc in scs)
    npatch = sum(sc.F * sc.K for sc in scs)
    nsys = sum(1 + 6 * sc.N + 36 * sc.N * sc.N for sc in scs)
    z = lambda n, v=0.0: torch.full((max(n, 1),), v, dtype=torch.float64, device="cuda:0")
    fb, pc, valid = z(nbf * E), z(npatch), z(nbf)
    fc, pcc, validc = z(nbf * E), z(npatch), z(nbf)
    fb_m, sys_m, sys_a = z(nbf * E, -3.0), z(nsys, -1.0), z(nsys, -2.0)
    lib, h = ctx.lib, ctx.handle
    assert lib.mbavo_eval_batch(h, B, arr, k, 1, fb.data_ptr(), pc.data_ptr(), valid.data_ptr()) == 0
    kern, lay = lib.mbavo_last_kernel(h).decode(), layout(ctx)
    assert lib.mbavo_eval_batch(h, B, arr, k, 0, fc.data_ptr(), pcc.data_ptr(), validc.data_ptr()) == 0
    kern_c, lay_c = lib.mbavo_last_kernel(h).decode(), layout(ctx)
    assert lib.mbavo_merge_device(h, B, arr, k, fb.data_ptr(), sys_a.data_ptr()) == 0
    assert lib.mbavo_eval_batch_merged(h, B, arr, k, fb_m.data_ptr(), sys_m.data_ptr(), None, None) == 0
    kern_m, lay_m = lib.mbavo_last_kernel(h).decode(), layout(ctx)
    torch.cuda.synchronize()
    n = lambda t, m: t.cpu().numpy()[:m]
    return dict(fb=n(fb, nbf * E).reshape(nbf, E), pc=n(pc, npatch), valid=n(valid, nbf), fc=n(fc, nbf * E).reshape(nbf, E)[:, 0],
                pcc=n(pcc, npatch), validc=n(validc, nbf), fb_m=n(fb_m, nbf * E).reshape(nbf, E), sys_m=n(sys_m, nsys),
                sys_a=n(sys_a, nsys), kern=kern, kern_c=kern_c, kern_m=kern_m, lay=lay, lay_c=lay_c, lay_m=lay_m)


def per_pixel_kernel(kern):
    """The instantiation that computes the per-patch costs: the pose prologue (k_fused's last argument) and the single launch
    (k_fused_sp's last argument) only change what happens before and after the pixel loop."""
    return kern.rsplit(",", 1)[0]
