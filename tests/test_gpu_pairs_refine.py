"""mbavo_pairs_refine_depths on the device, through the C ABI, against the numpy restatement (tests/pairs_refine_ref.py) run on
entries rebuilt on the host from the object's own device arrays (pairs_oracle.read_entry), and against mbavo_eval_batch.

Shapes: B = 3 pairs of 48 x 64 textures at L = 2, grid cells of 8, border 1 (patches near the rim leave the image: keypoints that
are not full).  Cases: k = 2 / N = 2, k = 4 / N = 4 and N = 6; S = 3 and S = 8; patterns of P = 1, 4, 5 and 8; the three keyframe
formats; an every-candidate object (K > 256: several tiles shared by several workgroups, whose sums meet in workgroup order) and a
prepare_points object whose lists put several points on one pixel; the rendered pairs of tests/pairs_refine_scene.py (true depths)
for the oracle's difference quotient and the Gauss-Newton property.

Bound.  Integer outputs are identical.  Doubles: per array, max |device - restatement| / max |restatement| <= BOUND = 8 x the
largest such figure measured over these cases on an MI355X (the device's prologue rounds the pose entries in another order than
the host spline the restatement uses), which is below the 1e-9 of tests/test_gpu_fullsize.py.  Every figure is printed before it
is asserted (-s)."""
import ctypes as C

import numpy as np
import pytest

import pairs_depth_support as ds
import pairs_device as dv
import pairs_oracle as po
import pairs_refine_ref as ref
import pairs_refine_scene as sc
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -2
B, L, H, W, CELL, THR = 3, 2, 48, 64, 8, 4.0
MEASURED = 1.32e-14  # the largest relative difference seen over these cases on an MI355X (profiles/r30_pairs_refine.txt)
BOUND = 1e-9 if MEASURED == 0.0 else min(8 * MEASURED, 1e-9)
PAT1 = np.array([[0, 0]], np.int32)
PAT4 = np.array([[0, 0], [1, 0], [0, 1], [-1, -1]], np.int32)
PAT5 = np.array([[0, 0], [2, 0], [0, 2], [-2, 0], [0, -2]], np.int32)
# (k, N, segment the samples lie on, S, pattern, keyframe_format)
CASES = [(2, 2, 0, 3, None, 0), (4, 4, 0, 3, PAT4, 1), (4, 6, 1, 8, PAT5, 2), (4, 4, 0, 8, PAT1, 0), (2, 2, 0, 8, PAT5, 2), (4, 6, 2, 3, None, 1)]
_IMAGES = {}


def _images():
    if not _IMAGES:
        rng = np.random.default_rng(30)
        sharp = np.stack([synth.texture_image(H, W, seed=60 + 3 * b, octaves=(16, 8, 4)) for b in range(B)])
        blur = np.stack([np.clip(np.roll(sharp[b], (1, -1), (0, 1)).astype(np.int32) + rng.integers(-4, 5, (H, W)), 0, 255).astype(np.uint8) for b in range(B)])
        depth = rng.uniform(1.0, 3.0, (B, H, W)).astype(np.float32)
        _IMAGES.update(sharp=np.ascontiguousarray(sharp), blur=np.ascontiguousarray(blur), depth=depth)
    return _IMAGES


def _motion(k, N, start, rotate_only=False):
    rng = np.random.default_rng(11)
    kt, kR = np.zeros((B, N, 3)), np.zeros((B, N, 4))
    for b in range(B):
        kt[b], kR[b] = synth.trajectory("harness", N, 0.004 * (b + 1), 0.01 * (b + 1))
        kt[b] += rng.normal(0, 0.02, 3)
        if rotate_only:
            kt[b] = 0.0
    cap = (start + 0.4 + 0.05 * np.arange(B)) * 0.5
    return dict(cap=cap, exp=np.full(B, 0.04), t0=np.zeros(B), dt=0.5, kt=kt, kR=kR)


def _object(ctx, k, N, S, pattern, fmt, pairs=B, dense=False):
    from mba_vo_amd import workloads
    return workloads.PairBatch(ctx, pairs, L=L, H=H, W=W, S=S, k=k, N=N, cell=0 if dense else CELL, thresh=THR, border=1, every_candidate=dense,
                               pattern=pattern, keyframe_format=fmt)


def _prepared(ctx, case, sel=slice(None), dense=False, depth=None, points=None, rotate_only=False):
    k, N, start, S, pattern, fmt = case
    c, m = _images(), _motion(k, N, start, rotate_only)
    n = len(range(B)[sel])
    pb = _object(ctx, k, N, S, pattern, fmt, pairs=n, dense=dense)
    d = c["depth"] if depth is None else depth
    sharp, blur = dv.dev(np.ascontiguousarray(c["sharp"][sel]), np.ascontiguousarray(c["blur"][sel]))
    if points is None:
        counts = pb.prepare(sharp, dv.dev(np.ascontiguousarray(d[sel]))[0], blur)
    else:
        counts = pb.prepare_points(sharp, blur, points)
    assert pb.set_motion(m["cap"][sel], m["exp"][sel], m["t0"][sel], m["dt"], m["kt"][sel], m["kR"][sel]) == 0
    return pb, counts


_arrays, _run = ds.refine_arrays, ds.refine_run


def _state_bytes(pb):
    """Everything of the object a refinement must not touch, and its depths: per entry (xy, z), then knots."""
    ents = [(dv.peek(pb.array[e].d_kp_xy, 2 * pb.array[e].K, np.float64), dv.peek(pb.array[e].d_kp_z, pb.array[e].K, np.float64)) for e in range(pb.B * pb.L)]
    return ents, pb.knots()


_rel = ds.rel


def _check(mbavo, ctx, pb, counts, k, tag, level=0, apply=False, **kw):
    """One call against the restatement (pairs_depth_support.refine_check at this file's BOUND); returns the largest relative difference."""
    return ds.refine_check(mbavo, ctx, pb, counts, k, tag, BOUND, level=level, apply=apply, **kw)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_kernel_against_restatement(mbavo, gpu_ctx, case):
    k = CASES[case][0]
    pb, counts = _prepared(gpu_ctx, CASES[case])
    try:
        assert (counts > 0).all()
        worst = _check(mbavo, gpu_ctx, pb, counts, k, "case %d report" % case, level=-1)
        worst = max(worst, _check(mbavo, gpu_ctx, pb, counts, k, "case %d apply" % case, level=0, apply=True))
        print("case %d: largest relative difference %.3g (bound %.3g)" % (case, worst, BOUND))
    finally:
        pb.close()


def test_some_keypoint_is_not_full_and_stays(mbavo, gpu_ctx):
    """border = 1: patches at the rim leave the current image -- zeros, valid < P, not moved."""
    pb, counts = _prepared(gpu_ctx, CASES[0])
    try:
        out, arr, cap = _run(pb, 0, True)
        seen = 0
        for b in range(B):
            K = counts[b, 0]
            part = arr["valid"][b, :K] < 8
            seen += int(part.sum())
            assert (arr["g"][b, :K][part] == 0).all() and (arr["h"][b, :K][part] == 0).all() and (arr["cost"][b, :K][part] == 0).all()
            assert out[b].num_full == K - part.sum()
        assert seen > 0
    finally:
        pb.close()


def test_cost_is_the_evaluations_patch_cost(mbavo, gpu_ctx):
    """cost scaled as the evaluation scales it, 1 / (K P) formed once and multiplied, equals mbavo_eval_batch(with_hessian = 0)'s
    d_patch_cost on the same entry with d_outlier = NULL, bit for bit, for full keypoints."""
    import torch
    capi = mbavo.capi
    for case in (CASES[0], CASES[2]):
        k = case[0]
        pb, counts = _prepared(gpu_ctx, case)
        try:
            out, arr, cap = _run(pb, 0)
            for b in range(B):
                q = capi.Problem()
                C.memmove(C.byref(q), C.byref(pb.array[b * L]), C.sizeof(capi.Problem))
                K, E = q.K, mbavo.load().mbavo_packed_len(k)
                fb, pc, valid = (torch.zeros(n, dtype=torch.float64, device="cuda:0") for n in (E, K, 1))
                capi.check(gpu_ctx.lib.mbavo_eval_batch(gpu_ctx.handle, 1, C.byref(q), k, 0, fb.data_ptr(), pc.data_ptr(), valid.data_ptr()), "mbavo_eval_batch")
                torch.cuda.synchronize()
                full = arr["valid"][b, :K] == q.P
                assert full.sum() > K // 2
                inv = 1.0 / float(K * q.P)
                assert np.array_equal((arr["cost"][b, :K] * inv)[full], pc.cpu().numpy()[full]), (case, b)
        finally:
            pb.close()


def test_apply_zero_changes_nothing_and_repeats(mbavo, gpu_ctx):
    pb, counts = _prepared(gpu_ctx, CASES[1])
    try:
        before = _state_bytes(pb)
        out1, arr1, _ = _run(pb, -1)
        out2, arr2, _ = _run(pb, -1)
        after = _state_bytes(pb)
        for (xy0, z0), (xy1, z1) in zip(before[0], after[0]):
            assert dv.same_bits(xy0, xy1) and dv.same_bits(z0, z1)
        assert dv.same_bits(before[1][0], after[1][0]) and dv.same_bits(before[1][1], after[1][1])
        assert bytes(out1) == bytes(out2) and all(dv.same_bits(arr1[key], arr2[key]) for key in arr1)
        # level = -1 is the L calls with level = l, bit for bit
        cap = pb.capacities()
        off = np.concatenate([[0], np.cumsum(cap)])
        for l in range(L):
            outl, arrl, _ = _run(pb, l)
            for b in range(B):
                assert bytes(outl[b]) == bytes(out1[b * L + l])
                assert all(dv.same_bits(arrl[key][b], np.ascontiguousarray(arr1[key][b, off[l]:off[l + 1]])) for key in arrl)
        # a B = 1 object holding pair b alone returns pair b's bits
        for b in range(B):
            one, _ = _prepared(gpu_ctx, CASES[1], sel=slice(b, b + 1))
            try:
                outb, arrb, _ = _run(one, -1)
                assert bytes(outb) == bytes(out1)[b * L * 32:(b + 1) * L * 32]
                assert all(dv.same_bits(arrb[key][0], np.ascontiguousarray(arr1[key][b])) for key in arrb)
            finally:
                one.close()
    finally:
        pb.close()


def test_apply_changes_only_counted_depths(mbavo, gpu_ctx):
    pb, counts = _prepared(gpu_ctx, CASES[2])
    try:
        before = _state_bytes(pb)
        rc, out = pb.refine_depths(level=1, apply=True)
        assert rc == 0
        after = _state_bytes(pb)
        assert dv.same_bits(before[1][0], after[1][0]) and dv.same_bits(before[1][1], after[1][1])
        for e, ((xy0, z0), (xy1, z1)) in enumerate(zip(before[0], after[0])):
            assert dv.same_bits(xy0, xy1)
            if e % L == 1:
                assert 0 < (z0 != z1).sum() <= out[e // L].num_moved
            else:
                assert dv.same_bits(z0, z1)
    finally:
        pb.close()


def test_clamp_and_depth_limits(mbavo, gpu_ctx):
    pb, counts = _prepared(gpu_ctx, CASES[0])
    try:
        z0 = [dv.peek(pb.array[b * L].d_kp_z, counts[b, 0], np.float64) for b in range(B)]
        out_free, _, _ = _run(pb, 0, False, max_rel_step=0.9)
        rc, out = pb.refine_depths(level=0, apply=True, max_rel_step=0.01)
        assert rc == 0
        for b in range(B):
            z1 = dv.peek(pb.array[b * L].d_kp_z, counts[b, 0], np.float64)
            assert out[b].num_moved > 0 and (np.abs(z0[b] / z1 - 1.0) <= 0.01 * (1 + 1e-12)).all()   # |d_rho| / rho
            assert out[b].sum_sq_rel <= out[b].num_moved * 1e-4 * (1 + 1e-12) and out_free[b].sum_sq_rel > out[b].sum_sq_rel
            dv.poke(pb.array[b * L].d_kp_z, z0[b])
        # a window no depth of these maps (1 .. 3, steps of at most 25 %) can land in: nothing moves
        for kw in (dict(z_min=50.0), dict(z_min=1e-3, z_max=0.5)):
            out, _, _ = _run(pb, 0, True, **kw)
            assert all(out[b].num_moved == 0 and out[b].sum_sq_rel == 0.0 for b in range(B))
            assert all(dv.same_bits(dv.peek(pb.array[b * L].d_kp_z, counts[b, 0], np.float64), z0[b]) for b in range(B))
    finally:
        pb.close()


def test_rotation_only_has_no_depth_information(mbavo, gpu_ctx):
    """A purely rotating pair: the warp does not depend on depth, h_rho is at rounding level and min_info keeps the depths."""
    pb, counts = _prepared(gpu_ctx, CASES[1], rotate_only=True)
    try:
        out, arr, _ = _run(pb, 0, True, min_info=1e-6)
        for b in range(B):
            K = counts[b, 0]
            z = dv.peek(pb.array[b * L].d_kp_z, K, np.float64)
            h_rho = z ** 4 * arr["h"][b, :K]
            print("rotation only, pair %d: largest h_rho %.3g" % (b, h_rho.max()))
            assert h_rho.max() < 1e-6 and out[b].num_moved == 0 and out[b].num_full > 0
    finally:
        pb.close()


def test_every_candidate_points_and_empty_level(mbavo, gpu_ctx):
    k = CASES[3][0]
    pb, counts = _prepared(gpu_ctx, CASES[3], dense=True)  # P = 1: tiles of 256 keypoints
    try:
        assert counts[:, 0].min() > 512
        _check(mbavo, gpu_ctx, pb, counts, k, "every candidate", level=-1)
    finally:
        pb.close()
    rng = np.random.default_rng(5)
    pts = []
    for b in range(B):
        xy = rng.integers(6, 40, (10, 2)).astype(np.float64)  # (level 1 holds 12 keypoints: the longest list a grid object of this size takes)
        xy[5:10] = xy[0:5]  # the same pixels again, with other depths
        pts.append((xy, rng.uniform(1.0, 3.0, 10)))
    pb, counts = _prepared(gpu_ctx, CASES[0], points=pts)
    try:
        assert (counts[:, 0] == 10).all()
        _check(mbavo, gpu_ctx, pb, counts, CASES[0][0], "points", level=-1, apply=True)
    finally:
        pb.close()
    pb, counts = _prepared(gpu_ctx, CASES[0], depth=np.zeros((B, H, W), np.float32))  # no depth anywhere: K = 0
    try:
        assert (counts == 0).all()
        out, arr, _ = _run(pb, -1, True)
        assert all((r.status, r.num_keypoints, r.num_full, r.num_moved, r.cost, r.sum_sq_rel) == (0, 0, 0, 0, 0.0, 0.0) for r in out)
        assert all((v == -7).all() for v in arr.values())
    finally:
        pb.close()


def test_pair_off_its_knots(mbavo, gpu_ctx):
    """mbavo_pairs_set_states can put a pair's times off its knots: that pair reports MBAVO_E_RANGE and nothing of it is written."""
    case = CASES[0]
    pb, counts = _prepared(gpu_ctx, case)
    try:
        good, arr_good, _ = _run(pb, 0)
        m = _motion(case[0], case[1], case[2])
        states = (mbavo.capi.VoState * B)()
        for b, st in enumerate(states):  # the same knots and times through the state; pair 1's knots start long after its frame
            st.t0, st.dt, st.N, st.is_first = (100.0 if b == 1 else float(m["t0"][b])), m["dt"], case[1], 0
            st.knots_t[:3 * case[1]] = list(m["kt"][b].ravel())
            st.knots_R[:4 * case[1]] = list(m["kR"][b].ravel())
            st.T_keyframe[6] = st.T_prev_b2w[6] = 1.0
        assert pb.set_states(states) == 0
        z1 = dv.peek(pb.array[1 * L].d_kp_z, counts[1, 0], np.float64)
        out, arr, _ = _run(pb, 0, True)
        assert (out[1].status, out[1].num_keypoints, out[1].num_full, out[1].num_moved) == (E_RANGE, counts[1, 0], 0, 0)
        assert np.isnan(out[1].cost) and np.isnan(out[1].sum_sq_rel)
        assert all((v[1] == -7).all() for v in arr.values()) and dv.same_bits(dv.peek(pb.array[1 * L].d_kp_z, counts[1, 0], np.float64), z1)
        for b in (0, 2):
            assert out[b].status == 0 and out[b].cost == good[b].cost and all(dv.same_bits(arr[key][b], arr_good[key][b]) for key in arr)
    finally:
        pb.close()


def test_rejected_calls_launch_nothing_and_counts(mbavo, gpu_ctx):
    capi, lib = mbavo.capi, gpu_ctx.lib
    case = CASES[0]
    k, N, start, S, pattern, fmt = case
    fresh = _object(gpu_ctx, k, N, S, pattern, fmt)
    try:
        out = (capi.PairsRefine * B)()
        ok = ref.opts_struct(capi)
        assert ref.call(lib, fresh.handle, ok, out) == E_ARG  # before the first prepare
        c = _images()
        fresh.prepare(*dv.dev(c["sharp"], c["depth"], c["blur"]))
        assert ref.call(lib, fresh.handle, ok, out) == E_ARG  # before the first motion
        assert fresh.refine_stats() == (0, 0, 0)
    finally:
        fresh.close()
    pb, counts = _prepared(gpu_ctx, case)
    try:
        before = _state_bytes(pb)
        out = (capi.PairsRefine * (B * L))()
        assert pb.refine_depths(level=-1)[0] == 0 and pb.refine_stats() == (1, 1, B * L * 32)
        bad = [None, ref.opts_struct(capi, level=-2), ref.opts_struct(capi, level=L), ref.opts_struct(capi, apply=2), ref.opts_struct(capi, apply=-1),
               ref.opts_struct(capi, min_info=-1.0), ref.opts_struct(capi, min_info=float("nan")), ref.opts_struct(capi, max_rel_step=float("inf")),
               ref.opts_struct(capi, max_rel_step=1.0), ref.opts_struct(capi, max_rel_step=-0.1), ref.opts_struct(capi, z_min=-1.0),
               ref.opts_struct(capi, z_max=float("nan")), ref.opts_struct(capi, z_min=2.0, z_max=1.0), ref.opts_struct(capi, z_max=0.005)]
        for o in bad:
            assert ref.call(lib, pb.handle, o, out) == E_ARG and pb.refine_stats() == (0, 0, 0), None if o is None else bytes(o)
        assert lib.mbavo_pairs_refine_depths(None, C.byref(ok), out, None, None, None, None) == E_ARG
        after = _state_bytes(pb)
        assert all(dv.same_bits(a[1], b_[1]) for a, b_ in zip(before[0], after[0]))
        # the stated cost: one launch; records: one synchronisation and B (or B L) records back; without records nothing is waited for
        assert pb.refine_depths(level=0)[0] == 0 and pb.refine_stats() == (1, 1, B * 32)
        assert pb.refine_depths(level=-1, want_records=False) == (0, None) and pb.refine_stats() == (1, 0, 0)
        assert pb.refine_depths(level=1, apply=True, want_records=False) == (0, None) and pb.refine_stats() == (1, 0, 0)
    finally:
        pb.close()


def _scene_object(ctx):
    """The rendered pairs of tests/pairs_refine_scene.py (true depths, ground-truth knots): B = 3, L = 2, grid cell 8, S = 3, k = 4."""
    from mba_vo_amd import workloads
    c, m = sc.scene(), sc.motion()
    pb = workloads.PairBatch(ctx, B, L=L, H=H, W=W, S=sc.S, k=sc.K_DEG, N=sc.N, cell=CELL, thresh=THR, border=4, huber=sc.HUBER)
    counts = pb.prepare(*dv.dev(np.ascontiguousarray(c["sharp"]), np.ascontiguousarray(c["depth"]), np.ascontiguousarray(c["blur"])))
    assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
    return pb, counts


def test_kernel_against_the_oracles_difference_quotient(mbavo, gpu_ctx, orc):
    """The kernel's g against K P (c_i(D + d) - c_i(D - d)) / (2 d) of the oracle's patch costs on entries rebuilt from the device,
    on the keypoints tests/test_pairs_refine_api.py selects (the oracle's patch centres keep their pixels, all valid); bound: that
    test's recorded gap x 4, the kernel being within 1e-9 of the restatement."""
    from mba_vo_amd import workloads
    capi = mbavo.capi
    c, m = sc.scene(), sc.motion()
    host = [sc.entry(b) for b in range(B)]
    # the very keypoints of the CPU test, handed over as the caller's points (an every-candidate object: every level has room for them)
    pb = workloads.PairBatch(gpu_ctx, B, L=L, H=H, W=W, S=sc.S, k=sc.K_DEG, N=sc.N, cell=0, thresh=THR, border=4, huber=sc.HUBER, every_candidate=True)
    try:
        sharp, blur = dv.dev(np.ascontiguousarray(c["sharp"]), np.ascontiguousarray(c["blur"]))
        counts = pb.prepare_points(sharp, blur, [(e["xy"], e["z"]) for e in host])
        assert (counts[:, 0] == host[0]["K"]).all() and pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
        out, arr, cap = _run(pb, 0)
        for b in range(B):
            e = po.read_entry(capi, pb.array[b * L], sc.K_DEG)
            assert np.array_equal(e["xy"], host[b]["xy"]) and np.array_equal(e["z"], host[b]["z"])
            q1, q2, use = sc.oracle_quotient(orc, gpu_ctx.lib, capi, e, 3e-3)
            g = arr["g"][b, :e["K"]]
            gap = np.abs(g - q1)[use].max() / np.abs(g[use]).max()
            print("pair %d: %d of %d keypoints qualify, gap %.3g of the largest |g| %.3g (bound %.3g)" % (b, use.sum(), e["K"], gap, np.abs(g[use]).max(), 4 * sc.GAP))
            assert 2 * use.sum() >= e["K"] and gap <= 4 * sc.GAP
    finally:
        pb.close()


def test_repeated_steps_lower_cost_and_depth_error(mbavo, gpu_ctx):
    """Level-0 depths perturbed by +-5 % around the TRUE depths of the rendered scene, knots fixed at the truth: over three
    apply = 1 calls the record's cost does not rise from one call to the next, and the median relative depth error of the full
    keypoints with h_rho above the batch median ends below its start.  A property of Gauss-Newton on this scene, checked with the
    restatement on the CPU first (tests/test_pairs_refine_api.py::test_gauss_newton_on_this_scene); later calls sit at the fixed
    point, where the cost moves by rounding-size amounts either way."""
    pb, counts = _scene_object(gpu_ctx)
    try:
        truth = [dv.peek(pb.array[b * L].d_kp_z, counts[b, 0], np.float64) for b in range(B)]
        for b in range(B):
            dv.poke(pb.array[b * L].d_kp_z, truth[b] * (1.0 + 0.05 * np.random.default_rng(3 + b).choice([-1.0, 1.0], truth[b].size)))
        costs, errs = [], []
        for it in range(4):
            z = [dv.peek(pb.array[b * L].d_kp_z, counts[b, 0], np.float64) for b in range(B)]
            out, arr, _ = _run(pb, 0, it < 3)
            h_rho = np.concatenate([z[b] ** 4 * arr["h"][b, :counts[b, 0]] for b in range(B)])
            full = np.concatenate([arr["valid"][b, :counts[b, 0]] == 8 for b in range(B)])
            rel = np.concatenate([np.abs(z[b] / truth[b] - 1.0) for b in range(B)])
            sel = full & (h_rho > np.median(h_rho[full]))
            costs.append([out[b].cost for b in range(B)])
            errs.append(float(np.median(rel[sel])))
        print("cost per pair, call by call:", np.array(costs).T, " median relative depth error:", errs)
        assert all(c1[b] <= c0[b] for c0, c1 in zip(costs, costs[1:]) for b in range(B))
        assert errs[-1] < errs[0]
    finally:
        pb.close()
