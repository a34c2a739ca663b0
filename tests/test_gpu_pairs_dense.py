"""mbavo_pairs_opts.every_candidate = 1: every semi-dense candidate of B pairs x L levels as keypoints, held bit for bit against the
per-image route (mbavo_pyramid_levels_u8, the gradient entry points, mbavo_detect_semidense with cell 0, then the border filter in
numpy) and against the numpy restatement of tests/pairs_dense_ref.py; the same bits for any B; mbavo_pairs_update against a fresh
prepare; launch counts that do not depend on B; mbavo_lm_batch_levels on the library's array against a hand-assembled one; and
mbavo_pairs_assess / mbavo_pairs_track_frame at K ~ 3 x 10^5.

The device walks a level in segments of 256 pixels, four to a workgroup (1024 pixels), and scans 256 segment counts per step:
the shapes below sit on both sides of each of those sizes."""
import ctypes as C
import math

import numpy as np
import pytest

import pairs_cases as cases
import pairs_dense_ref as dref
import pairs_device as dv
import pairs_ref
import pairs_step as ps
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

THR = 1.0  # below the ramp's gradient magnitude (sqrt 2)


def _pair(kind, H, W, seed):
    """(sharp, depth) of one pair.  flat: textured with a flat band (segments and rows without a candidate), depth everywhere;
    holes: textured, a depth map with holes (0 and a positive value below 1e-2); flat_holes: both; const: a constant image (K = 0
    on every level); ramp: (c + r) % 251 with depth 1 (K at its maximum on level 0)."""
    rng = np.random.default_rng(seed)
    img = synth.texture_image(H, W, seed=seed, octaves=(16, 8, 4))
    depth = rng.uniform(0.5, 3.0, (H, W)).astype(np.float32)
    if kind in ("flat", "flat_holes"):
        img[H // 5:H // 5 + max(3, H // 3), :] = 128  # whole rows
    if kind in ("holes", "flat_holes"):
        holes = rng.uniform(0, 1, (H, W))
        depth[holes < 0.15] = 0.0
        depth[(holes >= 0.15) & (holes < 0.2)] = 0.005
    if kind == "const":
        img[:] = 93
    if kind == "ramp":
        img, depth = dref.ramp(H, W), np.ones((H, W), np.float32)
    return img, depth


def _batch_inputs(kinds, H, W, seed=1):
    pairs = [_pair(kind, H, W, seed + 10 * b) for b, kind in enumerate(kinds)]
    other = synth.texture_image(H, W, seed=seed + 100, octaves=(16, 8, 4))
    blur = np.stack([np.roll(other, (3 * b + 1, 5 * b + 2), (0, 1)) for b in range(len(kinds))])
    return np.ascontiguousarray(np.stack([p[0] for p in pairs])), np.ascontiguousarray(np.stack([p[1] for p in pairs])), np.ascontiguousarray(blur)


def _per_image(mbavo, ctx, sharp_t, depth_t, blur_t, L, thr=THR):
    """What the per-image public calls give for B pairs, per (pair, level): both pyramids, the three gradient images and the
    keypoints of mbavo_detect_semidense(cell 0) before the border filter."""
    import torch
    lib, capi = ctx.lib, mbavo.capi
    B, H, W = sharp_t.shape
    out, keep = [], []
    for b in range(B):
        pyr = {}
        for name, src in (("ref", sharp_t[b]), ("cur", blur_t[b])):
            lv = [src.contiguous().view(-1).clone()] + [torch.empty((H >> l) * (W >> l), dtype=torch.uint8, device="cuda:0") for l in range(1, L)]
            ptrs = (C.c_void_p * L)(*[a.data_ptr() for a in lv])
            capi.check(lib.mbavo_pyramid_levels_u8(ctx.handle, ptrs, H, W, L), "mbavo_pyramid_levels_u8")
            pyr[name] = lv
        depth = depth_t[b].contiguous()
        for l in range(L):
            Hl, Wl = H >> l, W >> l
            ref = pyr["ref"][l]
            g0 = torch.empty(Hl * Wl * 2, dtype=torch.float32, device="cuda:0")
            g1 = torch.empty(Hl * Wl * 2, dtype=torch.float16, device="cuda:0")
            g2 = torch.empty(Hl * Wl, dtype=torch.int32, device="cuda:0")
            capi.check(lib.mbavo_image_gradients_u8(ref.data_ptr(), Hl, Wl, g0.data_ptr(), None), "gradients")
            capi.check(lib.mbavo_image_gradients_u8_half(ref.data_ptr(), Hl, Wl, g1.data_ptr(), None), "gradients_half")
            capi.check(lib.mbavo_pack_keyframe_u8(ref.data_ptr(), Hl, Wl, g2.data_ptr(), None), "pack_keyframe")
            cap = Hl * Wl
            xy = torch.zeros(cap * 2, dtype=torch.float64, device="cuda:0")
            kz = torch.zeros(cap, dtype=torch.float64, device="cuda:0")
            cnt = C.c_int(0)
            capi.check(lib.mbavo_detect_semidense(ctx.handle, ref.data_ptr(), Hl, Wl, l, H, W, 0, 0, float(thr), depth.data_ptr(),
                                                  xy.data_ptr(), kz.data_ptr(), cap, C.byref(cnt)), "mbavo_detect_semidense")
            K = cnt.value
            assert K <= cap
            keep.append((ref, pyr["cur"][l], g0, xy, kz))
            out.append(dict(ref=ref.cpu().numpy(), cur=pyr["cur"][l].cpu().numpy(), raw_K=K, raw_xy=xy.cpu().numpy()[:2 * K].reshape(-1, 2),
                            raw_z=kz.cpu().numpy()[:K], H=Hl, W=Wl, dev=keep[-1],
                            grads=[g0.cpu().numpy().view(np.uint8), g1.cpu().numpy().view(np.uint8), g2.cpu().numpy().view(np.uint8)]))
    return out


def _filtered(want, borders, L):
    out = []
    for e, w in enumerate(want):
        xy, z = pairs_ref.border_filter(w["raw_xy"], w["raw_z"], w["H"], w["W"], borders[e % L])
        out.append(dict(w, xy=xy, z=z))
    return out


def _batch(ctx, B, L, H, W, border, fmt=0, **kw):
    from mba_vo_amd import workloads
    return workloads.PairBatch(ctx, B, L=L, H=H, W=W, border=border, keyframe_format=fmt, cell=0, thresh=THR, every_candidate=True, **kw)


def _check_contents(got, want, kinds, L, H, W, borders):
    """The inputs exercise what they should."""
    for b, kind in enumerate(kinds):
        lv = got[b * L:(b + 1) * L]
        if kind == "const":
            assert all(len(g["z"]) == 0 for g in lv)  # K = 0 on every level; the entries are there all the same
        if kind == "ramp" and borders[0] == 0:
            assert len(lv[0]["z"]) == (H - 2) * (W - 2) and lv[0]["xy"][-1].tolist() == [W - 2.0, H - 2.0]  # the last slot written
        if kind in ("holes", "flat_holes"):
            w = want[b * L]
            mag = pairs_ref.gradient_magnitude(w["ref"].reshape(H, W))
            assert w["raw_K"] < int((mag > np.float32(THR)).sum())  # the depth test dropped candidates
        if kind in ("flat", "flat_holes"):
            flat = (lv[0]["xy"][:, 1] * W + lv[0]["xy"][:, 0]).astype(np.int64)
            segs = np.bincount(flat // 256, minlength=(H * W + 255) // 256)
            rows = np.bincount(lv[0]["xy"][:, 1].astype(np.int64), minlength=H)
            assert (rows[1:-1] == 0).any() and (H * W < 2048 or (segs == 0).any())  # rows / segments without a candidate


# (B, L, H, W, kinds): odd level sizes and rows that are no multiple of 64; 32 x 64 = 2 x 1024 pixels, an exact multiple of the
# workgroup's pixels (and of the segment's); 25 x 41 = 1024 + 1; 10 x 12 = 120, less than one segment
SHAPES = [(3, 3, 50, 70, ("flat_holes", "const", "ramp")), (4, 1, 32, 64, ("flat", "holes", "const", "ramp")),
          (4, 1, 25, 41, ("flat", "holes", "const", "ramp")), (4, 1, 10, 12, ("flat", "holes", "const", "ramp"))]


@pytest.mark.parametrize("B,L,H,W,kinds", SHAPES)
def test_every_array_matches_per_image_calls(mbavo, gpu_ctx, B, L, H, W, kinds):
    """Every array of every (pair, level), K included, with border 0 and max(4, 20 >> l) (2 on the 10 x 12 image) and in the three
    keyframe formats; the numpy restatement on every level."""
    sharp, depth, blur = _batch_inputs(kinds, H, W, seed=B + L + H)
    ts, td, tb = dv.dev(sharp, depth, blur)
    raw = _per_image(mbavo, gpu_ctx, ts, td, tb, L)
    on = [2] * L if H < 16 else cases.borders(L, True)
    for borders, fmt in (([0] * L, 0), (on, 0), (on, 1), (on, 2)):
        want = _filtered(raw, borders, L)
        pb = _batch(gpu_ctx, B, L, H, W, borders, fmt)
        try:
            counts = pb.prepare(ts, td, tb)
            got = dv.read_batch(pb, counts)
            dv.assert_same(got, want, fmt, (B, L, H, W, borders, fmt))
            assert [len(g["z"]) for g in got] == counts.ravel().tolist() == [len(w["z"]) for w in want]
            assert all(pb.array[e].d_kp_xy and pb.array[e].d_kp_z for e in range(B * L))
            _check_contents(got, want, kinds, L, H, W, borders)
            if fmt == 0:
                if borders[0]:
                    assert sum(len(w["z"]) for w in want) < sum(w["raw_K"] for w in want)  # the border test dropped candidates
                for e in range(B * L):
                    b, l = divmod(e, L)
                    rxy, rz = dref.keypoints(got[e]["ref"].reshape(H >> l, W >> l), l, THR, depth[b], borders[l])
                    assert np.array_equal(got[e]["xy"], rxy) and np.array_equal(got[e]["z"], rz), e
        finally:
            pb.close()


_LARGE = {}


def _large():
    """B = 2, L = 4, 480 x 640: 1200 segments on level 0, a scan of five 256-steps.  Border 0 on level 0 (the ramp pair's K is the
    largest there is), max(4, 20 >> l) below."""
    if not _LARGE:
        B, L, H, W = 2, 4, 480, 640
        sharp, depth, blur = _batch_inputs(("flat_holes", "ramp"), H, W, seed=11)
        _LARGE.update(B=B, L=L, H=H, W=W, sharp=sharp, depth=depth, blur=blur, borders=[0] + cases.borders(L, True)[1:])
    return _LARGE


def test_large_level_matches_per_image_calls(mbavo, gpu_ctx):
    c = _large()
    B, L, H, W = c["B"], c["L"], c["H"], c["W"]
    ts, td, tb = dv.dev(c["sharp"], c["depth"], c["blur"])
    want = _filtered(_per_image(mbavo, gpu_ctx, ts, td, tb, L), c["borders"], L)
    pb = _batch(gpu_ctx, B, L, H, W, c["borders"], 2)
    try:
        counts = pb.prepare(ts, td, tb)
        got = dv.read_batch(pb, counts)
        dv.assert_same(got, want, 2, "large")
        _check_contents(got, want, ("flat_holes", "ramp"), L, H, W, c["borders"])
        assert counts[1, 0] == (H - 2) * (W - 2) and counts[0, 0] > 256 * 256  # more keypoints than one scan step has pixels
        for e in range(B * L):
            b, l = divmod(e, L)
            rxy, rz = dref.keypoints(got[e]["ref"].reshape(H >> l, W >> l), l, THR, c["depth"][b], c["borders"][l])
            assert np.array_equal(got[e]["xy"], rxy) and np.array_equal(got[e]["z"], rz), e
    finally:
        pb.close()


def test_same_bits_for_any_B(mbavo, gpu_ctx):
    """Pair 0 of a B = 1 batch equals pair 0 of a B = 5 batch."""
    L, H, W = 3, 50, 70
    sharp, depth, blur = _batch_inputs(("flat_holes", "holes", "ramp", "flat", "const"), H, W, seed=5)
    borders = cases.borders(L, True)
    got = {}
    for B in (1, 5):
        pb = _batch(gpu_ctx, B, L, H, W, borders, 1)
        try:
            counts = pb.prepare(*dv.dev(sharp[:B], depth[:B], blur[:B]))
            got[B] = (dv.read_batch(pb, counts)[:L], counts[0].tolist())
        finally:
            pb.close()
    assert got[1][1] == got[5][1] and min(got[1][1]) > 0
    for a, b in zip(got[1][0], got[5][0]):
        assert all(np.array_equal(a[key], b[key]) for key in ("ref", "cur", "grad", "xy", "z"))


SENTINEL = -7.0


@pytest.mark.parametrize("n_key", [0, 1, 4])
def test_update_equals_prepare(mbavo, gpu_ctx, n_key):
    """B = 4, L = 3, 50 x 70.  After an update every array and K equal a fresh prepare of the composite inputs; the keyframe side
    of a pair not listed is not written: its keypoint and gradient arrays were filled with a sentinel before the update and hold
    it afterwards, over their whole capacity."""
    B, L, H, W = 4, 3, 50, 70
    sharp, depth, blur = _batch_inputs(("flat_holes", "holes", "flat", "ramp"), H, W, seed=31)
    s2, d2, b2 = _batch_inputs(("holes", "ramp", "flat_holes", "const"), H, W, seed=77)
    keys = {0: [], 1: [2], 4: [0, 1, 2, 3]}[n_key]
    borders = cases.borders(L, True)
    used, fresh = _batch(gpu_ctx, B, L, H, W, borders, 0), _batch(gpu_ctx, B, L, H, W, borders, 0)
    try:
        before = used.prepare(*dv.dev(sharp, depth, blur))
        caps = dref.capacities(H, W, L)
        for b in range(B):
            if b in keys:
                continue
            for l in range(L):
                q = used.array[b * L + l]
                dv.poke(q.d_kp_xy, np.full(2 * caps[l], SENTINEL))
                dv.poke(q.d_kp_z, np.full(caps[l], SENTINEL))
                dv.poke(q.d_ref_dIxy, np.full(caps[l] * 8, 0xA5, np.uint8))
        for j in keys:
            sharp[j], depth[j] = s2[j], d2[j]
        args = [dv.dev(b2)[0], keys]
        if keys:
            args += dv.dev(np.ascontiguousarray(s2[keys]), np.ascontiguousarray(d2[keys]))
        counts = used.update(*args)
        want = fresh.prepare(*dv.dev(sharp, depth, b2))
        assert np.array_equal(counts, want)
        assert n_key == 0 or not np.array_equal(counts, before)
        for e, (a, w) in enumerate(zip(dv.read_batch(used, counts), dv.read_batch(fresh, want))):
            b, l = divmod(e, L)
            assert np.array_equal(a["ref"], w["ref"]) and np.array_equal(a["cur"], w["cur"]), e
            q = used.array[e]
            if b in keys:
                assert all(np.array_equal(a[key], w[key]) for key in ("grad", "xy", "z")), e
            else:
                assert np.all(dv.peek(q.d_kp_xy, 2 * caps[l], np.float64) == SENTINEL) and np.all(dv.peek(q.d_kp_z, caps[l], np.float64) == SENTINEL), e
                assert np.all(a["grad"] == 0xA5), e
    finally:
        used.close()
        fresh.close()


def test_launches_and_synchronisations_do_not_depend_on_B(mbavo, gpu_ctx):
    """Prepare: at most ceil((L-1)/3) + 4 launches; update: at most ceil((L-1)/3) + 5, no keyframe launch with n_key = 0.  Either
    call: one synchronisation and the B x L counts device-to-host, the same for B = 2 and B = 64 and for n_key = 1 and B."""
    for L, H, W in ((1, 120, 160), (4, 120, 160), (5, 128, 160)):
        pyr = math.ceil((L - 1) / 3)
        seen_p, seen_u = [], []
        for B in (2, 64):
            sharp, depth, blur = _batch_inputs(("flat_holes", "holes"), H, W, seed=L)
            sharp, depth, blur = (np.ascontiguousarray(np.tile(a, (B // 2, 1, 1))) for a in (sharp, depth, blur))
            pb = _batch(gpu_ctx, B, L, H, W, 4)
            try:
                assert pb.stats()[:3] == (0, 0, 0)
                ts, td, tb = dv.dev(sharp, depth, blur)
                counts = pb.prepare(ts, td, tb)
                launches, syncs, d2h, held = pb.stats()
                assert syncs == 1 and launches <= pyr + 4 and d2h == 4 * B * L
                nbytes, cells = C.c_longlong(0), (C.c_int * 8)()
                assert gpu_ctx.lib.mbavo_pairs_plan(C.byref(pb.opts), C.byref(nbytes), cells) == 0 and held == nbytes.value
                assert list(cells[:L]) == dref.capacities(H, W, L) and counts[:, 0].min() > 0
                seen_p.append(launches)
                for keys in ([B - 1], list(range(B))):
                    pb.update(tb, keys, ts[keys].contiguous(), td[keys].contiguous())
                    upd, _ = pb.step_stats()
                    assert upd[0] <= pyr + 5 and upd[1] == 1 and upd[2] == 4 * B * L, (L, B, upd)
                    seen_u.append(upd)
                pb.update(tb)
                none = pb.step_stats()[0]
                assert none[0] == pyr and none[1] == 1  # the pyramids of the new current frames alone
            finally:
                pb.close()
        assert len(set(seen_p)) == 1 and len({u[:2] for u in seen_u}) == 1, (L, seen_p, seen_u)


def test_lm_on_the_librarys_array_matches_hand_assembled(mbavo, gpu_ctx):
    """B = 3, L = 2, 48 x 64, one-pixel patches, k = 2, S = 4: mbavo_lm_batch_levels on mbavo_pairs_problems and on an array whose
    images, gradients and keypoints come from the per-image calls: identical results, trace records and knots."""
    capi = mbavo.capi
    B, L, H, W, k, N = 3, 2, 48, 64, 2, 2
    sharp, depth, _ = _batch_inputs(("flat", "holes", "flat_holes"), H, W, seed=9)
    blur = np.ascontiguousarray(np.roll(sharp, (1, 1), (1, 2)))
    ts, td, tb = dv.dev(sharp, depth, blur)
    borders = [4, 4]
    want = _filtered(_per_image(mbavo, gpu_ctx, ts, td, tb, L), borders, L)
    pb = _batch(gpu_ctx, B, L, H, W, borders, 0, S=4, k=k, N=N, pattern=np.array([[0, 0]], np.int32))
    try:
        import torch
        counts = pb.prepare(ts, td, tb)
        twin = (capi.Problem * (B * L))()
        C.memmove(twin, pb.array, C.sizeof(twin))
        keep = []
        for e, w in enumerate(want):
            ref, cur, g0 = w["dev"][:3]
            xy, z = dv.dev(np.ascontiguousarray(w["xy"]).ravel(), np.ascontiguousarray(w["z"]))
            cur_ptr = torch.tensor([cur.data_ptr()], dtype=torch.int64, device="cuda:0")
            keep += [xy, z, cur_ptr]
            q = twin[e]
            assert q.P == 1 and q.S == 4 and q.K == counts.ravel()[e] == len(w["z"]) and q.K > 100
            q.d_ref_img, q.d_ref_dIxy, q.d_cur_imgs = ref.data_ptr(), g0.data_ptr(), cur_ptr.data_ptr()
            q.d_kp_xy, q.d_kp_z, q.K = xy.data_ptr(), z.data_ptr(), len(w["z"])
            assert q.d_kp_xy != pb.array[e].d_kp_xy and q.d_ref_img != pb.array[e].d_ref_img
        rng = np.random.default_rng(2)
        kt0 = rng.normal(0, 2e-3, (B, N, 3))
        kR0 = np.tile(np.array([0.0, 0, 0, 1]), (B, N, 1)) + rng.normal(0, 1e-3, (B, N, 4))
        kR0 /= np.linalg.norm(kR0, axis=2, keepdims=True)
        motion = (np.full(B, 0.3), np.full(B, 0.04), np.zeros(B), 0.5, kt0, kR0)
        assert pb.set_motion(*motion) == 0
        for e in range(B * L):  # (t0, dt and the start index were set after the copy)
            twin[e].t0, twin[e].dt = pb.array[e].t0, pb.array[e].dt
        want_f, want_r, kinds = dv.run_lm(gpu_ctx, capi, B, L, twin, k)
        want_kt, want_kR = pb.knots()
        assert 1 in kinds and np.abs(want_kt - kt0).max() > 1e-9  # accepted steps: the comparison is not vacuous
        assert pb.set_motion(*motion) == 0
        got_f, got_r, _ = dv.run_lm(gpu_ctx, capi, B, L, pb.array, k)
        assert got_f == want_f and got_r == want_r
        kt, kR = pb.knots()
        assert np.array_equal(kt, want_kt) and np.array_equal(kR, want_kR)
    finally:
        pb.close()


def test_assess_and_track_frame_at_large_K(orc, mbavo, gpu_ctx):
    """The 480 x 640 batch: mbavo_pairs_assess against the oracle's orc_is_keyframe (tests/pairs_step.py) on the level-0 keypoints
    the device holds, within that file's bound, num_keypoints0 = level-0 K; then one mbavo_pairs_track_frame with a new keyframe
    for one pair: 0, and status 0 for every pair."""
    capi = mbavo.capi
    c = _large()
    B, L, H, W, k, N = c["B"], c["L"], c["H"], c["W"], 2, 2
    ts, td, tb = dv.dev(c["sharp"], c["depth"], c["blur"])
    pb = _batch(gpu_ctx, B, L, H, W, c["borders"], 2, S=2, k=k, N=N, pattern=np.array([[0, 0]], np.int32))
    try:
        counts = pb.prepare(ts, td, tb)
        assert counts[1, 0] == (H - 2) * (W - 2)
        kt, kR = np.zeros((B, N, 3)), np.zeros((B, N, 4))
        for b in range(B):
            kt[b], kR[b] = synth.trajectory("harness", N, 0.012 * (0.6 + b), 0.02 * (0.6 + b))
        cap, exp = np.array([0.3, 0.21]), np.array([0.04, 0.3])
        assert pb.set_motion(cap, exp, np.zeros(B), 0.5, kt, kR) == 0
        out = pb.assess(ps.FLOW0, ps.FLOW1, ps.KERNEL)
        assert pb.step_stats()[1][:2] == (1, 1)
        for b in range(B):
            q = pb.array[b * L]
            xy, z = dv.peek(q.d_kp_xy, 2 * q.K, np.float64).reshape(-1, 2), dv.peek(q.d_kp_z, q.K, np.float64)
            v, af, ak = ps.oracle_assess(orc, pb.intr, xy, z, k, 0.0, 0.5, kt[b], kR[b], cap[b], exp[b])
            a = out[b]
            print("assess pair %d: K %d flow %.9g / %.9g kernel %.9g / %.9g verdict %d / %d" % (b, q.K, a.avg_flow, af, a.avg_kernel, ak, a.is_keyframe, v))
            assert a.status == 0 and a.num_keypoints0 == counts[b, 0] == len(z) and af > 0 and ak > 0
            assert abs(a.avg_flow - af) <= ps.bound(af), (b, a.avg_flow, af)
            assert abs(a.avg_kernel - ak) <= ps.bound(ak), (b, a.avg_kernel, ak)
            if ps.margin_ok(af, ak):
                assert a.is_keyframe == v, b
        # one frame of both trackers, a new keyframe for pair 1
        assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0
        o = capi.LmBatchOpts()
        o.spline_deg_k, o.max_num_iterations, o.max_consecutive_nonmonotonic_steps = k, 3, 5
        o.solver_type, o.sync_every = 0, 0
        o.min_step_quality, o.min_abs_cost_decrease, o.max_chi_square_error = 0.5, 1e-3, 3.0
        new_sharp, new_depth = dv.dev(np.ascontiguousarray(c["sharp"][:1]), np.ascontiguousarray(c["depth"][:1]))
        new_blur = dv.dev(np.ascontiguousarray(np.roll(c["sharp"][[0, 0]], (1, 1), (1, 2))))[0]
        frames, counts2, res, _ = pb.track_frame(new_blur, np.full(B, 0.1), np.full(B, 0.02), o, (ps.FLOW0, ps.FLOW1, ps.KERNEL), [1], new_sharp, new_depth)
        assert counts2[0].tolist() == counts[0].tolist() == counts2[1].tolist()  # pair 1 now holds pair 0's keyframe
        for b in range(B):
            assert frames[b].a.status == 0 and frames[b].a.num_keypoints0 == counts2[b, 0], b
            assert np.isfinite(np.array(frames[b].T_world)).all()
    finally:
        pb.close()
