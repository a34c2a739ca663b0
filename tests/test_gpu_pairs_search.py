"""mbavo_pairs_search_depths on the device, through the C ABI.  Nothing here has a tolerance: the cost volume is held bit for bit to
mbavo_pairs_refine_depths(apply = 0) with each candidate's depths written into the object, the selection bit for bit to the numpy
selection (tests/pairs_search_ref.py) applied to the device's own volume, the records bit for bit to the lane_sum restatement.

Shapes: B = 3 pairs of 48 x 64 textures at L = 3, grid cells of 8, border 1; k = 2 and 4, the three keyframe formats, P = 8 and 1,
level = -1 and single levels, absolute and relative ranges; an every-candidate object at L = 2 with 300 points per pair (P = 8: tiles of
128 keypoints, K no multiple of it, several workgroups per level); a level with K = 0; ND = 2, 5, 16 and 64.  The recovery setting
is the one tests/test_pairs_search_api.py establishes on the restatement, asserted here without its factor (the figures of an
MI355X are in profiles/r32_pairs_search.txt)."""
import ctypes as C

import numpy as np
import pytest

import pairs_depth_support as ds
import pairs_device as dv
import pairs_filter_scene as fs
import pairs_refine_scene as sc
import pairs_search_ref as sref
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -2
B, L, H, W, CELL, THR = 3, 3, 48, 64, 8, 4.0
PAT1 = np.array([[0, 0]], np.int32)
# (k, N, segment the samples lie on, S, pattern, keyframe_format), then level, relative, rho_lo, rho_hi of the volume test
CASES = [((2, 2, 0, 3, None, 0), -1, 0, 0.3, 1.1), ((4, 4, 0, 3, PAT1, 1), 1, 1, 0.6, 1.5), ((4, 6, 1, 8, None, 2), -1, 1, 0.6, 1.5),
         ((4, 4, 0, 8, PAT1, 0), 0, 0, 0.3, 1.1)]
REC = 32
# the recovery setting of tests/test_pairs_search_api.py
START_Z, ND_REC, RHO_LO, RHO_HI, MIN_RATIO, MIN_SHARE = 0.4, 16, 0.25, 1.0, 1.05, 0.9
_IMAGES = {}


def _images():
    if not _IMAGES:
        rng = np.random.default_rng(30)
        sharp = np.stack([synth.texture_image(H, W, seed=60 + 3 * b, octaves=(16, 8, 4)) for b in range(B)])
        blur = np.stack([np.clip(np.roll(sharp[b], (1, -1), (0, 1)).astype(np.int32) + rng.integers(-4, 5, (H, W)), 0, 255).astype(np.uint8) for b in range(B)])
        depth = rng.uniform(1.0, 3.0, (B, H, W)).astype(np.float32)
        _IMAGES.update(sharp=np.ascontiguousarray(sharp), blur=np.ascontiguousarray(blur), depth=depth)
    return _IMAGES


def _motion(k, N, start):
    rng = np.random.default_rng(11)
    kt, kR = np.zeros((B, N, 3)), np.zeros((B, N, 4))
    for b in range(B):
        kt[b], kR[b] = synth.trajectory("harness", N, 0.004 * (b + 1), 0.01 * (b + 1))
        kt[b] += rng.normal(0, 0.02, 3)
    cap = (start + 0.4 + 0.05 * np.arange(B)) * 0.5
    return dict(cap=cap, exp=np.full(B, 0.04), t0=np.zeros(B), dt=0.5, kt=kt, kR=kR)


def _object(ctx, case, pairs=B, dense=False, levels=L):
    from mba_vo_amd import workloads
    k, N, start, S, pattern, fmt = case
    return workloads.PairBatch(ctx, pairs, L=levels, H=H, W=W, S=S, k=k, N=N, cell=0 if dense else CELL, thresh=THR, border=1, every_candidate=dense,
                               pattern=pattern, keyframe_format=fmt)


def _prepared(ctx, case, sel=slice(None), dense=False, depth=None, points=None, levels=L):
    c, m = _images(), _motion(*case[:3])
    pb = _object(ctx, case, pairs=len(range(B)[sel]), dense=dense, levels=levels)
    d = c["depth"] if depth is None else depth
    sharp, blur = dv.dev(np.ascontiguousarray(c["sharp"][sel]), np.ascontiguousarray(c["blur"][sel]))
    counts = pb.prepare(sharp, dv.dev(np.ascontiguousarray(d[sel]))[0], blur) if points is None else pb.prepare_points(sharp, blur, points)
    assert pb.set_motion(m["cap"][sel], m["exp"][sel], m["t0"][sel], m["dt"], m["kt"][sel], m["kR"][sel]) == 0
    return pb, counts


def _points(n, seed=5):
    rng = np.random.default_rng(seed)
    return [(np.stack([rng.integers(6, W - 6, n), rng.integers(6, H - 6, n)], 1).astype(np.float64), rng.uniform(1.0, 3.0, n)) for _ in range(B)]


_depths, _layout, _search, _check_selection = ds.depths, ds.level_layout, ds.search_run, ds.search_check_selection


def _branches(res, nd):
    """How many keypoints of a checked call took each branch of steps 3 and 4 (the restatement's selection on the device's volume,
    which the device's arrays equal bit for bit)."""
    n = dict(keypoints=0, none_full=0, at_an_end=0, neighbour_not_full=0, den_not_positive=0, parabola=0, on_the_clamp=0, tie=0, no_runner_up=0)
    for sel, _, _ in res.values():
        best, par = sel["best"], sel["parabola"]
        inner = (best > 0) & (best < nd - 1)
        n["keypoints"] += best.size
        n["none_full"] += int((best < 0).sum())
        n["at_an_end"] += int(((best >= 0) & ~inner).sum())
        n["parabola"] += int(par.sum())
        n["no_runner_up"] += int(((best >= 0) & np.isnan(sel["cost_second"])).sum())
        for i in np.flatnonzero(inner):
            c = sel["volume"][i]
            if np.isnan(c[best[i] - 1]) or np.isnan(c[best[i] + 1]):
                n["neighbour_not_full"] += 1
            elif not par[i]:
                n["den_not_positive"] += 1
            elif abs(sel["rho"][i] - sel["rho_best"][i]) == 0.5 * sel["step"][i]:
                n["on_the_clamp"] += 1
        n["tie"] += int(sum((sel["volume"][i] == sel["cost_best"][i]).sum() > 1 for i in np.flatnonzero(best >= 0)))
    return n


@pytest.mark.parametrize("case", range(len(CASES)))
def test_volume_is_the_refinement_at_every_candidate(mbavo, gpu_ctx, case):
    import torch
    obj, level, relative, lo, hi = CASES[case]
    nd = 5
    pb, counts = _prepared(gpu_ctx, obj)
    try:
        assert (counts > 0).all()
        z0 = _depths(pb)
        out, arr = _search(pb, nd, lo, hi, level=level, relative=relative, min_ratio=1.02)
        assert pb.search_stats() == (1, 1, len(out) * REC)
        _check_selection(pb, out, arr, nd, lo, hi, level=level, relative=relative, z=z0, tag="case %d" % case, min_ratio=1.02)
        n, off, levels = _layout(pb, level)
        cost = torch.zeros((B, n), dtype=torch.float64, device="cuda:0")
        valid = torch.zeros((B, n), dtype=torch.int32, device="cuda:0")
        n_full = 0
        for d in range(nd):
            for e in range(B * L):
                dv.poke(pb.array[e].d_kp_z, np.ascontiguousarray(sref.candidates(z0[e], nd, lo, hi, relative)[3][:, d]))
            assert pb.refine_depths(level=level, apply=False, cost=cost, valid=valid)[0] == 0
            c, v = cost.cpu().numpy(), valid.cpu().numpy()
            for b in range(B):
                for l in levels:
                    K, P = pb.array[b * L + l].K, pb.array[b * L + l].P
                    full = v[b, off[l]:off[l] + K] == P
                    got = arr["volume"][b, off[l]:off[l] + K, d]
                    assert np.array_equal(np.isnan(got), ~full), (case, d, b, l)
                    assert dv.same_bits(got[full], c[b, off[l]:off[l] + K][full]), (case, d, b, l)
                    n_full += int(full.sum())
        assert n_full > 0
        for e in range(B * L):
            dv.poke(pb.array[e].d_kp_z, z0[e])
        again, arr2 = _search(pb, nd, lo, hi, level=level, relative=relative, min_ratio=1.02)  # the depths are back: the same bytes
        assert bytes(again) == bytes(out) and all(a.tobytes() == arr2[key].tobytes() for key, a in arr.items())
    finally:
        pb.close()


def test_grid_shapes_determinism_and_batching(mbavo, gpu_ctx):
    obj = CASES[0][0]
    lo, hi = 0.3, 1.1
    # 300 points per pair on an every-candidate object: P = 8, tiles of 128, K no multiple of it, G >= 2 (L = 2: a list may not
    # be longer than the smallest level's capacity, and level 2 has 16 x 12 pixels)
    pb, counts = _prepared(gpu_ctx, obj, dense=True, points=_points(300), levels=2)
    try:
        assert (counts[:, 0] == 300).all() and pb.capacities()[0] > 128
        z0 = _depths(pb)
        seen = {}
        for nd in (2, 16, 64):
            ratio = 0.0 if nd == 2 else 1.05  # (two candidates have no runner-up)
            out, arr = _search(pb, nd, lo, hi, min_ratio=ratio)
            res = _check_selection(pb, out, arr, nd, lo, hi, z=z0, tag="dense ND %d" % nd, min_ratio=ratio)
            assert sum(int(a.sum()) for _, a, _ in res.values()) > 0
            taken = _branches(res, nd)
            print("dense ND %d: %s" % (nd, taken))
            seen[nd] = taken
            out2, arr2 = _search(pb, nd, lo, hi, min_ratio=ratio)
            assert bytes(out) == bytes(out2) and all(a.tobytes() == arr2[key].tobytes() for key, a in arr.items())
        # the branches of steps 3 and 4 that these volumes exercise (measured, of 1800 keypoints at ND 16 / 64: no full candidate 2 /
        # 2, best at an end 1394 / 1371, a neighbour not full 6 / 5, a parabola 398 / 422, no runner-up 5 / 2).  Image data cannot
        # reach the others: with c_0 the lowest cost and ties going to the lower index, c_- > c_0 and den > 0 short of an overflow,
        # delta passes 0.5 only by a rounding at costs 2^54 apart, and two sums of doubles do not tie.  Those are held on
        # hand-made volumes in tests/test_pairs_search_api.py; the device agrees with that selection bit for bit above.
        for nd in (16, 64):
            assert all(seen[nd][key] > 0 for key in ("none_full", "at_an_end", "neighbour_not_full", "parabola", "no_runner_up")), seen[nd]
        first = (bytes(out), arr)
        for b in range(B):  # pair b alone in a B = 1 object
            one, _ = _prepared(gpu_ctx, obj, sel=slice(b, b + 1), dense=True, points=_points(300)[b:b + 1], levels=2)
            try:
                o1, a1 = _search(one, 64, lo, hi, min_ratio=1.05)
                assert bytes(o1) == first[0][b * 2 * REC:(b + 1) * 2 * REC]
                assert all(a1[key][0].tobytes() == first[1][key][b].tobytes() for key in a1)
            finally:
                one.close()
    finally:
        pb.close()
    # no depth anywhere: K = 0 on every level
    pb, counts = _prepared(gpu_ctx, obj, depth=np.zeros((B, H, W), np.float32))
    try:
        assert (counts == 0).all()
        out, arr = _search(pb, 5, lo, hi)
        assert all((r.status, r.num_keypoints, r.num_searched, r.num_accepted, r.cost, r.sum_ratio) == (0, 0, 0, 0, 0.0, 0.0) for r in out)
        assert all((a == -7).all() for a in arr.values())
    finally:
        pb.close()


def _snapshot(pb, k):
    st = pb.filter_state()
    n = pb.B * sum(pb.capacities())
    state = [dv.peek(st["ptr"][i], n, dt).tobytes() for i, dt in enumerate((np.float64, np.float64, np.int32, np.int32))]
    xy = [dv.peek(pb.array[e].d_kp_xy, 2 * pb.array[e].K, np.float64).tobytes() for e in range(pb.B * pb.L)]
    return state, xy, [z.tobytes() for z in _depths(pb)], [pb.array[e].K for e in range(pb.B * pb.L)], [a.tobytes() for a in pb.knots()]


def test_apply_writes_exactly_the_accepted_depths(mbavo, gpu_ctx):
    obj = CASES[0][0]
    k = obj[0]
    lo, hi, nd = 0.3, 1.1, 16
    pb, counts = _prepared(gpu_ctx, obj)
    try:
        assert pb.filter_depths(prior_rel_sigma=0.1)[0] == 0  # (the filter has a state to leave alone)
        before = _snapshot(pb, k)
        z0 = _depths(pb)
        out, arr = _search(pb, nd, lo, hi, min_ratio=1.05)
        assert _snapshot(pb, k) == before  # apply = 0: no byte of the object changes
        res = _check_selection(pb, out, arr, nd, lo, hi, z=z0, tag="apply 0", min_ratio=1.05)
        out1, arr1 = _search(pb, nd, lo, hi, min_ratio=1.05, apply=True)
        assert bytes(out1) == bytes(out) and all(a.tobytes() == arr1[key].tobytes() for key, a in arr.items())
        after = _snapshot(pb, k)
        assert (after[0], after[1], after[3], after[4]) == (before[0], before[1], before[3], before[4])
        z1 = _depths(pb)
        moved = 0
        for (b, l), (sel, acc, z_new) in res.items():
            e = b * L + l
            assert dv.same_bits(z1[e][~acc], z0[e][~acc]) and dv.same_bits(z1[e][acc], (1.0 / sel["rho"])[acc]), (b, l)
            moved += int(acc.sum())
        assert moved > 0 and sum(r.num_accepted for r in out) == moved
        # the calls that follow run and read the new depths
        rc, fil = pb.filter_depths(reset=1, prior_rel_sigma=0.1)
        assert rc == 0 and all(r.seeded == 1 and r.status == 0 for r in fil)
        st = pb.filter_state()
        mu = st["mu"].cpu().numpy()
        for (b, l), (sel, acc, z_new) in res.items():
            fresh = st["n_obs"].cpu().numpy()[b, st["offset"][l]:st["offset"][l] + counts[b, l]] == 0
            got = mu[b, st["offset"][l]:st["offset"][l] + counts[b, l]]
            assert dv.same_bits(got[fresh], (1.0 / z1[b * L + l])[fresh])  # (seeded from the searched depths)
        twin, _ = _prepared(gpu_ctx, obj)
        try:
            for e in range(B * L):
                dv.poke(twin.array[e].d_kp_z, z1[e])
            assert dv.run_lm(gpu_ctx, mbavo.capi, B, L, pb.array, k)[:2] == dv.run_lm(gpu_ctx, mbavo.capi, B, L, twin.array, k)[:2]
        finally:
            twin.close()
    finally:
        pb.close()


def _off_knots_states(mbavo, case):
    m = _motion(*case[:3])
    states = (mbavo.capi.VoState * B)()
    for b, st in enumerate(states):  # the same knots and times through the state; pair 1's knots start long after its frame
        st.t0, st.dt, st.N, st.is_first = (100.0 if b == 1 else float(m["t0"][b])), m["dt"], case[1], 0
        st.knots_t[:3 * case[1]] = list(m["kt"][b].ravel())
        st.knots_R[:4 * case[1]] = list(m["kR"][b].ravel())
        st.T_keyframe[6] = st.T_prev_b2w[6] = 1.0
    return states


def test_pair_off_its_knots(mbavo, gpu_ctx):
    obj = CASES[0][0]
    good, counts = _prepared(gpu_ctx, obj)
    pb, _ = _prepared(gpu_ctx, obj)
    try:
        out_good, arr_good = _search(good, 5, 0.3, 1.1, apply=True)
        z0 = _depths(pb)
        assert pb.set_states(_off_knots_states(mbavo, obj)) == 0
        out, arr = _search(pb, 5, 0.3, 1.1, apply=True)
        z1, zg = _depths(pb), _depths(good)
        for l in range(L):
            r = out[1 * L + l]
            assert (r.status, r.num_keypoints, r.num_searched, r.num_accepted) == (E_RANGE, counts[1, l], 0, 0) and np.isnan(r.cost) and np.isnan(r.sum_ratio)
            assert dv.same_bits(z1[1 * L + l], z0[1 * L + l])
        assert all((a[1] == -7).all() for a in arr.values())  # nothing written for it
        for b in (0, 2):
            assert all(a[b].tobytes() == arr_good[key][b].tobytes() for key, a in arr.items())
            for l in range(L):
                assert bytes(out[b * L + l]) == bytes(out_good[b * L + l]) and dv.same_bits(z1[b * L + l], zg[b * L + l])
    finally:
        good.close(); pb.close()


def test_rejected_calls_launch_nothing(mbavo, gpu_ctx):
    capi, lib = mbavo.capi, gpu_ctx.lib
    obj = CASES[0][0]
    fresh = _object(gpu_ctx, obj)
    try:
        out = (capi.PairsSearch * (B * L))()
        ok = sref.opts_struct(capi)
        assert sref.call(lib, fresh.handle, ok, out) == E_ARG  # before the first prepare
        c = _images()
        fresh.prepare(*dv.dev(c["sharp"], c["depth"], c["blur"]))
        assert sref.call(lib, fresh.handle, ok, out) == E_ARG and fresh.search_stats() == (0, 0, 0)  # before the first motion
    finally:
        fresh.close()
    pb, counts = _prepared(gpu_ctx, obj)
    try:
        assert pb.filter_depths(prior_rel_sigma=0.1)[0] == 0
        assert pb.search_depths(8, 0.3, 1.1, level=0)[0] == 0 and pb.search_stats() == (1, 1, B * REC)
        before = _snapshot(pb, obj[0])
        out = (capi.PairsSearch * (B * L))()
        nan, inf = float("nan"), float("inf")
        mk = lambda **kw: sref.opts_struct(capi, **kw)
        bad = [None, mk(level=-2), mk(level=L), mk(apply=2), mk(apply=-1), mk(num_candidates=1), mk(num_candidates=65), mk(num_candidates=0),
               mk(relative=2), mk(relative=-1), mk(rho_lo=0.0), mk(rho_lo=-0.1), mk(rho_lo=1.0, rho_hi=1.0), mk(rho_lo=1.0, rho_hi=0.5),
               mk(rho_lo=nan), mk(rho_hi=inf), mk(rho_hi=nan), mk(min_ratio=0.5), mk(min_ratio=-1.0), mk(min_ratio=nan), mk(min_ratio=inf),
               mk(min_curv=-1.0), mk(min_curv=nan), mk(min_curv=inf), mk(z_min=-1.0), mk(z_min=nan), mk(z_max=nan), mk(z_max=inf),
               mk(z_min=2.0, z_max=1.0), mk(z_max=0.005)]
        for o in bad:
            assert sref.call(lib, pb.handle, o, out) == E_ARG and pb.search_stats() == (0, 0, 0), None if o is None else bytes(o)
        assert _snapshot(pb, obj[0]) == before
        assert pb.search_depths(8, 0.3, 1.1, want_records=False) == (0, None) and pb.search_stats() == (1, 0, 0)  # nothing is waited for
        assert pb.search_depths(64, 0.3, 1.1, min_ratio=1.0)[0] == 0 and pb.search_stats() == (1, 1, B * L * REC)
    finally:
        pb.close()


def test_the_search_recovers_what_the_filter_alone_cannot(mbavo, gpu_ctx):
    """The setting of tests/test_pairs_search_api.py on the device, without its factor: every level-0 keypoint starts at START_Z;
    one object runs T filter calls, its twin a search on the widest-baseline frame first and then the same T filter calls, the
    first with reset = 1.  Asserted: the share accepted, and the twin's median relative depth error over the accepted keypoints is
    below the filter's alone and below T refinement steps' on the widest-baseline frame."""
    from mba_vo_amd import workloads
    c, m = sc.scene(), sc.motion()
    objs = []
    try:
        frames = np.stack([fs.frames(b) for b in range(B)], 1)  # T x B x H x W
        caps = np.stack([fs.caps(b) for b in range(B)], 1)      # T x B
        last = fs.T - 1
        for _ in range(3):
            pb = workloads.PairBatch(gpu_ctx, B, L=L, H=H, W=W, S=sc.S, k=sc.K_DEG, N=sc.N, cell=CELL, thresh=THR, border=4, huber=sc.HUBER)
            counts = pb.prepare(*dv.dev(np.ascontiguousarray(c["sharp"]), np.ascontiguousarray(c["depth"]), np.ascontiguousarray(frames[last])))
            assert pb.set_motion(caps[last], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
            objs.append(pb)
        refined, alone, both = objs
        z_of = lambda p: [dv.peek(p.array[b * L].d_kp_z, counts[b, 0], np.float64) for b in range(B)]
        truth = z_of(both)
        for p in objs:
            for b in range(B):
                dv.poke(p.array[b * L].d_kp_z, np.full(counts[b, 0], START_Z))
        for _ in range(fs.T):
            assert refined.refine_depths(level=0, apply=True)[0] == 0
        rc, out = both.search_depths(ND_REC, RHO_LO, RHO_HI, level=0, apply=True, min_ratio=MIN_RATIO)
        assert rc == 0
        z_s = z_of(both)
        acc = [z_s[b] != START_Z for b in range(B)]
        assert [int(a.sum()) for a in acc] == [r.num_accepted for r in out]
        for p in (alone, both):
            for t in range(fs.T):
                p.update(dv.dev(np.ascontiguousarray(frames[t]))[0])
                assert p.set_motion(caps[t], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
                rc, fil = p.filter_depths(level=0, apply=True, reset=int(t == 0), **fs.OPTS)
                assert rc == 0 and [r.seeded for r in fil] == [int(t == 0)] * B
        z_r, z_a, z_b = z_of(refined), z_of(alone), z_of(both)
        for b in range(B):
            sel = acc[b]
            err = lambda z: float(np.median(np.abs(z[sel] / truth[b][sel] - 1.0)))
            print("pair %d: %d of %d accepted; median relative error: start %.4f, %d refinements %.4f, %d filter calls %.4f, search %.4f, search + "
                  "filter %.4f" % (b, sel.sum(), sel.size, abs(START_Z / 2.0 - 1), fs.T, err(z_r[b]), fs.T, err(z_a[b]), err(z_s[b]), err(z_b[b])))
            assert sel.sum() >= MIN_SHARE * sel.size
            assert err(z_b[b]) < err(z_a[b]) and err(z_b[b]) < err(z_r[b])
    finally:
        for p in objs:
            p.close()
