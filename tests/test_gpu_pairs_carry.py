"""mbavo_pairs_carry_save / mbavo_pairs_carry_adopt on the device, through the C ABI, held to the numpy restatement
(tests/pairs_carry_ref.py: brute force, no index) on the object's own device arrays.  Records, flags, counts, d_rho, d_info, the
depths after apply = 1 and the filter's arrays after seed_filter = 1 are held bit for bit -- the order of every sum is specified.

Every object is built with prepare_points / update_points, so positions and depths are the test's own: every-candidate objects of
64 x 48, border 0, B = 3, L = 2.  With these intrinsics (32, 32, 32, 24) the ray and the projection of a whole pixel are exact, so a
translation of -1/32 along x moves a point of depth 2 by exactly half a pixel at level 0."""

import numpy as np
import pytest

import pairs_cases
import pairs_carry_ref as cref
import pairs_depth_support as ds
import pairs_device as dv
import pairs_smooth_ref as mref

pytestmark = pytest.mark.gpu

E_ARG = -1
H, W, B, L = 48, 64, 3, 2
K_DEG, N, S = 4, 4, 3
KS = [0, 1, 63, 64, 65, 257, 600]
HALF = np.array([-1.0 / 32, 0, 0, 0, 0, 0, 1.0])  # +0.5 px along x at depth 2, level 0
_Q = np.array([0.01, -0.02, 0.015, 1.0])
TILT = np.concatenate([[0.05, -0.03, 0.3], _Q / np.linalg.norm(_Q)])
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
SAVE = dict(radius=2, deflate=0.8)
ADOPT = dict(min_support=2, max_rel_diff=0.1)


def _object(ctx, nb=B, levels=L):
    from mba_vo_amd import workloads
    return workloads.PairBatch(ctx, nb, L=levels, H=H, W=W, S=S, k=K_DEG, N=N, cell=0, thresh=4.0, border=0, every_candidate=True)


@pytest.fixture(scope="module")
def images():
    sharp, _, blur = pairs_cases.inputs(B, H, W, seed=4, special=False)
    return dv.dev(sharp, blur)


def _points(rng, n):
    """n level-0 points inside x <= 61, y <= 45 (they stay inside level 1), on two surfaces, some sharing a pixel."""
    xy = np.stack([rng.integers(0, 62, n), rng.integers(0, 46, n)], 1).astype(np.float64)
    if n >= 8:
        xy[n // 2:n // 2 + 3] = xy[:3]  # shared pixels
    z = np.where(rng.uniform(size=n) < 0.5, 2.0, 3.0) * (1.0 + rng.uniform(-0.03, 0.03, n))
    return xy, z


def _special(xy, z):
    """The required cases, written over the first entries of a list of >= 8 points at depth 2 under HALF: (62, 47) lands exactly
    on the last row and column; (63, 20) has u + 0.5 = W exactly and is dropped; 4 and 5 land on one pixel."""
    xy[:6] = [[62, 47], [63, 20], [0, 0], [61, 47], [30, 30], [30, 30]]
    z[:6] = 2.0
    return xy, z


_entry, _bits, _same, _save, _arrays, _adopt = ds.carry_entry, ds.bits, ds.same, ds.carry_save_check, ds.carry_arrays, ds.carry_adopt_check


@pytest.mark.parametrize("shift", range(len(KS)))
def test_every_k_against_the_restatement(gpu_ctx, images, shift):
    """Pair b's old keyframe has KS[shift + b] points, its new one KS[shift + b + 3]; pairs 0 and 2 are listed, pair 1 is not."""
    sharp, blur = images
    rng = np.random.default_rng(100 + shift)
    ka, kb = [KS[(shift + b) % 7] for b in range(B)], [KS[(shift + b + 3) % 7] for b in range(B)]
    pb = _object(gpu_ctx)
    old = [_points(rng, k) for k in ka]
    if ka[0] >= 8:
        old[0] = _special(*old[0])
    counts = pb.prepare_points(sharp, blur, old)
    assert counts[:, 0].tolist() == ka and (counts[:, 1] <= counts[:, 0]).all()
    listed, Ts = [0, 2], np.stack([HALF, TILT])
    if ka[2] >= 4:  # one point behind the new camera (TILT moves it 0.3 forward), invalid depths
        q = pb.array[2 * L]
        z = dv.peek(q.d_kp_z, q.K, np.float64)
        z[:4] = [0.2, np.nan, 0.0, -1.0]
        dv.poke(q.d_kp_z, z)
    _, saved = _save(pb, listed, Ts, tag="K %s" % ka, **SAVE)
    assert pb.carry_stats()[0] == (2, 1, 24 * len(listed) * L)
    if ka[0] >= 8:
        s, xy0 = saved[(0, 0)], _entry(pb, 0, 0)[0]
        at = lambda x, y: np.flatnonzero((xy0[:, 0] == x) & (xy0[:, 1] == y))
        assert all(s["px"][i].tolist() == [63, 47] for i in at(62, 47)) and len(at(62, 47)) >= 1  # exactly on the last row and column
        assert all(s["px"][i].tolist() == [-1, -1] for i in at(63, 20)) and len(at(63, 20)) >= 1  # u + 0.5 = W: dropped
        assert len(at(30, 30)) >= 2 and all(s["px"][i].tolist() == [31, 30] for i in at(30, 30))    # two sources, one pixel
    if ka[2] >= 4:
        assert not saved[(2, 0)]["carried"][:4].any()
    new = [_points(rng, k) for k in kb]
    if kb[0] >= 8:
        new[0][0][:3] = [[63, 47], [62, 46], [31, 30]]
    counts = pb.update_points(None, [0, 1, 2], sharp, new)
    assert counts[:, 0].tolist() == kb
    _, _, res = _adopt(pb, listed, saved, SAVE["radius"], tag="K %s -> %s" % (ka, kb), apply=True, **ADOPT)
    assert pb.carry_stats()[1] == (1, 1, 32 * len(listed) * L)
    if ka[0] >= 257 and kb[0] >= 257:
        assert {0, 1, 2} <= set(res[(0, 0)]["flags"].tolist())
    # disarmed: a second adopt is rejected, nothing launched
    assert pb.carry_adopt(listed, **ADOPT)[0] == E_ARG and pb.carry_stats()[1] == (0, 0, 0)
    pb.close()


def _pair(rng, k=600):
    xy, z = _special(*_points(rng, k))
    return xy, z


def test_apply_0_changes_nothing_runs_repeat_and_a_pair_alone_gives_the_same_bits(gpu_ctx, images):
    sharp, blur = images
    rng = np.random.default_rng(7)
    old, new = [_pair(rng) for _ in range(B)], [_points(rng, 600) for _ in range(B)]
    pb = _object(gpu_ctx)
    pb.prepare_points(sharp, blur, old)
    listed, Ts = [0, 1, 2], np.stack([HALF, TILT, IDENT])
    out1, saved = _save(pb, listed, Ts, tag="batch", **SAVE)
    assert pb.carry_save(listed, Ts, want_records=False, **SAVE)[0] == 0 and pb.carry_stats()[0] == (2, 0, 0)  # replaces the sets; no wait
    out2, _ = _save(pb, listed, Ts, tag="again", **SAVE)
    assert bytes(out1) == bytes(out2)
    counts = pb.update_points(None, listed, sharp, new)
    held = dv.read_batch(pb, counts)
    rec1, arr1, _ = _adopt(pb, listed, saved, SAVE["radius"], tag="apply 0", apply=False, **ADOPT)
    dv.assert_twins(dv.read_batch(pb, counts), held, "apply = 0")
    # the old keyframes again, armed again: the same sets, the same answer; then without records nothing is waited for
    pb.prepare_points(sharp, blur, old)
    assert pb.carry_save(listed, Ts, want_records=False, **SAVE)[0] == 0
    pb.update_points(None, listed, sharp, new)
    rec2, arr2, _ = _adopt(pb, listed, saved, SAVE["radius"], tag="apply 0 again", apply=False, **ADOPT)
    assert bytes(rec1) == bytes(rec2) and all(np.array_equal(arr1[k].view(np.uint8), arr2[k].view(np.uint8)) for k in arr1)
    assert pb.carry_save(listed, Ts, want_records=False, **SAVE)[0] == 0
    assert pb.carry_adopt(listed, want_records=False, **ADOPT)[0] == 0 and pb.carry_stats()[1] == (1, 0, 0)
    pb.close()
    # pair 1 alone in an object of B = 1: the same bits in its records and arrays
    solo = _object(gpu_ctx, 1)
    solo.prepare_points(sharp[1:2].contiguous(), blur[1:2].contiguous(), old[1:2])
    rc, s1 = solo.carry_save([0], Ts[1:2], **SAVE)
    assert rc == 0 and bytes(s1) == bytes(out1)[24 * L:48 * L]
    solo.update_points(None, [0], sharp[1:2].contiguous(), new[1:2])
    t = _arrays(solo)
    rc, a1 = solo.carry_adopt([0], **t, **ADOPT)
    assert rc == 0 and bytes(a1) == bytes(rec1)[32 * L:64 * L]
    for k, v in t.items():
        assert np.array_equal(v.cpu().numpy()[0].view(np.uint8), arr1[k][1].view(np.uint8)), k
    solo.close()


def test_filter_weights_and_the_seeded_state(gpu_ctx, images):
    sharp, blur = images
    rng = np.random.default_rng(9)
    old, new = [_pair(rng) for _ in range(B)], [_points(rng, 600) for _ in range(B)]
    pb = _object(gpu_ctx)
    m = dict(cap=np.full(B, 0.2), exp=np.full(B, 0.04), t0=np.zeros(B), dt=0.5, kt=np.zeros((B, N, 3)), kR=np.tile([0, 0, 0, 1.0], (B, N, 1)))
    assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
    pb.prepare_points(sharp, blur, old)
    listed, Ts = [0, 2], np.stack([HALF, TILT])
    # before the filter's first accepted call: weights = 1 and seed_filter = 1 are rejected
    assert pb.carry_save(listed, Ts, weights=1, **SAVE)[0] == E_ARG and pb.carry_stats()[0] == (0, 0, 0)
    assert pb.carry_save(listed, Ts, **SAVE)[0] == 0
    assert pb.carry_adopt(listed, apply=True, seed_filter=True, **ADOPT)[0] == E_ARG and pb.carry_stats()[1] == (0, 0, 0)
    rc, fil = pb.filter_depths(level=-1, prior_rel_sigma=0.05, sigma_i=2.0)
    assert rc == 0 and all(f.seeded == 1 for f in fil)
    st = pb.filter_state()
    info = st["info"].cpu().numpy()
    info *= rng.uniform(0.5, 2.0, info.shape)
    info[0, [5, 17]] = [0.0, np.nan]
    st["info"].copy_(dv.dev(info)[0])
    _, saved = _save(pb, listed, Ts, info=info, tag="weights 1", weights=1, **SAVE)
    assert not saved[(0, 0)]["carried"][[5, 17]].any()
    pb.update_points(None, [0, 1, 2], sharp, new)
    keep = {k: st[k].cpu().numpy().copy() for k in ("mu", "info", "n_obs", "n_rej")}
    kw = dict(ADOPT, prior_rel_sigma=0.1, max_info=float(np.nanmedian(info[0, :600])))
    assert pb.carry_adopt(listed, apply=False, seed_filter=True, **kw)[0] == E_ARG  # seed_filter needs apply
    _, _, res = _adopt(pb, listed, saved, SAVE["radius"], tag="seed", apply=True, seed_filter=True, **kw)
    cap = pb.capacities()
    capped = 0
    for b in range(B):
        for l in range(L):
            o0, K = sum(cap[:l]), pb.array[b * L + l].K
            now = {k: st[k].cpu().numpy()[b, o0:o0 + cap[l]] for k in keep}
            if b not in listed:
                assert all(np.array_equal(now[k].view(np.uint8), keep[k][b, o0:o0 + cap[l]].view(np.uint8)) for k in keep), (b, l)
                continue
            r = res[(b, l)]
            assert _bits(now["mu"][:K], r["mu"]) and _bits(now["info"][:K], r["info_state"]), (b, l)
            assert (now["n_obs"][:K] == 0).all() and (now["n_rej"][:K] == 0).all()
            assert all(np.array_equal(now[k][K:].view(np.uint8), keep[k][b, o0 + K:o0 + cap[l]].view(np.uint8)) for k in keep), (b, l, "from K on")
            capped += int((r["info_state"][r["flags"] == 1] == kw["max_info"]).sum())
    assert capped > 0
    # the next filter call does not seed over it: the listed pairs report seeded = 0, the unlisted one (new keypoints) 1
    rc, fil = pb.filter_depths(level=-1, prior_rel_sigma=0.05, sigma_i=2.0)
    assert rc == 0 and [f.seeded for f in fil] == [0, 0, 1, 1, 0, 0]
    pb.close()


def test_rejections(gpu_ctx, images):
    sharp, blur = images
    rng = np.random.default_rng(3)
    fresh = _object(gpu_ctx, 1, 1)
    assert fresh.carry_save([0], IDENT[None], **SAVE)[0] == E_ARG and fresh.carry_stats() == ((0, 0, 0), (0, 0, 0))  # before the first prepare
    assert fresh.carry_adopt([0], **ADOPT)[0] == E_ARG
    fresh.close()
    pb = _object(gpu_ctx)
    pb.prepare_points(sharp, blur, [_points(rng, 100) for _ in range(B)])
    lib, capi = gpu_ctx.lib, __import__("mba_vo_amd").capi
    T2 = np.stack([IDENT, TILT])
    assert pb.carry_adopt([0], **ADOPT)[0] == E_ARG  # never armed
    so, ao = cref.save_opts(capi, **SAVE), cref.adopt_opts(capi, **ADOPT)
    for pairs, T, o in (([0, 1], T2, None), (None, T2, so), ([0, 1], None, so), ([], T2, so), ([1, 0], T2, so), ([1, 1], T2, so), ([0, 3], T2, so),
                        ([-1, 0], T2, so), ([0, 1, 2, 2], np.stack([IDENT] * 4), so)):
        assert cref.call_save(lib, pb.handle, pairs, T, o) == E_ARG, (pairs,)
        assert pb.carry_stats()[0] == (0, 0, 0)
    bad_T = []
    for j, v in ((0, np.nan), (2, np.inf), (6, 1.001), (6, 0.0), (3, np.nan), (6, 1.0 + 3e-9)):
        T = IDENT.copy()
        T[j] = v
        bad_T.append(T)
    for T in bad_T:
        assert pb.carry_save([1], T[None], **SAVE)[0] == E_ARG and pb.carry_stats()[0] == (0, 0, 0), T
    for kw in (dict(radius=0), dict(radius=17), dict(deflate=0.0), dict(deflate=1.01), dict(deflate=float("nan")), dict(weights=2), dict(weights=-1),
               dict(weights=1), dict(z_min=-1.0), dict(z_max=float("inf")), dict(z_min=float("nan")), dict(z_min=3.0, z_max=2.0)):
        assert pb.carry_save([0, 1], T2, **dict(SAVE, **kw))[0] == E_ARG and pb.carry_stats()[0] == (0, 0, 0), kw
    assert pb.carry_adopt([0], **ADOPT)[0] == E_ARG  # still not armed
    assert pb.carry_save([0, 1], T2, z_min=1.0, z_max=1.0, **SAVE)[0] == 0  # (the limits may coincide)
    zs = [_entry(pb, b, l)[1] for b in range(B) for l in range(L)]
    for pairs, o in (([0, 1], None), (None, ao), ([], ao), ([1, 0], ao), ([0, 0], ao), ([0, 3], ao), ([0, 2], ao)):  # (pair 2 is not armed)
        assert cref.call_adopt(lib, pb.handle, pairs, o) == E_ARG, (pairs,)
        assert pb.carry_stats()[1] == (0, 0, 0)
    for kw in (dict(apply=2), dict(apply=-1), dict(seed_filter=2), dict(seed_filter=1, apply=1), dict(min_support=0), dict(max_rel_diff=0.0),
               dict(max_rel_diff=1.5), dict(max_rel_diff=float("nan")), dict(z_min=-1.0), dict(z_max=-1.0), dict(z_max=float("inf")),
               dict(z_min=3.0, z_max=2.0), dict(prior_rel_sigma=-1.0), dict(max_info=float("nan"))):
        assert pb.carry_adopt([0, 1], **dict(ADOPT, **kw))[0] == E_ARG and pb.carry_stats()[1] == (0, 0, 0), kw
    assert all(_bits(z, _entry(pb, b, l)[1]) for z, (b, l) in zip(zs, [(b, l) for b in range(B) for l in range(L)]))
    assert pb.carry_adopt([0, 1], apply=True, **ADOPT)[0] == 0  # a rejected call disarms nothing
    pb.close()


def test_the_smoothing_through_the_shared_index_body_is_unchanged(gpu_ctx, images):
    """One case of tests/test_gpu_pairs_smooth.py again (its 700-point list without the pokes): flags, support and rho' bit for bit
    against the smoothing's own restatement, two launches."""
    import torch
    sharp, blur = images
    rng = np.random.default_rng(21)
    pb = _object(gpu_ctx)
    pts = [_points(rng, 700), (np.array([[20.0, 20.0]]), np.array([2.0])), (np.zeros((0, 2)), np.zeros(0))]
    pb.prepare_points(sharp, blur, pts)
    cap = pb.capacities()
    n = sum(cap)
    t = dict(rho=torch.full((B, n), -7.0, dtype=torch.float64, device="cuda:0"), flags=torch.full((B, n), 77, dtype=torch.uint8, device="cuda:0"),
             support=torch.full((B, n), -7, dtype=torch.int32, device="cuda:0"))
    kw = dict(radius=3, min_support=2, max_rel_diff=0.1, strength=0.7, fill=1)
    before = {(b, l): _entry(pb, b, l) for b in range(B) for l in range(L)}
    rc, out = pb.smooth_depths(**t, **kw)
    assert rc == 0 and pb.smooth_stats()[0] == 2
    arr = {k: v.cpu().numpy() for k, v in t.items()}
    for (b, l), (xy, z, _, _) in before.items():
        m = mref.smooth(xy, z, **kw)
        o0, K = sum(cap[:l]), len(z)
        assert np.array_equal(arr["flags"][b, o0:o0 + K], m["flags"]) and np.array_equal(arr["support"][b, o0:o0 + K], m["support"]), (b, l)
        assert _bits(arr["rho"][b, o0:o0 + K], m["rho"]), (b, l)
    pb.close()


def test_property_two_keyframes_of_a_rendered_scene(gpu_ctx, mbavo, images):
    """tests/test_pairs_carry_api.py's property with both calls on the device: the same bound on the adopted depths, the
    restatement's share."""
    sharp, blur = images
    scene = cref.property_scene(mbavo.load(), mbavo.capi, H, W)
    r = cref.PROPERTY["radius"]
    pb = _object(gpu_ctx, 1, 1)
    assert np.array_equal(scene["intr"], pb.intr)
    s1, b1 = sharp[:1].contiguous(), blur[:1].contiguous()
    assert pb.prepare_points(s1, b1, [scene["A"]]).tolist() == [[len(scene["A"][1])]]
    _, saved = _save(pb, [0], scene["T"][None], tag="property", radius=r)
    assert pb.update_points(None, [0], s1, [scene["B"]]).tolist() == [[len(scene["B"][1])]]
    _, _, res = _adopt(pb, [0], saved, r, tag="property", apply=True, **{k: v for k, v in cref.PROPERTY.items() if k != "radius"})
    z = _entry(pb, 0, 0)[1]
    want = cref.adopt(*scene["B"], cref.save(*scene["A"], scene["intr"], W, H, scene["T"]), **cref.PROPERTY)
    share_ref, _ = cref.property_figures(scene, want, r)
    share, worst = cref.property_figures(scene, dict(res[(0, 0)], z_new=z), r)
    print("on the device: adopted share %.4f (restated %.4f); largest error / ((radius + 1) gradient) = %.3f" % (share, share_ref, worst))
    assert share == share_ref and share >= cref.property_share_bound(scene, r)
    assert worst <= 1.0
    pb.close()
