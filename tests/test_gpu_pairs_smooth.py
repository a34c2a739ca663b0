"""mbavo_pairs_smooth_depths on the device, through the C ABI, held to the numpy restatement (tests/pairs_smooth_ref.py: a brute-force
neighbour search, no bins) on the object's own device arrays.  Flags, support counts, rho' and the depths after apply = 1 are held
bit for bit -- the order of the sums is specified; sum_sq_rel within K 2^-52 relative (a sum of K non-negative terms in any order)
and bit-identical from run to run and between B = 1 and B = 3.

Objects come from prepare_points, so coordinates are exact: every-candidate objects of 48 x 64 with border 0 (B = 3, L = 2: a list of
700 points with the image border, the bin seams and shared pixels in it, K = 1 and K = 0; B = 1, L = 1: K = capacity = 3072 > 1024
in descending raster order and as a random permutation) and one B = 1 object of 640 x 480 at radius 2, where the bin edge is 9."""

import numpy as np
import pytest

import pairs_cases
import pairs_depth_cases as dc
import pairs_depth_support as ds
import pairs_device as dv
import pairs_refine_scene as sc
import pairs_smooth_ref as mref
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

E_ARG = -1
H, W, B = 48, 64, 3
K_DEG, N, S = 4, 4, 3


def _motion(nb):
    rng = np.random.default_rng(11)
    kt, kR = np.zeros((nb, N, 3)), np.zeros((nb, N, 4))
    for b in range(nb):
        kt[b], kR[b] = synth.trajectory("harness", N, 0.004 * (b + 1), 0.01 * (b + 1))
        kt[b] += rng.normal(0, 0.02, 3)
    return dict(cap=(0.4 + 0.05 * np.arange(nb)) * 0.5, exp=np.full(nb, 0.04), t0=np.zeros(nb), dt=0.5, kt=kt, kR=kR)


def _object(ctx, nb, levels, h=H, w=W, motion=True):
    from mba_vo_amd import workloads
    pb = workloads.PairBatch(ctx, nb, L=levels, H=h, W=w, S=S, k=K_DEG, N=N, cell=0, thresh=4.0, border=0, every_candidate=True)
    if motion:
        m = _motion(nb)
        assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
    return pb


def _images(nb, h=H, w=W):
    sharp, _, blur = pairs_cases.inputs(nb, h, w, seed=4, special=False)
    return dv.dev(sharp, blur)


_depths = dc.surface_depths


def _list700(rng, s):
    """Level-0 points: random ones, the four image borders, the seams of bins of edge s, and pixels that are shared."""
    pts = [np.stack([rng.integers(0, W, 520), rng.integers(0, H, 520)], 1)]
    pts.append(np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [0, 7], [W - 1, 9], [30, 0], [31, H - 1]]))
    seam = [[x, y] for x in (s - 1, s, 2 * s - 1, 2 * s) for y in range(0, 20)] + [[x, y] for y in (s - 1, s) for x in range(20, 40)]
    pts.append(np.array(seam))
    p = np.concatenate(pts)
    p = np.concatenate([p, p[:700 - len(p)]])  # shared pixels
    assert len(p) == 700
    return p[rng.permutation(700)].astype(np.float64)


_entry, _layout, _bits, _smooth, _check = ds.smooth_entry, ds.level_layout, ds.bits, ds.smooth_run, ds.smooth_check


@pytest.fixture(scope="module")
def small(gpu_ctx):
    """B = 3, L = 2: pair 0 the 700-point list, pair 1 one point, pair 2 none; depths with invalid ones poked in."""
    rng = np.random.default_rng(21)
    pb = _object(gpu_ctx, B, 2)
    sharp, blur = _images(B)
    pts = [(_list700(rng, 3), _depths(rng, 700)), (np.array([[20.0, 20.0]]), np.array([2.0])), (np.zeros((0, 2)), np.zeros(0))]
    counts = pb.prepare_points(sharp, blur, pts)
    assert counts[:, 0].tolist() == [700, 1, 0] and 600 < counts[0, 1] < 700 and counts[1:, 1].tolist() == [1, 0]  # (x = 63 leaves level 1)
    for l in range(2):  # invalid depths: NaN, inf, 0, negative
        q = pb.array[l]
        z = dv.peek(q.d_kp_z, q.K, np.float64)
        z[[3, 50, 333, q.K - 1]] = [np.nan, np.inf, 0.0, -2.0]
        dv.poke(q.d_kp_z, z)
    yield dict(pb=pb, sharp=sharp, blur=blur, pts=pts, counts=counts)
    pb.close()


OPTS = dict(radius=3, min_support=2, max_rel_diff=0.1, strength=0.7, fill=1)


def test_rejections(gpu_ctx, small):
    pb = small["pb"]
    fresh = _object(gpu_ctx, 1, 1, motion=False)
    assert fresh.smooth_depths(**OPTS)[0] == E_ARG and fresh.smooth_stats() == (0, 0, 0)  # before the first prepare
    fresh.close()
    lib, capi = gpu_ctx.lib, __import__("mba_vo_amd").capi
    assert mref.call(lib, pb.handle, None) == E_ARG
    import torch
    wt = torch.ones(pb.B * sum(pb.capacities()), dtype=torch.float64, device="cuda:0")
    bad = [dict(level=-2), dict(level=2), dict(apply=2), dict(fill=-1), dict(sync_filter=2), dict(weights=3), dict(weights=-1), dict(weights=1),
           dict(sync_filter=1, apply=1), dict(weights=2), dict(radius=0), dict(radius=17), dict(min_support=0), dict(max_rel_diff=0.0),
           dict(max_rel_diff=1.5), dict(max_rel_diff=float("nan")), dict(strength=0.0), dict(strength=1.01), dict(max_intensity_diff=-1),
           dict(max_intensity_diff=256), dict(z_min=-1.0), dict(z_max=-1.0), dict(z_max=float("inf")), dict(z_min=float("nan")), dict(z_min=3.0, z_max=2.0)]
    zs = [_entry(pb, 0, l)[1] for l in range(2)]
    for kw in bad:  # (weights = 1 and sync_filter = 1: no filter call yet; weights = 2: no array)
        assert pb.smooth_depths(**dict(OPTS, **kw))[0] == E_ARG, kw
        assert pb.smooth_stats() == (0, 0, 0)
    assert pb.smooth_depths(**dict(OPTS, weights=2, weight=wt, z_min=1.0, z_max=1.0))[0] == 0  # (the limits may coincide)
    assert all(_bits(zs[l], _entry(pb, 0, l)[1]) for l in range(2))


def test_apply_0_against_the_restatement_changes_nothing_and_needs_no_motion(gpu_ctx, small):
    pb = small["pb"]
    held = dv.read_batch(pb, small["counts"])
    rc, rec0 = pb.refine_depths(level=-1)
    assert rc == 0
    rc, sea0 = pb.search_depths(8, 0.3, 1.1, level=-1)
    assert rc == 0
    for tag, kw in (("fill", OPTS), ("no fill", dict(OPTS, fill=0, min_support=3)), ("gate", dict(OPTS, max_intensity_diff=12, radius=5)),
                    ("limits", dict(OPTS, z_min=1.5, z_max=2.9)), ("r16", dict(OPTS, radius=16, min_support=40, max_rel_diff=0.05))):
        out, arr, res = _check(pb, tag=tag, **kw)
        flags = np.concatenate([m["flags"] for m in res.values()])
        assert {0, 1, 3} <= set(flags.tolist()) and (tag != "fill" or 2 in flags), (tag, np.bincount(flags))
    dv.assert_twins(dv.read_batch(pb, small["counts"]), held, "apply = 0")
    rc, rec1 = pb.refine_depths(level=-1)
    assert rc == 0 and bytes(rec0) == bytes(rec1)
    rc, sea1 = pb.search_depths(8, 0.3, 1.1, level=-1)
    assert rc == 0 and bytes(sea0) == bytes(sea1)
    # no pose is read: an object without a motion
    nm = _object(gpu_ctx, B, 2, motion=False)
    nm.prepare_points(small["sharp"], small["blur"], small["pts"])
    _check(nm, tag="no motion", **OPTS)
    nm.close()


def test_levels_one_by_one_equal_level_minus_1_and_runs_repeat(small):
    pb = small["pb"]
    out, arr = _smooth(pb, **OPTS)
    again, arr2 = _smooth(pb, **OPTS)
    assert bytes(out) == bytes(again) and all(np.array_equal(arr[k].view(np.uint8), arr2[k].view(np.uint8)) for k in arr)
    cap = pb.capacities()
    for l in range(pb.L):
        one, a1 = _smooth(pb, level=l, **OPTS)
        o0 = sum(cap[:l])
        for b in range(pb.B):
            assert bytes(one[b]) == bytes(out[b * pb.L + l])
            K = pb.array[b * pb.L + l].K
            for k in arr:
                assert np.array_equal(a1[k][b, :K].view(np.uint8), arr[k][b, o0:o0 + K].view(np.uint8)), (l, b, k)


def test_stats_index_rebuilds_and_the_sum_for_any_B(gpu_ctx, small):
    pb = small["pb"]
    rec = 40
    fresh = _object(gpu_ctx, B, 2)
    fresh.prepare_points(small["sharp"], small["blur"], small["pts"])
    for l in range(2):
        dv.poke(fresh.array[l].d_kp_z, _entry(pb, 0, l)[1])
    out, _ = _smooth(fresh, **OPTS)
    assert fresh.smooth_stats() == (2, 1, rec * B * 2)  # index, gather
    out2, arr2 = _smooth(fresh, **OPTS)
    assert fresh.smooth_stats() == (1, 1, rec * B * 2) and bytes(out) == bytes(out2)
    assert fresh.smooth_depths(want_records=False, **OPTS)[0] == 0 and fresh.smooth_stats() == (1, 0, 0)
    _smooth(fresh, level=1, **OPTS)
    assert fresh.smooth_stats() == (1, 1, rec * B)
    _smooth(fresh, **dict(OPTS, radius=4))  # another bin edge
    assert fresh.smooth_stats()[0] == 2
    _smooth(fresh, **OPTS)
    assert fresh.smooth_stats()[0] == 2
    # new keypoints for pair 1 alone: its index is rebuilt, the other pairs' results stay
    rng = np.random.default_rng(5)
    pts1 = (np.stack([rng.integers(0, W, 300), rng.integers(0, H, 300)], 1).astype(np.float64), _depths(rng, 300))
    fresh.update_points(None, [1], small["sharp"][1:2], [pts1])
    out3, arr3, _ = _check(fresh, tag="after update_points", **OPTS)
    assert fresh.smooth_stats()[0] == 2
    for b in (0, 2):
        assert bytes(out3[2 * b]) == bytes(out2[2 * b]) and bytes(out3[2 * b + 1]) == bytes(out2[2 * b + 1])
        assert all(np.array_equal(arr3[k][b].view(np.uint8), arr2[k][b].view(np.uint8)) for k in arr3)
    _smooth(fresh, **OPTS)
    assert fresh.smooth_stats()[0] == 1
    fresh.close()
    # pair 0 alone in an object of B = 1: the same bits in its records
    solo = _object(gpu_ctx, 1, 2)
    solo.prepare_points(small["sharp"][:1].contiguous(), small["blur"][:1].contiguous(), small["pts"][:1])
    for l in range(2):
        dv.poke(solo.array[l].d_kp_z, _entry(pb, 0, l)[1])
    one, _ = _smooth(solo, **OPTS)
    assert bytes(one[0]) == bytes(out[0]) and bytes(one[1]) == bytes(out[1])
    solo.close()


def test_filter_weights_sync_and_caller_weights(gpu_ctx, small):
    pb = _object(gpu_ctx, B, 2)
    pb.prepare_points(small["sharp"], small["blur"], small["pts"])
    # (a filter call moves its own state, so "unchanged by a smooth with apply = 0" is held between twins: this object is smoothed
    # before its first filter call, the twin never)
    twin = _object(gpu_ctx, B, 2)
    twin.prepare_points(small["sharp"], small["blur"], small["pts"])
    assert pb.smooth_depths(**OPTS)[0] == 0
    rc, fil0 = twin.filter_depths(level=-1, apply=False, prior_rel_sigma=0.05, sigma_i=2.0)
    assert rc == 0
    twin.close()
    rc, fil1 = pb.filter_depths(level=-1, apply=False, prior_rel_sigma=0.05, sigma_i=2.0)
    assert rc == 0 and bytes(fil0) == bytes(fil1) and any(f.num_fused > 0 for f in fil1)
    st = pb.filter_state()
    rng = np.random.default_rng(8)
    info = st["info"].cpu().numpy()
    info *= rng.uniform(0.5, 2.0, info.shape)
    info[0, [5, 17]] = [0.0, np.nan]
    st["info"].copy_(dv.dev(info)[0])
    keep = {k: st[k].cpu().numpy().copy() for k in ("mu", "info", "n_obs", "n_rej")}
    # the filter is ready now: sync_filter = 1 without apply = 1 is still rejected, nothing launched, nothing changed
    zs = [_entry(pb, 0, l)[1] for l in range(2)]
    assert pb.smooth_depths(**dict(OPTS, weights=1))[0] == 0 and pb.smooth_stats()[0] > 0
    assert pb.smooth_depths(**dict(OPTS, sync_filter=1, apply=0))[0] == E_ARG and pb.smooth_stats() == (0, 0, 0)
    assert all(_bits(zs[l], _entry(pb, 0, l)[1]) for l in range(2))
    assert all(np.array_equal(st[k].cpu().numpy().view(np.uint8), keep[k].view(np.uint8)) for k in keep)
    out, arr, res = _check(pb, weights_of=info, tag="weights 1", weights=1, sync_filter=1, apply=1, **OPTS)
    cap = pb.capacities()
    for key in ("info", "n_obs", "n_rej"):
        assert np.array_equal(st[key].cpu().numpy().view(np.uint8), keep[key].view(np.uint8)), key
    mu = st["mu"].cpu().numpy()
    moved_any = 0
    for (b, l), m in res.items():
        o0, K = sum(cap[:l]), m["num_keypoints"]
        want = np.where(m["moved"], m["rho"], keep["mu"][b, o0:o0 + K])
        assert _bits(mu[b, o0:o0 + K], want) and _bits(mu[b, o0 + K:o0 + cap[l]], keep["mu"][b, o0 + K:o0 + cap[l]]), (b, l)
        moved_any += int(m["moved"].sum())
    assert moved_any > 100
    # the caller's weights, zeros and a NaN among them, in the layout of the level asked for
    for level in (-1, 1):
        n, _, _ = _layout(pb, level)
        w = rng.uniform(0.2, 3.0, (pb.B, n))
        w[0, [1, 2, 40]] = [0.0, np.nan, -1.0]
        _check(pb, level=level, weights_of=w, tag="weights 2", weights=2, **OPTS)
    pb.close()


def _raster(rng, order):
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    z = np.where(xy[:, 0] < 30, 2.0, 3.0) * (1.0 + rng.uniform(-0.03, 0.03, len(xy)))
    z[rng.uniform(size=len(z)) < 0.05] = 0.9
    return xy[order], z[order]


def test_capacity_in_descending_raster_order_and_permuted_with_apply_1(gpu_ctx):
    """K = capacity = 3072: twelve keypoints per lane of the index kernel's waves, twelve tiles over twelve workgroups.  apply = 1 is
    a Jacobi sweep: the depths after it are the restatement's, which reads old depths only."""
    rng = np.random.default_rng(2)
    sharp, blur = _images(1)
    n = H * W
    perm = rng.permutation(n)
    kept = {}
    for name, order in (("descending", np.arange(n)[::-1]), ("permuted", perm)):
        pb = _object(gpu_ctx, 1, 1)
        xy, z = _raster(np.random.default_rng(9), order)
        assert pb.prepare_points(sharp, blur, [(xy, z)]).tolist() == [[n]]
        _, arr, res = _check(pb, tag=name, apply=1, radius=2, min_support=4, max_rel_diff=0.1, strength=1.0, fill=1)
        _check(pb, tag=name + ", second sweep", apply=1, radius=2, min_support=4, max_rel_diff=0.1, strength=1.0, fill=1)
        back = np.empty(n, np.int64)
        back[order] = np.arange(n)
        kept[name] = (arr["flags"][0][back], arr["support"][0][back])
        pb.close()
    # the classes and support counts are the keypoints', whatever their order in the list
    assert np.array_equal(kept["descending"][0], kept["permuted"][0]) and np.array_equal(kept["descending"][1], kept["permuted"][1])


def test_bins_wider_than_the_radius_at_640_x_480(gpu_ctx):
    """radius 2 at 640 x 480: 320 x 240 bins of edge 2 are too many, the edge is 9 (72 x 54 bins)."""
    h, w, s = 480, 640, 9
    rng = np.random.default_rng(13)
    pb = _object(gpu_ctx, 1, 1, h=h, w=w)
    sharp, blur = _images(1, h, w)
    seam = [[x, y] for x in (s - 1, s, 8 * s - 1, 8 * s) for y in range(0, 40)] + [[x, y] for y in (s - 1, s, 5 * s - 1, 5 * s) for x in range(0, 40)]
    edge = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [w - 1, h - 2], [w - 2, h - 1], [638, 478]]
    dense = np.stack([rng.integers(0, 90, 1200), rng.integers(0, 60, 1200)], 1)
    far = np.stack([rng.integers(0, w, 200), rng.integers(0, h, 200)], 1)
    xy = np.concatenate([np.array(seam), np.array(edge), dense, far]).astype(np.float64)
    xy = xy[rng.permutation(len(xy))]
    assert pb.prepare_points(sharp, blur, [(xy, _depths(rng, len(xy)))]).tolist() == [[len(xy)]]
    _check(pb, tag="s = 9", radius=2, min_support=2, max_rel_diff=0.1, strength=1.0, fill=1)
    assert pb.smooth_stats()[0] == 2
    _check(pb, tag="s = 9, radius 3", apply=1, radius=3, min_support=2, max_rel_diff=0.1, strength=1.0, fill=1)
    assert pb.smooth_stats()[0] == 1  # (radius 3 has the same bin edge: the index stands)
    pb.close()


@pytest.mark.parametrize("b", range(sc.B))
def test_one_sweep_after_the_search_brings_keypoints_back_within_a_step(gpu_ctx, mbavo, b):
    """tests/test_pairs_smooth_api.py's property with the sweep on the device, the bare inequalities."""
    e, truth, s = mref.noisy_search(mbavo.load(), mbavo.capi, b)
    pb = _object(gpu_ctx, 1, 1, h=sc.H, w=sc.W, motion=False)
    sharp, blur = dv.dev(np.ascontiguousarray(e["ref"][None]), np.ascontiguousarray(e["curs"][0][None]))
    assert pb.prepare_points(sharp, blur, [(e["xy"], s["z_new"])]).tolist() == [[e["K"]]]
    _, _, res = _check(pb, tag="property", apply=1, **mref.SWEEP)
    z = _entry(pb, 0, 0)[1]
    (off0, med0), (off1, med1) = mref.figures(s["z_new"], truth, s), mref.figures(z, truth, s)
    print("pair %d on the device: over a step off %d -> %d; median relative error %.4f -> %.4f" % (b, off0, off1, med0, med1))
    assert off1 <= off0 and (off0 == 0 or off1 < off0) and med1 <= med0
    pb.close()
