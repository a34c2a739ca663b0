"""The five depth stages of the pairs batch (refine, filter, search, smooth, carry) on the option-laden objects A - D of
tests/pairs_oracle.py, each held to its numpy restatement run on entries rebuilt from the object's own device arrays
(pairs_oracle.read_entry) -- the checks of tests/test_gpu_pairs_{refine,filter,search,smooth,carry}.py, shared through
tests/pairs_depth_support.py.  The stage tests themselves build one pinhole camera, 48 x 64 images and L <= 2; here the kernels run
with a camera set (objects B and D: a.of_pair[b], every level scaled from the pair's own camera), odd sizes under a packed keyframe
(A: 75 x 101), L = 3 (D: the third slot offset of level = -1), per-level K that differ (D: the caller's points) and
clearance-filtered lists (B, D).  What these objects must provide is asserted without a GPU in
tests/test_pairs_depth_options_inputs.py.

Bounds.  Integer outputs, flags, support counts and applied-or-not masks are identical.  What the stage files hold bit for bit is
held bit for bit: the smoothing and the carry, the search's selection and records on the device's own volume, and the volume against
mbavo_pairs_refine_depths at every candidate.  The doubles of refine, filter and the search's volume, which depend on the device's
pose prologue, are held to BOUND = 1e-9 per array (max |device - restatement| / max |restatement|), the figure of
tests/test_gpu_fullsize.py.  Keypoints on a knife edge (pairs_depth_support.knife: from the restatement alone) are left out, at most
1 % of a (pair, level); the number is printed.  Every figure is printed before it is asserted (-s); the largest per stage and object
on an MI355X are in profiles/r36_depth_options.txt."""
import contextlib

import numpy as np
import pytest

import pairs_carry_ref as cref
import pairs_depth_cases as dc
import pairs_depth_support as ds
import pairs_device as dv
import pairs_oracle as po
import pairs_refine_ref as ref
import pairs_search_ref as sref

pytestmark = pytest.mark.gpu

NAMES = sorted(po.OBJECTS)
BOUND = 1e-9


@pytest.fixture(scope="module")
def made(mbavo, gpu_ctx):
    """name -> (pb, counts): each object made once for the report-only checks, closed at the end of the module."""
    held = {}

    def get(name):
        if name not in held:
            held[name] = po.make_object(gpu_ctx, name)
        return held[name]
    yield get
    for pb, _ in held.values():
        pb.close()


@contextlib.contextmanager
def _second(ctx, name):
    """A second instance for the calls that write (apply = 1, the filter's state, the carry's update)."""
    pb, counts = po.make_object(ctx, name)
    try:
        yield pb, counts
    finally:
        pb.close()


def _figures(stage, name, log):
    print("FIGURE %-6s object %s: largest relative difference %.3g, keypoints left out %d of %d"
          % (stage, name, max(x[5] for x in log), sum(x[4] for x in log), sum(x[3] for x in log)))


@pytest.mark.parametrize("name", NAMES)
def test_refine(mbavo, gpu_ctx, made, name):
    o = po.OBJECTS[name]
    log = []
    pb, counts = made(name)
    ds.refine_check(mbavo, gpu_ctx, pb, counts, o["k"], name + " report", BOUND, level=-1, exclude=True, log=log, **dc.REFINE)
    assert sum(x[7]["num_moved"] for x in log) > 0 and sum(x[3] - x[7]["num_moved"] for x in log) > 0
    with _second(gpu_ctx, name) as (pb, counts):
        for l in range(o["L"]):
            ds.refine_check(mbavo, gpu_ctx, pb, counts, o["k"], "%s apply level %d" % (name, l), BOUND, level=l, apply=True, exclude=True, log=log, **dc.REFINE)
    _figures("refine", name, log)


@pytest.mark.parametrize("name", ["B", "D"])
def test_a_wrong_camera_must_fail(mbavo, gpu_ctx, made, name):
    """The comparison sees the fault it is there for: pair 0's restatement with pair 1's intrinsics is far from the device's g."""
    o = po.OBJECTS[name]
    log = []
    pb, counts = made(name)
    ds.refine_check(mbavo, gpu_ctx, pb, counts, o["k"], name + " report", BOUND, level=-1, exclude=True, log=log)
    by = {(b, l): x for x in log for b, l in [(x[1], x[2])]}
    for l in range(o["L"]):
        e, got = by[(0, l)][8], by[(0, l)][6]
        wrong = ref.refine(gpu_ctx.lib, mbavo.capi, dict(e, intr=by[(1, l)][8]["intr"]), o["k"], pb.capacities()[l])
        d = ds.rel(got["g"], wrong["g"])
        print("%s level %d: the device's g against pair 0's restatement under pair 1's camera: %.3g" % (name, l, d))
        assert d > 1e-6, (name, l, d)


@pytest.mark.parametrize("name", NAMES)
def test_filter(mbavo, gpu_ctx, name):
    o = po.OBJECTS[name]
    every, none = [[True] * o["L"] for _ in range(o["B"])], [[False] * o["L"] for _ in range(o["B"])]
    log = []
    with _second(gpu_ctx, name) as (pb, counts):
        ds.filter_check(mbavo, gpu_ctx, pb, o["k"], name + " call 0", every, BOUND, first=True, exclude=True, log=log, **dc.FILTER)
        _, out = ds.filter_check(mbavo, gpu_ctx, pb, o["k"], name + " call 1", none, BOUND, exclude=True, log=log, **dc.FILTER)
        assert sum(r.num_fused for r in out) > 0
        if name == "D":
            _, out = ds.filter_check(mbavo, gpu_ctx, pb, o["k"], name + " reset", every, BOUND, exclude=True, log=log, reset=1, **dc.FILTER)
            assert all(r.seeded == 1 for r in out)
    _figures("filter", name, log)


def _volume_is_the_refinement(pb, arr, z0, nd, lo, hi, relative, tag):
    """The device's volume against refine_depths(apply = 0) with each candidate's depths written into the object, bit for bit."""
    import torch
    n, off, levels = ds.level_layout(pb, -1)
    cost = torch.zeros((pb.B, n), dtype=torch.float64, device="cuda:0")
    valid = torch.zeros((pb.B, n), dtype=torch.int32, device="cuda:0")
    for d in range(nd):
        for e in range(pb.B * pb.L):
            dv.poke(pb.array[e].d_kp_z, np.ascontiguousarray(sref.candidates(z0[e], nd, lo, hi, relative)[3][:, d]))
        assert pb.refine_depths(level=-1, apply=False, cost=cost, valid=valid)[0] == 0
        c, v = cost.cpu().numpy(), valid.cpu().numpy()
        for b in range(pb.B):
            for l in levels:
                K, P = pb.array[b * pb.L + l].K, pb.array[b * pb.L + l].P
                full = v[b, off[l]:off[l] + K] == P
                got = arr["volume"][b, off[l]:off[l] + K, d]
                assert np.array_equal(np.isnan(got), ~full), (tag, d, b, l)
                assert dv.same_bits(got[full], c[b, off[l]:off[l] + K][full]), (tag, d, b, l)
    for e in range(pb.B * pb.L):
        dv.poke(pb.array[e].d_kp_z, z0[e])


@pytest.mark.parametrize("name", NAMES)
def test_search(mbavo, gpu_ctx, made, name):
    """ND = 6 is no multiple of the kernel's candidate batch.  apply = 0 at both kinds of range on the shared object (its depths are
    written for the volume check and put back), apply = 1 on a second one."""
    o, capi = po.OBJECTS[name], mbavo.capi
    log, n_acc, n_all = [], 0, 0
    pb, counts = made(name)
    for relative, (lo, hi) in enumerate((dc.ABSOLUTE, dc.RELATIVE)):
        tag = "%s relative %d" % (name, relative)
        entries = {(b, l): po.read_entry(capi, pb.array[b * pb.L + l], o["k"]) for b in range(pb.B) for l in range(pb.L)}
        z0 = ds.depths(pb)
        out, arr = ds.search_run(pb, dc.ND, lo, hi, relative=relative, min_ratio=dc.MIN_RATIO)
        res = ds.search_check_selection(pb, out, arr, dc.ND, lo, hi, relative=relative, z=z0, tag=tag, min_ratio=dc.MIN_RATIO)
        n_acc, n_all = n_acc + sum(int(a.sum()) for _, a, _ in res.values()), n_all + sum(a.size for _, a, _ in res.values())
        ds.search_check_volume(mbavo, gpu_ctx, pb, o["k"], entries, arr, dc.ND, lo, hi, BOUND, relative=relative, tag=tag, log=log)
        _volume_is_the_refinement(pb, arr, z0, dc.ND, lo, hi, relative, tag)
        assert all(dv.same_bits(a, b_) for a, b_ in zip(ds.depths(pb), z0))
    assert 0 < n_acc < n_all
    with _second(gpu_ctx, name) as (pb, counts):
        lo, hi = dc.RELATIVE
        z0 = ds.depths(pb)
        out, arr = ds.search_run(pb, dc.ND, lo, hi, relative=1, min_ratio=dc.MIN_RATIO, apply=True)
        res = ds.search_check_selection(pb, out, arr, dc.ND, lo, hi, relative=1, z=z0, tag=name + " apply", min_ratio=dc.MIN_RATIO)
        z1 = ds.depths(pb)
        for (b, l), (sel, acc, z_new) in res.items():
            e = b * pb.L + l
            assert dv.same_bits(z1[e][~acc], z0[e][~acc]) and dv.same_bits(z1[e][acc], (1.0 / sel["rho"])[acc]), (name, b, l)
        assert sum(r.num_accepted for r in out) == sum(int(a.sum()) for _, a, _ in res.values()) > 0
    _figures("search", name, log)


@pytest.mark.parametrize("name", NAMES)
def test_smooth(mbavo, gpu_ctx, name):
    """Bit for bit; on D once more with the filter's information as weights and the filter's mean kept in step."""
    with _second(gpu_ctx, name) as (pb, counts):
        out, arr, res = ds.smooth_check(pb, tag=name, apply=1, **dc.smooth_opts(name))
        flags = np.concatenate([m["flags"] for m in res.values()])
        print("FIGURE smooth object %s: bit for bit; classes (invalid, supported, filled, outlier) %s" % (name, np.bincount(flags, minlength=4).tolist()))
        assert {1, 2, 3} <= set(flags.tolist()) and sum(int(m["moved"].sum()) for m in res.values()) > 0
        if name != "D":
            return
        rc, fil = pb.filter_depths(level=-1, apply=False, **dc.FILTER)
        assert rc == 0 and any(f.num_fused > 0 for f in fil)
        st = pb.filter_state()
        keep = {k: st[k].cpu().numpy().copy() for k in ("mu", "info", "n_obs", "n_rej")}
        out, arr, res = ds.smooth_check(pb, weights_of=keep["info"], tag="D, the filter's weights", weights=1, sync_filter=1, apply=1, **dc.smooth_opts(name))
        cap = pb.capacities()
        for key in ("info", "n_obs", "n_rej"):
            assert np.array_equal(st[key].cpu().numpy().view(np.uint8), keep[key].view(np.uint8)), key
        mu, moved = st["mu"].cpu().numpy(), 0
        for (b, l), m in res.items():
            o0, K = sum(cap[:l]), m["num_keypoints"]
            want = np.where(m["moved"], m["rho"], keep["mu"][b, o0:o0 + K])
            assert ds.bits(mu[b, o0:o0 + K], want) and ds.bits(mu[b, o0 + K:o0 + cap[l]], keep["mu"][b, o0 + K:o0 + cap[l]]), (b, l)
            moved += int(m["moved"].sum())
        assert moved > 0


@pytest.mark.parametrize("name", sorted(dc.CARRY_PAIRS))
def test_carry(mbavo, gpu_ctx, name):
    """Save under the pair's own camera, the update to the next keyframe, adopt: bit for bit.  B: pair 2 (on camera 1, the unified
    one) through the second frame of tests/test_gpu_pairs_oracle.py; D: pairs 0 and 2 (cameras 0 and 2) through prepare_points
    with second lists.  A pair reading the wrong camera warps its points elsewhere and fails here."""
    o, c2 = po.OBJECTS[name], dc.second_inputs(name)
    listed = dc.CARRY_PAIRS[name]
    Ts = np.stack([dc.carry_pose(gpu_ctx.lib, mbavo.capi, name, b) for b in listed])
    with _second(gpu_ctx, name) as (pb, counts):
        _, saved = ds.carry_save_check(pb, listed, Ts, tag=name, intr_of=lambda b: po.to_intr(o, b), **dc.SAVE)
        n_car, n_all = sum(s["num_carried"] for s in saved.values()), sum(s["num_keypoints"] for s in saved.values())
        assert 0 < n_car < n_all
        if name == "B":
            c = po.inputs(name)
            new = pb.update(po._t(c["new_blur"]), [2], po._t(c["new_sharp"]), po._t(c["new_depth"]))
            assert not np.array_equal(new[2], counts[2])
        else:
            new = pb.prepare_points(po._t(c2["sharp"]), po._t(c2["blur"]), c2["points"])
        po.set_motion(pb, c2["motion"])
        _, _, res = ds.carry_adopt_check(pb, listed, saved, dc.SAVE["radius"], tag=name, apply=True, **dc.ADOPT)
        flags = np.concatenate([m["flags"] for m in res.values()])
        print("FIGURE carry  object %s: bit for bit; carried %d of %d; flags (empty, adopted, sparse, range) %s" % (name, n_car, n_all, np.bincount(flags, minlength=4).tolist()))
        assert (flags == cref.ADOPTED).any() and (flags != cref.ADOPTED).any()
