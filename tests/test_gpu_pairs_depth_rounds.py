"""The depth stages of the pairs batch with more than 64 tiles per (pair, level): a workgroup of every depth kernel takes a second
tile, and of the P = 8 kernels a third.  Each (pair, level) is served by G = min(64, ceil(capacity / T)) workgroups that loop over
tiles g, g + G, ..; the stage tests stop at K = 3072, where every workgroup has one tile.  Here one every-candidate object of
128 x 136 (capacity 17408, L = 1, the 8-pixel pattern) is filled through prepare_points (tests/pairs_depth_cases.py):

  pair 0, K = 16385: 65 tiles of 256 -- workgroup 0 of smooth / carry takes a second tile that holds one keypoint;
                     129 tiles of 128 -- workgroup 0 of refine / filter / search takes three tiles;
  pair 1, K = 17000: workgroups 0 - 2 take a second tile of 256, the last one ragged; workgroups 0 - 4 three tiles of 128.

So the reuse of a tile's LDS behind the trailing barrier, a lane's sums carried from tile to tile, the search's per-keypoint state
across tiles, the staging slots of later rounds and the index kernels at more than 64 members per lane all run, against the
restatements that already model them (pairs_refine_ref.lane_sum, pairs_carry_ref.record_sum).  Bounds: those of
tests/test_gpu_pairs_depth_options.py.  Besides, per stage: pair 1 alone in a B = 1 object returns the bits it has in the B = 2
object (the per-(pair, level) partial and ticket offsets differ between the two), and a report-only call repeated returns the
same bits (which it could not with a ticket left standing by the call before)."""
import numpy as np
import pytest

import pairs_depth_cases as dc
import pairs_depth_support as ds
import pairs_device as dv
import pairs_oracle as po

pytestmark = pytest.mark.gpu

BOUND = 1e-9
R = dc.ROUNDS
K_DEG = R["k"]
CAPACITY = 17408


def _object(ctx, sel=slice(None), which=0):
    """The rounds object (or the pairs `sel` of it alone) with its motion set and the invalid depths in place."""
    from mba_vo_amd import synth, workloads
    nb = len(range(R["B"])[sel])
    pb = workloads.PairBatch(ctx, nb, L=1, H=R["H"], W=R["W"], S=R["S"], k=K_DEG, N=R["N"], cell=0, every_candidate=True, border=0, pattern=synth.PATTERN8)
    try:
        assert pb.capacities() == [CAPACITY]
        _fill(pb, sel, which)
        m = dc.harness_motion(R["B"], R["N"])
        assert pb.set_motion(m["cap"][sel], m["exp"][sel], m["t0"][sel], m["dt"], m["kt"][sel], m["kR"][sel]) == 0
    except Exception:
        pb.close()
        raise
    return pb


def _fill(pb, sel=slice(None), which=0):
    """prepare_points with the lists `which`; a list's invalid depths are written afterwards, so that K is the list's length."""
    sharp, blur = dc.rounds_images()
    lists = dc.rounds_lists(which)[sel]
    clean = [(xy, np.where(np.isfinite(z) & (z > 0), z, 2.0)) for xy, z in lists]
    counts = pb.prepare_points(*dv.dev(np.ascontiguousarray(sharp[sel]), np.ascontiguousarray(blur[sel])), clean)
    assert counts.tolist() == [[len(z)] for _, z in lists]
    for b, (xy, z) in enumerate(lists):
        assert dv.same_bits(dv.peek(pb.array[b].d_kp_xy, 2 * len(z), np.float64).reshape(-1, 2), xy)
        dv.poke(pb.array[b].d_kp_z, z)
    return counts


@pytest.fixture(scope="module")
def both(gpu_ctx):
    """The B = 2 object for the report-only calls, and pair 1 alone in a B = 1 object."""
    pb, one = _object(gpu_ctx), None
    try:
        one = _object(gpu_ctx, slice(1, 2))
        yield pb, one
    finally:
        pb.close()
        if one is not None:
            one.close()


def _same_bits_alone_and_again(call, both, rec):
    """call(pb) -> (records, dict of host arrays, first axis the pair): twice on the B = 2 object, once on pair 1 alone."""
    pb, one = both
    out1, arr1 = call(pb)
    out2, arr2 = call(pb)
    assert bytes(out1) == bytes(out2) and all(arr1[k].tobytes() == arr2[k].tobytes() for k in arr1)
    outb, arrb = call(one)
    assert bytes(outb) == bytes(out1)[rec:2 * rec]
    assert all(arrb[k][0].tobytes() == arr1[k][1].tobytes() for k in arr1)


def test_the_object_holds_what_the_tiles_need(both):
    pb, one = both
    assert [pb.array[b].K for b in range(2)] == list(R["KS"]) and one.array[0].K == R["KS"][1]
    for K in R["KS"]:
        assert K > 64 * 256 and -(-K // 128) > 2 * 64 and K <= CAPACITY


def test_refine(mbavo, gpu_ctx, both):
    log = []
    pb = _object(gpu_ctx)
    try:
        counts = np.array([[K] for K in R["KS"]])
        ds.refine_check(mbavo, gpu_ctx, pb, counts, K_DEG, "rounds apply", BOUND, level=0, apply=True, exclude=True, log=log, **dc.REFINE)
    finally:
        pb.close()
    print("FIGURE refine object rounds: largest relative difference %.3g, keypoints left out %d" % (max(x[5] for x in log), sum(x[4] for x in log)))

    def call(p):
        out, arr, _ = ds.refine_run(p, 0, False, **dc.REFINE)
        return out, arr
    _same_bits_alone_and_again(call, both, 32)


def test_filter(mbavo, gpu_ctx, both):
    log = []
    pb = _object(gpu_ctx)
    try:
        ds.filter_check(mbavo, gpu_ctx, pb, K_DEG, "rounds call 0", [[True], [True]], BOUND, first=True, exclude=True, log=log, **dc.FILTER)
        _, out = ds.filter_check(mbavo, gpu_ctx, pb, K_DEG, "rounds call 1", [[False], [False]], BOUND, exclude=True, log=log, **dc.FILTER)
        assert all(r.num_fused > 0 and r.num_rejected > 0 for r in out)
    finally:
        pb.close()
    print("FIGURE filter object rounds: largest relative difference %.3g, keypoints left out %d" % (max(x[5] for x in log), sum(x[4] for x in log)))

    def call(p):  # (reset = 1: every call starts from the seeded state, whatever the calls before it left)
        out = ds.filter_run(p, level=0, apply=False, reset=1, **dc.FILTER)
        st, _ = ds.filter_state(p)
        return out, st
    _same_bits_alone_and_again(call, both, 48)


def test_search(mbavo, gpu_ctx, both):
    pb, one = both
    lo, hi = dc.RELATIVE
    log = []
    entries = {(b, 0): po.read_entry(mbavo.capi, pb.array[b], K_DEG) for b in range(2)}
    z0 = ds.depths(pb)
    out, arr = ds.search_run(pb, dc.ND, lo, hi, level=0, relative=1, min_ratio=dc.MIN_RATIO)
    res = ds.search_check_selection(pb, out, arr, dc.ND, lo, hi, level=0, relative=1, z=z0, tag="rounds", min_ratio=dc.MIN_RATIO)
    assert all(0 < a.sum() < a.size for _, a, _ in res.values())
    ds.search_check_volume(mbavo, gpu_ctx, pb, K_DEG, entries, arr, dc.ND, lo, hi, BOUND, level=0, relative=1, tag="rounds", log=log)
    print("FIGURE search object rounds: largest relative difference %.3g, keypoints left out %d" % (max(x[5] for x in log), sum(x[4] for x in log)))
    _same_bits_alone_and_again(lambda p: ds.search_run(p, dc.ND, lo, hi, level=0, relative=1, min_ratio=dc.MIN_RATIO), both, 32)


def test_smooth(gpu_ctx, both):
    """Two Jacobi sweeps, bit for bit.  Radius 2 and radius 3 share the bin edge 3 at 136 x 128 (68 x 64 bins of edge 2 are more
    than the index holds), so the second sweep launches the gather alone: the index of 17000 keypoints, more than 64 members per
    lane of its waves, stands."""
    kw = dict(min_support=4, max_rel_diff=0.1, strength=1.0, fill=1)
    pb = _object(gpu_ctx)
    try:
        _, _, res = ds.smooth_check(pb, tag="rounds", apply=1, radius=2, **kw)
        assert pb.smooth_stats()[0] == 2  # index, gather
        flags = np.concatenate([m["flags"] for m in res.values()])
        print("FIGURE smooth object rounds: bit for bit; classes (invalid, supported, filled, outlier) %s" % np.bincount(flags, minlength=4).tolist())
        assert {0, 1, 2} <= set(flags.tolist())  # (so dense that no keypoint lacks four neighbours)
        ds.smooth_check(pb, tag="rounds, second sweep", apply=1, radius=3, **kw)
        assert pb.smooth_stats()[0] == 1
    finally:
        pb.close()
    _same_bits_alone_and_again(lambda p: ds.smooth_run(p, level=0, radius=2, **kw), both, 40)


def test_carry(gpu_ctx):
    """Save both pairs, the next keyframe's lists of the same lengths through prepare_points, adopt: bit for bit; then pair 1 alone."""
    Ts = dc.rounds_poses()
    pb = _object(gpu_ctx)
    try:
        out_s, saved = ds.carry_save_check(pb, [0, 1], Ts, tag="rounds", **dc.SAVE)
        assert all(0 < s["num_carried"] < s["num_keypoints"] for s in saved.values())
        _fill(pb, which=1)
        out_a, arr, res = ds.carry_adopt_check(pb, [0, 1], saved, dc.SAVE["radius"], tag="rounds", apply=True, **dc.ADOPT)
        flags = np.concatenate([m["flags"] for m in res.values()])
        print("FIGURE carry  object rounds: bit for bit; flags (empty, adopted, sparse, range) %s" % np.bincount(flags, minlength=4).tolist())
        assert {1, 2} <= set(flags.tolist())
    finally:
        pb.close()
    one = _object(gpu_ctx, slice(1, 2))
    try:
        rc, s1 = one.carry_save([0], Ts[1:2], **dc.SAVE)
        assert rc == 0 and bytes(s1) == bytes(out_s)[24:48]
        _fill(one, slice(1, 2), which=1)
        t = ds.carry_arrays(one)
        rc, a1 = one.carry_adopt([0], apply=True, **t, **dc.ADOPT)
        assert rc == 0 and bytes(a1) == bytes(out_a)[32:64]
        assert all(v.cpu().numpy()[0].tobytes() == arr[k][1].tobytes() for k, v in t.items())
    finally:
        one.close()
