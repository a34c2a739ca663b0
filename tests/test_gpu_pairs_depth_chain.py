"""The depth stages of a pairs batch back to back: refine, filter, search, smooth, carry_save, the update of the listed pairs,
carry_adopt, and the same six again with other option values; then every stage called TWICE in a row with different options behind
queued device work.  Every stage's call goes through one scratch type (pairs_prep.h: DepthCall), whose pinned mirror the stage's
next call overwrites once the previous upload has left it.

Chain A takes no records, so no stage call waits for the stream (the update between save and adopt does: it reads the counts
back); chain B, on an identically prepared object, takes the records of every call and so waits after each.  What both leave
behind -- the records of a final filter_depths(apply = 0) and every keypoint depth -- must be the same bits.

The twice-in-a-row part is what holds the wait in DepthCall::open: a few dozen milliseconds of matrix products are queued on the
stream first, so the first call's upload has not run when the second call fills the same mirror; without the wait the first launch
would read the second call's options (and seed words, bin edges, pair list) and chain A would differ from chain B.  The hand-over's
two calls share one scratch, so there the pair is carry_save, carry_adopt.

The object: every_candidate = 1 at 32 x 24, B = 3, L = 2 -- capacities 768 and 192, so a (pair, level 0) is shared by several
workgroups (3 of 256 keypoints, 6 of the evaluation's 128) and its keypoints fill more than one tile, while level 1 has one tile of
256; pair 1's exposure lies off its knots (its knots start long after its frame: tests/test_gpu_pairs_filter.py's construction)."""

import numpy as np
import pytest

import pairs_cases
import pairs_device as dv
import pairs_refine_scene as sc

pytestmark = pytest.mark.gpu

B, L, H, W = 3, 2, 24, 32
LISTED = [0, 2]
_Q = np.array([0.004, -0.006, 0.003, 1.0])
POSE = np.concatenate([[0.02, -0.01, 0.03], _Q / np.linalg.norm(_Q)])
ROUNDS = (
    dict(refine=dict(level=-1, apply=True, max_rel_step=0.1), filter=dict(level=-1, apply=True, sigma_i=2.0, prior_rel_sigma=0.05),
         search=dict(num_candidates=9, rho_lo=0.9, rho_hi=1.1, level=-1, apply=True, relative=True),
         smooth=dict(radius=2, min_support=2, max_rel_diff=0.2, level=-1, apply=True, fill=True, sync_filter=True, weights=1),
         save=dict(radius=2, deflate=0.8, weights=1), adopt=dict(min_support=1, max_rel_diff=0.1, apply=True, seed_filter=True, prior_rel_sigma=0.05)),
    dict(refine=dict(level=0, apply=True, max_rel_step=0.3, min_info=1e-3), filter=dict(level=-1, apply=True, sigma_i=1.0, prior_rel_sigma=0.1, gate_chi2=9.0),
         search=dict(num_candidates=5, rho_lo=0.8, rho_hi=1.25, level=1, apply=True, relative=True, min_ratio=1.0),
         smooth=dict(radius=3, min_support=1, max_rel_diff=0.1, strength=0.5, level=-1, apply=True),
         save=dict(radius=3, deflate=0.5), adopt=dict(min_support=2, max_rel_diff=0.3, apply=True, z_min=0.5, z_max=50.0)),
)
# launches of (refine, filter, search, smooth, carry_save, carry_adopt): the smoothing builds its index in both rounds -- first use,
# then new keypoints in the listed pairs and another bin edge
LAUNCHES = (1, 1, 1, 2, 2, 1)


@pytest.fixture(scope="module")
def inputs():
    sharp, _, blur = pairs_cases.inputs(B, H, W, seed=4, special=False)
    rng = np.random.default_rng(11)
    depth = rng.uniform(1.5, 3.0, (B, H, W)).astype(np.float32)
    new_sharp = np.ascontiguousarray(np.roll(sharp[LISTED], (2, 3), (1, 2)))
    new_depth = rng.uniform(1.5, 3.0, (len(LISTED), H, W)).astype(np.float32)
    return dv.dev(sharp, depth, blur, new_sharp, new_depth)


def _prepared(mbavo, ctx, inputs):
    from mba_vo_amd import workloads
    sharp, depth, blur = inputs[:3]
    pb = workloads.PairBatch(ctx, B, L=L, H=H, W=W, S=sc.S, k=sc.K_DEG, N=sc.N, cell=0, thresh=0.5, border=0, every_candidate=True)
    counts = pb.prepare(sharp, depth, blur)
    m = sc.motion()
    assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
    states = (mbavo.capi.VoState * B)()
    for b, st in enumerate(states):  # the same knots and times through the state; pair 1's knots start long after its frame
        st.t0, st.dt, st.N, st.is_first = (100.0 if b == 1 else float(m["t0"][b])), m["dt"], sc.N, 0
        st.knots_t[:3 * sc.N] = list(m["kt"][b].ravel())
        st.knots_R[:4 * sc.N] = list(m["kR"][b].ravel())
        st.T_keyframe[6] = st.T_prev_b2w[6] = 1.0
    assert pb.set_states(states) == 0
    return pb, counts


def _queue_work():
    """A few dozen milliseconds of device work on the stream the object runs on, nothing waited for."""
    import torch
    x = torch.full((4096, 4096), 1.0 / 4096, dtype=torch.float32, device="cuda:0")
    for _ in range(24):
        x = x @ x


def _chain(pb, inputs, records):
    """Both rounds and the stages twice in a row, then (the records of a final filter call as bytes, every (pair, level)'s depths, the launches of every call)."""
    new_sharp, new_depth = inputs[3:]
    launches = []
    for o in ROUNDS:
        rc, _ = pb.refine_depths(want_records=records, **o["refine"])
        assert rc == 0, ("refine", rc)
        launches.append(pb.refine_stats()[0])
        rc, _ = pb.filter_depths(want_records=records, **o["filter"])
        assert rc == 0, ("filter", rc)
        launches.append(pb.filter_stats()[0])
        rc, _ = pb.search_depths(want_records=records, **o["search"])
        assert rc == 0, ("search", rc)
        launches.append(pb.search_stats()[0])
        rc, _ = pb.smooth_depths(want_records=records, **o["smooth"])
        assert rc == 0, ("smooth", rc)
        launches.append(pb.smooth_stats()[0])
        rc, _ = pb.carry_save(LISTED, np.tile(POSE, (len(LISTED), 1)), want_records=records, **o["save"])
        assert rc == 0, ("carry_save", rc)
        launches.append(pb.carry_stats()[0][0])
        pb.update(None, LISTED, new_sharp, new_depth)
        rc, _ = pb.carry_adopt(LISTED, want_records=records, **o["adopt"])
        assert rc == 0, ("carry_adopt", rc)
        launches.append(pb.carry_stats()[1][0])
    # every stage twice in a row behind queued work: the second call may fill the mirror only once the first upload has left it
    first, second = ROUNDS
    for name, a, b in (("refine", lambda: pb.refine_depths(want_records=records, **first["refine"]), lambda: pb.refine_depths(want_records=records, **second["refine"])),
                       ("filter", lambda: pb.filter_depths(want_records=records, **first["filter"]), lambda: pb.filter_depths(want_records=records, **second["filter"])),
                       ("search", lambda: pb.search_depths(want_records=records, **first["search"]), lambda: pb.search_depths(want_records=records, **second["search"])),
                       ("smooth", lambda: pb.smooth_depths(want_records=records, **first["smooth"]), lambda: pb.smooth_depths(want_records=records, **second["smooth"])),
                       ("carry", lambda: pb.carry_save(LISTED, np.tile(POSE, (len(LISTED), 1)), want_records=records, **first["save"]),
                        lambda: pb.carry_adopt(LISTED, want_records=records, **second["adopt"]))):
        _queue_work()
        for call in (a, b):
            rc, _ = call()
            assert rc == 0, (name, "twice", rc)
    rc, out = pb.filter_depths(level=-1, apply=False, sigma_i=2.0)
    assert rc == 0, ("final filter", rc)
    depths = [dv.peek(pb.array[e].d_kp_z, pb.array[e].K, np.float64) for e in range(B * L)]
    return bytes(out), [(r.status, r.num_keypoints, r.num_full, r.num_fused) for r in out], depths, launches


def test_chain_without_waiting_equals_chain_with_records(mbavo, gpu_ctx, inputs):
    a, counts_a = _prepared(mbavo, gpu_ctx, inputs)
    b, counts_b = _prepared(mbavo, gpu_ctx, inputs)
    try:
        assert np.array_equal(counts_a, counts_b)
        print("keypoints per (pair, level):", counts_a.tolist())
        assert counts_a[:, 0].min() > 256 and counts_a[:, 1].max() < 256 and counts_a[:, 1].min() > 0  # more than one tile / less than one
        rec_a, sum_a, z_a, launches_a = _chain(a, inputs, records=False)
        rec_b, sum_b, z_b, launches_b = _chain(b, inputs, records=True)
        print("final filter records (status, K, full, fused):", sum_a)
        print("launches:", launches_a)
        assert launches_a == list(LAUNCHES) * 2 and launches_b == launches_a
        assert sum_a[1 * L][0] == -2 and sum_a[0][0] == 0 and sum_a[0][2] > 0  # pair 1 off its knots; pair 0 evaluated
        assert rec_a == rec_b, (sum_a, sum_b)
        for e, (x, y) in enumerate(zip(z_a, z_b)):
            assert dv.same_bits(x, y), ("depths of entry", e)
    finally:
        a.close(); b.close()
