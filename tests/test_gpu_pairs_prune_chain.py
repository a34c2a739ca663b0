"""The prune between the depth stages of a pairs batch, back to back behind queued device work: search, filter, smooth (which writes the
class bytes), prune on those bytes, filter, carry_save -- the pattern of tests/test_gpu_pairs_depth_chain.py, whose object this is
(every_candidate = 1 at 32 x 24, B = 3, L = 2; pair 1's exposure off its knots).

Chain A takes no records, so nothing waits for the stream but the prune's own mandatory read-back of the counts; chain B, on an
identically prepared object, takes every call's records and so waits after each.  The prune's scratch is a DepthCall like the other
stages': a few dozen milliseconds of matrix products are queued first, and the prune is called twice in a row with other options,
so the second call may fill the pinned mirror only once the first upload has left it.  What both chains leave behind -- every
keypoint array, the filter's state, K, the records of a final filter_depths(apply = 0) -- must be the same bits."""
import numpy as np
import pytest

import pairs_cases
import pairs_device as dv
import pairs_prune_ref as pref
import pairs_refine_scene as sc

pytestmark = pytest.mark.gpu

B, L, H, W = 3, 2, 24, 32
LISTED = [0, 2]
_Q = np.array([0.004, -0.006, 0.003, 1.0])
POSE = np.concatenate([[0.02, -0.01, 0.03], _Q / np.linalg.norm(_Q)])


@pytest.fixture(scope="module")
def inputs():
    sharp, _, blur = pairs_cases.inputs(B, H, W, seed=4, special=False)
    depth = np.random.default_rng(11).uniform(1.5, 3.0, (B, H, W)).astype(np.float32)
    return dv.dev(sharp, depth, blur)


def _prepared(mbavo, ctx, inputs):
    from mba_vo_amd import workloads
    pb = workloads.PairBatch(ctx, B, L=L, H=H, W=W, S=sc.S, k=sc.K_DEG, N=sc.N, cell=0, thresh=0.5, border=0, every_candidate=True)
    counts = pb.prepare(*inputs)
    m = sc.motion()
    t0 = np.where(np.arange(B) == 1, 100.0, m["t0"])  # pair 1's knots start long after its frame
    assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
    states = (mbavo.capi.VoState * B)()
    for b, st in enumerate(states):
        st.t0, st.dt, st.N, st.is_first = float(t0[b]), m["dt"], sc.N, 0
        st.knots_t[:3 * sc.N] = list(m["kt"][b].ravel())
        st.knots_R[:4 * sc.N] = list(m["kR"][b].ravel())
        st.T_keyframe[6] = st.T_prev_b2w[6] = 1.0
    assert pb.set_states(states) == 0
    return pb, counts


def _queue_work():
    import torch
    x = torch.full((4096, 4096), 1.0 / 4096, dtype=torch.float32, device="cuda:0")
    for _ in range(24):
        x = x @ x


def _chain(pb, records):
    import torch
    cap = pb.capacities()
    flags = torch.full((B, sum(cap)), 77, dtype=torch.uint8, device="cuda:0")
    keep = torch.full((B, sum(cap)), 99, dtype=torch.uint8, device="cuda:0")
    stats = []
    _queue_work()
    rc, _ = pb.search_depths(9, 0.9, 1.1, level=-1, apply=True, relative=True, want_records=records)
    assert rc == 0, ("search", rc)
    rc, _ = pb.filter_depths(level=-1, apply=True, sigma_i=2.0, prior_rel_sigma=0.05, reset=1, want_records=records)
    assert rc == 0, ("filter", rc)
    rc, _ = pb.smooth_depths(2, min_support=3, max_rel_diff=0.05, level=-1, apply=True, flags=flags, want_records=records)
    assert rc == 0, ("smooth", rc)
    # twice in a row: a count of level 1 alone with other criteria, then the prune on the smoothing's bytes
    rc, _ = pb.prune_keypoints(LISTED, level=1, apply=False, check_depth=True, z_min=2.0, min_keep=7, want_records=records)
    assert rc == 0, ("prune count", rc)
    stats.append(pb.prune_stats())
    rc, out = pb.prune_keypoints(LISTED, level=-1, apply=True, flags=flags, drop_mask=(1 << 0) | (1 << 3), keep=keep, want_records=records)
    assert rc == 0, ("prune", rc)
    stats.append(pb.prune_stats())
    Ks = [pb.array[e].K for e in range(B * L)]  # (the host knows K when the call returns, records or not)
    rc, _ = pb.filter_depths(level=-1, apply=True, sigma_i=2.0, prior_rel_sigma=0.05, want_records=records)
    assert rc == 0, ("filter after", rc)
    rc, _ = pb.carry_save(LISTED, np.tile(POSE, (len(LISTED), 1)), 2, deflate=0.8, weights=1, want_records=records)
    assert rc == 0, ("carry_save", rc)
    rc, last = pb.filter_depths(level=-1, apply=False, sigma_i=2.0)
    assert rc == 0, ("final filter", rc)
    return dict(snap=pref.snapshot(pb), last=bytes(last), seeded=[r.seeded for r in last], Ks=Ks, keep=keep.cpu().numpy(), stats=stats,
                counts=pref.device_counts(pb))


def test_chain_without_waiting_equals_chain_with_records(mbavo, gpu_ctx, inputs):
    a, counts_a = _prepared(mbavo, gpu_ctx, inputs)
    b, counts_b = _prepared(mbavo, gpu_ctx, inputs)
    try:
        assert np.array_equal(counts_a, counts_b) and counts_a[:, 0].min() > 256  # more than one tile at level 0
        ra, rb = _chain(a, records=False), _chain(b, records=True)
        print("K before", counts_a.tolist(), "after", ra["Ks"], "seeded by the filters after the prune", ra["seeded"])
        n = len(LISTED)
        assert ra["stats"] == [(1, 0, 0), (1, 1, 4 * B * L + 32 * n * L)] and rb["stats"] == [(1, 1, 32 * n), (1, 1, 4 * B * L + 32 * n * L)]
        assert ra["Ks"] == rb["Ks"] == ra["counts"].ravel().tolist() and np.array_equal(ra["counts"], rb["counts"])
        assert ra["Ks"][2:4] == counts_a[1].tolist() and any(k < c for k, c in zip(ra["Ks"], counts_a.ravel()))  # pair 1 not listed; something went
        assert not any(ra["seeded"])  # the filter carried on from the moved state
        assert ra["last"] == rb["last"] and np.array_equal(ra["keep"], rb["keep"])
        cap = a.capacities()
        for p in range(B):
            for l in range(L):  # up to the count before the prune: what lies behind it was never written by either object
                K0, o = int(counts_a[p, l]), sum(cap[:l])
                x, y = ra["snap"]["ents"][(p, l)], rb["snap"]["ents"][(p, l)]
                assert x["K"] == y["K"] and dv.same_bits(x["xy"][:K0], y["xy"][:K0]) and dv.same_bits(x["z"][:K0], y["z"][:K0]), (p, l)
                for key in ra["snap"]["state"]:
                    assert np.array_equal(ra["snap"]["state"][key][p, o:o + K0].view(np.uint8), rb["snap"]["state"][key][p, o:o + K0].view(np.uint8)), (p, l, key)
    finally:
        a.close(); b.close()
