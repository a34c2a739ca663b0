"""What the GPU tests of mbavo_pairs_predict_hypotheses share (helper, no test in it): one call held to the ORACLE on the entries
rebuilt from the object's own device arrays (pairs_oracle.read_entry) with the restated candidate knots (tests/pairs_hyp_ref.py) and
to the restated selection rule; the launch rule of the engine's last evaluation; and, for the option-laden objects A - D of
tests/pairs_oracle.py, the tracker states, the times and the hypothesis sets of tests/test_gpu_pairs_hyp_options.py, which need no
device, so that tests/test_pairs_prune_hyp_options_inputs.py can assert with the oracle on the CPU what the GPU file rests on."""
import ctypes as C

import numpy as np

import pairs_hyp_ref as hr
import pairs_oracle as po


def launches_of_last_evaluation(ctx):
    """The rule mbavo_pairs_report_stats documents, on the engine's witnesses."""
    name = ctx.lib.mbavo_last_kernel(ctx.handle).decode()
    lay = (C.c_int * 8)()
    assert ctx.lib.mbavo_last_layout(ctx.handle, lay) == 0
    if name.startswith("k_fused_sp<") and name.endswith(",true>"):
        return 1
    return (0 if name.endswith(",true>") else 1) + (1 if lay[0] > 0 else 0) + 1


def check_scores(orc, mbavo, ctx, pb, states, cap, exp, opts, tag):
    """One call; every (b, m) against the oracle on the rebuilt entry; the record against the selection rule on the device's own
    numbers.  opts: dict(scales, twists, level, and optionally min_valid_frac, min_gain).  Returns (records, oracle (scores, valids,
    eligible, costs) per pair, candidates per pair)."""
    capi, lib = mbavo.capi, ctx.lib
    scales, twists, level = opts["scales"], opts["twists"], opts["level"]
    min_valid_frac, min_gain = opts.get("min_valid_frac", 0), opts.get("min_gain", 0)
    M = 1 + len(scales)
    rc, rec = pb.predict_hypotheses(cap, exp, scales, twists, level=level, min_valid_frac=min_valid_frac, min_gain=min_gain)
    assert rc == 0, (tag, rc)
    worst, oracle, cands = 0.0, [], []
    for b in range(pb.B):
        q = pb.array[b * pb.L + level]
        e = po.read_entry(capi, q, pb.k)
        assert e["cap"][0] == cap[b] and e["exp"][0] == exp[b] and e["t0"] == cap[b] - 0.5 * exp[b] and e["start"][0] == 0, (tag, b)
        cs = hr.candidates(lib, capi.dp, states[b], cap[b], scales, twists)
        scores, valids, elig, costs = hr.oracle_scores(orc, e, cs, min_valid_frac)
        r = rec[b]
        assert r.num_keypoints == e["K"] == q.K, (tag, b)
        for m in range(16):
            if m >= M:
                assert r.score[m] == 0.0 and r.valid[m] == 0.0, (tag, b, m)
                continue
            assert r.valid[m] == valids[m], (tag, b, m, r.valid[m], valids[m])
            if np.isnan(scores[m]):
                assert np.isnan(r.score[m]), (tag, b, m)
            else:
                rel = abs(r.score[m] - scores[m]) / max(abs(scores[m]), 1e-300)
                worst = max(worst, rel)
                assert rel <= hr.SCORE_REL, (tag, b, m, r.score[m], scores[m], rel)
        dev_elig = [hr.eligible(r.score[m], e["K"], e["P"], r.valid[m], min_valid_frac) for m in range(M)]
        assert (r.winner, r.status, r.num_eligible) == hr.winner([r.score[m] for m in range(M)], dev_elig, min_gain), (tag, b)
        oracle.append((scores, valids, elig, costs))
        cands.append(cs)
    print("hypotheses %s: M %d level %d, scores within %.3e of the oracle's (bound %.0e), winners %s"
          % (tag, M, level, worst, hr.SCORE_REL, [r.winner for r in rec]))
    return rec, oracle, cands


# ---------------------------------------------------------------------------------------------------------------- objects A - D
MS = (1, 3, 16)
DT_FRAME = 0.1
# the flung-out hypothesis: pairs_hyp_ref.WIN_TWISTS[5], ten kilometres along x
FLING = hr.WIN_TWISTS[hr.FLUNG - 1]
# per object the seed of the velocities and of the hypotheses: chosen on the CPU (tests/test_pairs_prune_hyp_options_inputs.py) so
# that on every level and pair the two best eligible scores are more than 1 % apart and some winner is not 0
SEEDS = dict(A=2, B=4, C=2, D=3)


def object_times(name):
    """(cap, exp) of the hypothesis calls on an object: its own motion's.  The predict starts every pair's spline at
    cap - exp / 2 with the states' knot spacing, so every blur sample lies on segment 0, which has its k knots on every object
    (samples_on_knots holds for every pair)."""
    m, o = po.inputs(name)["motion"], po.OBJECTS[name]
    assert float(m["exp"].max()) < m["dt"] and o["k"] <= o["N"]
    return np.ascontiguousarray(m["cap"]), np.ascontiguousarray(m["exp"])


def object_states(capi, name):
    """B tracker states on the object's own motion (tests/test_gpu_pairs_prune_chain.py: _prepared): its knots and knot spacing,
    identity keyframe and previous poses, the previous frame DT_FRAME before the capture time, and a velocity that is not zero --
    about a pixel per frame across the image at the objects' depths and focal lengths, in a direction of its own per pair."""
    o, m = po.OBJECTS[name], po.inputs(name)["motion"]
    rng = np.random.default_rng(5100 + SEEDS[name])
    B, N = o["B"], o["N"]
    states = (capi.VoState * B)()
    for b, st in enumerate(states):
        st.t0, st.dt, st.N, st.is_first = float(m["t0"][b]), float(m["dt"]), N, 0
        st.knots_t[:3 * N] = m["kt"][b].ravel().tolist()
        st.knots_R[:4 * N] = m["kR"][b].ravel().tolist()
        st.T_keyframe[6] = st.T_prev_b2w[6] = 1.0
        v, w = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
        v[2] *= 0.3
        w[2] *= 0.3
        st.velocity[:] = np.r_[0.25 * v / np.linalg.norm(v), 0.12 * w / np.linalg.norm(w)].tolist()
        st.prev_timestamp = float(m["cap"][b]) - DT_FRAME
    return states


def hypotheses(name, M):
    """(scales, twists, index of the flung-out hypothesis or None) of the M - 1 challengers: scales of either sign, twists in v, in w
    and in both, None among them; with M > 1 the last hypothesis is flung out of view."""
    if M == 1:
        return [], [], None
    rng = np.random.default_rng(5200 + 10 * SEEDS[name] + M)
    scales = rng.uniform(-1.5, 2.5, M - 1)
    scales[0] = 0.0
    twists = [np.r_[rng.normal(0, 0.02, 3), rng.normal(0, 0.01, 3)].tolist() for _ in range(M - 1)]
    twists[0] = None
    if M > 3:
        twists[1][:3] = [0.0] * 3
        twists[2][3:] = [0.0] * 3
    scales[M - 2], twists[M - 2] = 1.0, FLING
    return scales.tolist(), twists, M - 1


def host_entry(name, levels, b, level):
    """The read_entry-shaped dict of pair b's entry of `level` after a hypothesis call, from pairs_oracle.host_levels: the times
    as the predict publishes them (the knots are left to the caller)."""
    cap, exp = object_times(name)
    e = dict(levels[b][level])
    e.update(cap=cap[b:b + 1].copy(), exp=exp[b:b + 1].copy(), t0=float(cap[b] - 0.5 * exp[b]), start=np.zeros(1, np.int32), kt=None, kR=None)
    return e
