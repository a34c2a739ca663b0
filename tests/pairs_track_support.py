"""What the tracker's tests share (helper, no test in it): one pair's assessment held to the oracle's orc_is_keyframe on what the
device itself holds (tests/test_gpu_pairs_step.py, tests/test_gpu_pairs_track_options.py), mbavo_lm_batch_levels held to
pairs_oracle.oracle_lm_levels on the rebuilt entries (tests/test_gpu_pairs_oracle.py and the tracked frame of
tests/test_gpu_pairs_track_options.py), the predict and the commit held to the host algebra of tests/pairs_track.py; and, for the
option-laden objects A - D of tests/pairs_oracle.py, the thresholds, tracker states, times and second frames of
tests/test_gpu_pairs_track_options.py, which need no device, so that tests/test_pairs_track_options_inputs.py can assert with the
oracle on the CPU what the GPU file rests on.

Times.  mbavo_pairs_predict starts every pair's spline at cap - exp / 2, so after a predict the first blur sample lies on segment 0
whatever the capture time is, and the exposure alone decides how far the last one reaches.  Object A (k = 4, N = 5) therefore meets
its last admissible segment, idx == 1 == N - k, after a predict through the exposure EXP_LAST_SEGMENT_A (the frame's last sample
and the assessment's cap + exp / 2 lie on segment 1), and the range edge through EXP_PAST_THE_KNOTS_A (the last sample on segment
2).  The tracked frame of check 5 has the exposure EXP_TRACKED on every object (A's own): every sample of the frame lies on the
capture time's segment, as the LM's merge of a frame's block at that start index assumes, and far enough into it for every knot of
the segment to carry weight -- with the objects' 0.04 s the samples stay within 8 % of the segment's start, the last knot's basis
weight is below 1e-4 (k = 4) and the oracle's two builds end 1e+4 apart on D, while B accepts no step at all."""
import ctypes as C

import numpy as np

import pairs_device as dv
import pairs_oracle as po
import pairs_step as ps
import pairs_track as pt
import pairs_prune_support as psup

E_ARG, E_RANGE = -1, -2
CAP = 256  # trace records per pair

# ---- objects A - D: (flow_mag0, flow_mag1, max_blur_kernel_mag) per object, chosen on the CPU from the oracle's averages on
# pairs_oracle.host_levels under the objects' own motion (pairs_oracle.motion, seed 0: no other seed was needed) so that both verdicts
# occur within each object, every pair passes pairs_step.margin_ok, and all three outcomes of the test are taken: "moved and sharp"
# (flow > flow_mag0, kernel < max), "moved but blurred" (flow between the two, kernel >= max: no keyframe) and "moved far"
# (flow > flow_mag1).  The oracle's (avg_flow, avg_kernel) per pair:
#   A  (2.101, 1.129) (6.304, 2.148) (13.04, 3.244)          B  (0.890, 0.052) (0.669, 0.080) (0.951, 0.135) (1.965, 0.182)
#   C  (3.399, 0.106) (1.866, 0.203) (5.046, 0.314)          D  (1.525, 0.049) (1.344, 0.082) (2.810, 0.148)
MOTION_SEED = 0
THRESHOLDS = dict(A=(4.0, 10.0, 1.7), B=(0.8, 1.5, 0.1), C=(1.5, 4.5, 0.15), D=(1.0, 2.0, 0.06))
# seed of pairs_track.make_states per object: chosen on the CPU (tests/test_pairs_track_options_inputs.py) so that on the tracked
# frame the oracle and its contracted build take the same decisions on every pair and accepted and rejected steps both occur
# (and the two builds end within 3e-6 of each other in every knot: the device's 1e-5 is not asked of a frame the reference itself
# cannot place)
STATE_SEEDS = dict(A=1, B=4, C=4, D=9)
EXP_TRACKED = 0.35
EXP_LAST_SEGMENT_A = 0.7
EXP_PAST_THE_KNOTS_A = 1.0 + 1e-6
PRUNE_SEED = psup.SEED_ALL  # the keep patterns of check 4: pairs_prune_support.keep_patterns on every pair, min_keep 0


def motion_of(name):
    """The motion the tracker tests set: the object's own (seed MOTION_SEED)."""
    return po.inputs(name)["motion"] if MOTION_SEED == 0 else po.motion(po.OBJECTS[name], MOTION_SEED)


def frame_times(name, exp=None):
    """(cap, exp) of a predict on the object: its own motion's, or the given exposure on every pair."""
    m = motion_of(name)
    e = m["exp"] if exp is None else np.full(len(m["exp"]), float(exp))
    return np.ascontiguousarray(m["cap"], dtype=np.float64), np.ascontiguousarray(e, dtype=np.float64)


def algebra_times(name):
    """The frame of check 3: object A with the exposure that puts the last sample on idx == N - k, the others with their own."""
    return frame_times(name, EXP_LAST_SEGMENT_A if name == "A" else None)


def sample_indices(o, cap, exp, t0, dt):
    """Segment index of the S blur samples of one frame (the kernels' own sample times) and of cap, cap -/+ exp / 2."""
    S = o["S"]
    blur = [int(np.floor(((cap - exp * 0.5 + s * exp / (S - 1 + 1e-8)) - t0) / dt)) for s in range(S)]
    return blur, [int(np.floor((t - t0) / dt)) for t in (cap, cap - 0.5 * exp, cap + 0.5 * exp)]


def object_states(capi, name):
    """pairs_track.make_states on the object's N, dt and knots: random T_keyframe and T_prev_b2w, velocities scaled per pair, pair 1
    at rest, pair 2 with |omega| < 1e-10, the previous frame 0.1 s before the capture time.  (The predict's start time does not
    depend on the velocity: samples_on_knots passes for any.)"""
    o, m = po.OBJECTS[name], motion_of(name)
    case = dict(B=o["B"], kt=m["kt"], kR=m["kR"], t0=m["t0"], dt=m["dt"], cap=m["cap"])
    return pt.make_states(capi, case, seed=STATE_SEEDS[name])


def second_inputs(name):
    """The inputs of the tracked frame: pairs_oracle.second_frame where the object has one (B: new blurred frames and a new
    keyframe for pair 2); else the object's inputs under new blurred frames made the same way -- the keyframes shifted the other way,
    noised."""
    if name == "B":
        return po.second_frame(name)
    o, c = po.OBJECTS[name], dict(po.inputs(name))
    rng = np.random.default_rng(9100 + o["seed"])
    c["blur"] = np.ascontiguousarray(np.stack([np.clip(np.roll(s, (-1, 1), (0, 1)).astype(np.int32) + rng.integers(-4, 5, s.shape), 0, 255).astype(np.uint8)
                                               for s in c["sharp"]]))
    return c


def predicted_motion(lib, capi, name, states, cap, exp):
    """The motion a predict from `states` leaves, by the host algebra: a dict as pairs_oracle.motion makes them."""
    o = po.OBJECTS[name]
    want = [pt.host_predict(lib, capi.dp, states[b], cap[b], exp[b]) for b in range(o["B"])]
    return dict(cap=cap, exp=exp, t0=np.array([w[0] for w in want]), dt=float(states[0].dt),
                kt=np.ascontiguousarray(np.stack([w[1].reshape(o["N"], 3) for w in want])),
                kR=np.ascontiguousarray(np.stack([w[2].reshape(o["N"], 4) for w in want])))


def tracked_host_levels(lib, capi, name):
    """pairs_oracle.host_levels of the tracked frame: the second inputs under the motion the predict leaves."""
    cap, exp = frame_times(name, EXP_TRACKED)
    m = predicted_motion(lib, capi, name, object_states(capi, name), cap, exp)
    return po.host_levels(name, dict(second_inputs(name), motion=m))


def pruned_level0(name, levels=None):
    """Per pair (xy, z) of level 0 after the prune of check 4, from pairs_oracle.host_levels and the restatement."""
    import pairs_prune_ref as pref
    levels = po.host_levels(name) if levels is None else levels
    Ks = np.array([[e["K"] for e in pair] for pair in levels])
    keeps = psup.keep_patterns(Ks, PRUNE_SEED)
    cap = [int(Ks[:, l].max()) for l in range(Ks.shape[1])]
    flags = psup.flag_bytes(Ks.shape[0], cap, keeps, np.random.default_rng(PRUNE_SEED))
    out = []
    for b, pair in enumerate(levels):
        e = pair[0]
        want = pref.prune(e["K"], e["xy"], e["z"], None, flags=flags[b, :cap[0]], apply=1, drop_mask=psup.MASK)
        assert want["K"] == int(keeps[(b, 0)].sum())
        out.append((want["xy"][:want["K"]], want["z"][:want["K"]]))
    return out


# ---------------------------------------------------------------------------------------------------------------- the assessment
def pose(lib, capi, k, t0, dt, kt, kR, t):
    p, q = np.zeros(3), np.zeros(4)
    kt, kR = np.ascontiguousarray(kt).ravel(), np.ascontiguousarray(kR).ravel()
    rc = lib.mbavo_spline_get_pose(k, float(t0), float(dt), capi.dp(kt), capi.dp(kR), kR.size // 4, float(t), capi.dp(p), capi.dp(q), None, None)
    return rc, np.r_[p, q]


def keypoints0(pb, b):
    """The pair's level-0 keypoints, read back from entry b * L."""
    q = pb.array[b * pb.L]
    return dv.peek(q.d_kp_xy, 2 * q.K, np.float64).reshape(-1, 2), dv.peek(q.d_kp_z, q.K, np.float64)


def check_assessment(orc, mbavo, ctx, pb, a, b, k, t0, dt, cap, exp, intr, tag, need_margin=True, thresholds=(ps.FLOW0, ps.FLOW1, ps.KERNEL)):
    """One pair's assessment against the oracle on the pair's own knots and level-0 keypoints as the device holds them."""
    capi = mbavo.capi
    kt, kR = pb.knots()
    xy, z = keypoints0(pb, b)
    v, af, ak = ps.oracle_assess(orc, intr, xy, z, k, t0, dt, kt[b], kR[b], cap, exp, thresholds)
    print("assess %s pair %d: K %d flow %.9g / %.9g kernel %.9g / %.9g verdict %d / %d" % (tag, b, len(z), a.avg_flow, af, a.avg_kernel, ak, a.is_keyframe, v))
    assert a.status == 0 and a.num_keypoints0 == len(z), (tag, b)
    assert abs(a.avg_flow - af) <= ps.bound(af), (tag, b, a.avg_flow, af)
    assert abs(a.avg_kernel - ak) <= ps.bound(ak), (tag, b, a.avg_kernel, ak)
    if need_margin:
        assert ps.margin_ok(af, ak, thresholds=thresholds), (tag, b, af, ak)  # the inputs are fixed: no pair is left out
    if ps.margin_ok(af, ak, thresholds=thresholds):
        assert a.is_keyframe == v, (tag, b, af, ak)
    poses = []
    for t in (cap, cap - 0.5 * exp, cap + 0.5 * exp):
        rc, T = pose(ctx.lib, capi, k, t0, dt, kt[b], kR[b], t)
        assert rc == 0
        poses.append(T)
    assert np.abs(np.array(a.T) - poses[0]).max() <= 1e-12, (tag, b)
    return v, ps.count_behind(intr, xy, z, poses)


def check_object_assessment(orc, mbavo, ctx, pb, name, out, t0, cap, exp, counts0, tag, need_margin=True):
    """Every pair of an object's assessment `out` against the oracle under the pair's own level-0 intrinsics; counts0: the level-0
    counts the assessment must state.  Returns the oracle's verdicts."""
    o = po.OBJECTS[name]
    verdicts = []
    for b in range(o["B"]):
        v, behind = check_assessment(orc, mbavo, ctx, pb, out[b], b, o["k"], t0[b], pb.array[b * pb.L].dt, cap[b], exp[b], po.to_intr(o, b), tag,
                                     need_margin=need_margin, thresholds=THRESHOLDS[name])
        assert out[b].num_keypoints0 == counts0[b] == pb.array[b * pb.L].K, (tag, b, out[b].num_keypoints0, counts0[b])
        assert out[b].num_behind == behind, (tag, b, out[b].num_behind, behind)
        verdicts.append(v)
    return verdicts


# ---------------------------------------------------------------------------------------------------------------- predict and commit
def problem_times(pb):
    return [(pb.array[e].t0, pb.array[e].dt, pb.array[e].h_start_idx[0]) for e in range(pb.B * pb.L)]


def _worse(figures, name, got, want):
    d = float(np.abs(np.asarray(got, dtype=np.float64).ravel() - np.asarray(want, dtype=np.float64).ravel()).max())
    figures[name] = max(figures.get(name, 0.0), d)


def check_predict(mbavo, ctx, pb, states, cap, exp, figures, twin=None):
    """A predict from `states` (as set): the knots against pairs_track.host_predict into `figures`, the problems' t0 and start index
    equal to `twin`'s set_motion at the same times, nothing but the knots and t0 moved.  Returns (host predictions per pair, t0,
    knots_t, knots_R, the states after the predict)."""
    capi, lib = mbavo.capi, ctx.lib
    assert pb.predict(cap, exp) == 0
    gkt, gkR = pb.knots()
    want = [pt.host_predict(lib, capi.dp, states[b], cap[b], exp[b]) for b in range(pb.B)]
    for b in range(pb.B):
        _worse(figures, "predict_knots_t", gkt[b], want[b][1])
        _worse(figures, "predict_knots_R", gkR[b], want[b][2])
    t0 = np.array([w[0] for w in want])
    if twin is not None:
        assert twin.set_motion(cap, exp, t0, states[0].dt, gkt, gkR) == 0
        assert problem_times(pb) == problem_times(twin)
    after_predict = pb.get_states()
    for b in range(pb.B):  # the stored velocity is not scaled; nothing but the knots and t0 moved
        a, s = pt.state_arrays(after_predict[b]), pt.state_arrays(states[b])
        assert a["t0"] == t0[b] and a["dt"] == s["dt"] and a["prev_timestamp"] == s["prev_timestamp"], b
        assert all(np.array_equal(a[key], s[key]) for key in ("velocity", "T_prev", "T_keyframe")), b
        assert np.array_equal(a["kt"], gkt[b].ravel()) and np.array_equal(a["kR"], gkR[b].ravel()), b
    return want, t0, gkt, gkR, after_predict


def check_commit(mbavo, ctx, pb, k, after_predict, t0, kt, kR, dt_frames, ass, out, cap, figures):
    """A commit's frames `out` and the states behind it: the assessment the same bytes as `ass` (mbavo_pairs_assess just before),
    the knots bit for bit untouched where the verdict is 0, velocity, T_prev, T_keyframe, the knots and T_world against
    pairs_track.host_commit fed with the device's pose into `figures`, prev_timestamp == cap.  kt, kR: the knots before the commit.
    Returns the verdicts."""
    capi, lib = mbavo.capi, ctx.lib
    after = pb.get_states()
    verdicts = []
    for b in range(pb.B):
        assert bytes(out[b].a) == bytes(ass[b]), b
        assert ass[b].status == 0, (b, ass[b].status)
        v = ass[b].is_keyframe
        verdicts.append(v)
        h = pt.host_commit(lib, capi.dp, k, after_predict[b], t0[b], kt[b], kR[b], dt_frames[b], np.array(ass[b].T), v, cap[b])
        got = pt.state_arrays(after[b])
        if not v:
            assert np.array_equal(got["kt"], kt[b].ravel()) and np.array_equal(got["kR"], kR[b].ravel()), b
        for name, g, w in (("velocity", got["velocity"], h["velocity"]), ("T_prev", got["T_prev"], h["T_prev"]), ("T_keyframe", got["T_keyframe"], h["T_keyframe"]),
                           ("knots_t", got["kt"], h["kt"]), ("knots_R", got["kR"], h["kR"]), ("T_world", np.array(out[b].T_world), h["T_world"])):
            _worse(figures, name, g, w)
        assert got["prev_timestamp"] == cap[b] and got["t0"] == t0[b], b
    return verdicts


def assert_under_the_cap(figures, tag):
    """Every algebra figure against pairs_track.ALGEBRA_CAP, printed first."""
    print("FIGURE algebra %s: %s (cap %.0e)" % (tag, "  ".join("%s %.3e" % kv for kv in sorted(figures.items())), pt.ALGEBRA_CAP))
    for name, d in figures.items():
        assert d <= pt.ALGEBRA_CAP, (tag, name, d)


# ---------------------------------------------------------------------------------------------------------------- the LM
def rebuilt(orc, capi, pb, k):
    """[pair][level] (OrcProblem, keep) of the entries as they are now."""
    return [[po.oracle_problem(orc, capi, pb.array[b * pb.L + l], k) for l in range(pb.L)] for b in range(pb.B)]


def trace_tuples(trace, res, B, cap=CAP):
    out = []
    for b in range(B):
        assert 0 < res[b].num_trace <= cap
        out.append([(t.level, t.iter, t.kind, t.num_outliers, t.radius, t.eval_cost, t.candidate_cost, t.model_change, t.quality)
                    for t in trace[b * cap:b * cap + res[b].num_trace]])
    return out


def device_lm(mbavo, ctx, pb, k):
    import torch
    capi = mbavo.capi
    res, trace = (capi.LmBatchResult * pb.B)(), (capi.TraceRec * (pb.B * CAP))()
    o = po.lm_opts(capi, k)
    assert ctx.lib.mbavo_lm_batch_levels(ctx.handle, pb.B, pb.L, pb.array, C.byref(o), res, trace, CAP) == 0
    torch.cuda.synchronize()
    return trace_tuples(trace, res, pb.B), res


def _spread(a, f):
    cost = max(max(abs(x[i] - y[i]) / max(1.0, abs(x[i])) for i in (5, 6)) for x, y in zip(a["trace"], f["trace"]))
    return cost, max(float(np.abs(a["kt"] - f["kt"]).max()), float(np.abs(a["kR"] - f["kR"]).max()))


def check_lm(orc, mbavo, ctx, pb, name, tag, start=None, got_out=None):
    """mbavo_lm_batch_levels from the knots as they are against oracle_lm_levels on the rebuilt problems; returns the oracle's runs.
    start: the start index every entry must state (default: the object's own); got_out: a dict that receives the device's records
    and results."""
    o = po.OBJECTS[name]
    start = o["start"] if start is None else start
    entries = rebuilt(orc, mbavo.capi, pb, o["k"])
    want = [po.oracle_lm_levels(orc, pair) for pair in entries]
    fma = orc.fma_variant()
    spread = (0.0, 0.0)
    if fma is not None:  # the reference's own two roundings on the same inputs (tests/test_gpu_pairs_oracle.py: the module docstring)
        for b, pair in enumerate(entries):
            f = po.oracle_lm_levels(fma, [po.problem_of(fma, dict(keep[-1])) for _, keep in pair])
            assert [t[:4] for t in f["trace"]] == [t[:4] for t in want[b]["trace"]], (tag, b)
            spread = tuple(max(s, v) for s, v in zip(spread, _spread(want[b], f)))
    cost_bound, knot_bound = 1e-6, 1e-5  # DESIGN section 2, as stated
    got, res = device_lm(mbavo, ctx, pb, o["k"])
    if got_out is not None:
        got_out.update(records=got, res=res)
    kt, kR = pb.knots()
    worst_cost = worst_knot = 0.0
    for b in range(o["B"]):
        assert pb.array[b * o["L"]].h_start_idx[0] == entries[b][0][1][-1]["start"][0] == start, (tag, b)
        assert [t[:4] for t in got[b]] == [t[:4] for t in want[b]["trace"]], (tag, b, [t[:4] for t in got[b]], [t[:4] for t in want[b]["trace"]])
        for d, w in zip(got[b], want[b]["trace"]):
            for i in (5, 6):
                worst_cost = max(worst_cost, abs(d[i] - w[i]) / max(1.0, abs(w[i])))
        worst_cost = max(worst_cost, abs(res[b].final_cost - want[b]["cost"]) / max(1.0, abs(want[b]["cost"])))
        worst_knot = max(worst_knot, float(np.abs(kt[b] - want[b]["kt"]).max()), float(np.abs(kR[b] - want[b]["kR"]).max()))
        assert res[b].num_outliers == want[b]["trace"][-1][3], (tag, b)
    kinds = [t[2] for b in range(o["B"]) for t in got[b]]
    print("LM %s: costs %.3e = %.3f of 1e-6 (oracle against its FMA build: %.2e), knots %.3e = %.3f of 1e-5 (%.2e); accepted %d rejected %d"
          % (tag, worst_cost, worst_cost / cost_bound, spread[0], worst_knot, worst_knot / knot_bound, spread[1], kinds.count(1), kinds.count(2)))
    assert kinds.count(1) > 0 and kinds.count(2) > 0, tag
    assert worst_cost <= cost_bound, (tag, worst_cost, cost_bound)
    assert worst_knot <= knot_bound, (tag, worst_knot, knot_bound)
    return want
