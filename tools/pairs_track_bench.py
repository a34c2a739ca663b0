"""The pose bookkeeping of a frame of B trackers (640 x 480, 4 pyramid levels), on the device against the route available without
it, inside one process, interleaved, `reps` repetitions each after a warm-up, every repetition ending in a device
synchronisation:
  (a) mbavo_pairs_predict + mbavo_pairs_commit (one launch each, one copy of B x 144 bytes, one synchronisation);
  (b) the same bookkeeping as a caller did it before: mbavo_pairs_get_knots, per pair the C ABI's pose algebra (mbavo_se3_exp,
      mbavo_spline_transform_by_right), mbavo_pairs_set_motion, mbavo_pairs_assess, then per pair mbavo_transform_inverse / _mul,
      mbavo_se3_log and, for a new keyframe, mbavo_spline_transform_to followed by a second mbavo_pairs_set_motion.  Driven from
      Python, so (b) INCLUDES the ctypes call overhead of its 5 .. 8 calls per pair; a C caller pays less.
  and the whole frame through mbavo_pairs_track_frame (update with new blurred frames, predict, mbavo_lm_batch_levels, commit).
Nothing is asserted about the times; the file reports what was seen.  Checks that (a) and (b) reach the same verdicts.
The output file has two sections: the timings, which this tool rewrites, and below the line "## measured bounds" the figures the
GPU tests print (tests/pairs_track.py says how they get there), which this tool keeps.
Usage: python tools/pairs_track_bench.py [B ...] [--out FILE]  (default 64 512 -> profiles/r12_pairs_track.txt)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

L_LEVELS, H, W, CELL, THRESH, N, K_DEG = 4, 480, 640, 30, 4.0, 4, 4
FLOW0, FLOW1, KERNEL = 2.5, 6.0, 3.0
DT, DT_FRAME, EXP = 0.5, 0.1, 0.04
BOUNDS_MARK = "## measured bounds"


def _stat(ts):
    return {"min_ms": round(min(ts), 3), "median_ms": round(statistics.median(ts), 3), "max_ms": round(max(ts), 3)}


def host_route(lib, capi, pb, st, cap, exp):
    """(b): one frame's bookkeeping with the knots read back and the C ABI's algebra per pair.  st: list of dicts(T_keyframe,
    T_prev, velocity, prev) the caller owns; returns the verdicts."""
    dp = capi.dp
    B = pb.B
    kt, kR = pb.knots()
    t0 = cap - 0.5 * exp
    dT = np.zeros(7)
    for b in range(B):
        s = st[b]
        s["dt_frame"] = cap[b] - s["prev"]
        vel = s["velocity"] * s["dt_frame"]
        lib.mbavo_se3_exp(dp(vel), dp(dT))
        q, t = np.ascontiguousarray(dT[3:]), np.ascontiguousarray(dT[:3])
        lib.mbavo_spline_transform_by_right(dp(kt[b]), dp(kR[b]), N, dp(q), dp(t))
    assert pb.set_motion(cap, exp, t0, DT, kt, kR) == 0
    out = pb.assess(FLOW0, FLOW1, KERNEL)
    Tpi, dTn, lg, Tn = np.zeros(7), np.zeros(7), np.zeros(6), np.zeros(7)
    ident_q, ident_t = np.array([0.0, 0, 0, 1]), np.zeros(3)
    moved = False
    for b in range(B):
        s, a = st[b], out[b]
        T = np.array(a.T)
        lib.mbavo_transform_inverse(dp(s["T_prev"]), dp(Tpi))
        lib.mbavo_transform_mul(dp(Tpi), dp(T), dp(dTn))
        lib.mbavo_se3_log(dp(dTn), dp(lg))
        s["velocity"] = lg / s["dt_frame"]
        s["T_prev"] = T
        if a.is_keyframe:
            lib.mbavo_transform_mul(dp(s["T_keyframe"]), dp(T), dp(Tn))
            s["T_keyframe"] = Tn.copy()
            lib.mbavo_spline_transform_to(K_DEG, float(t0[b]), DT, dp(kt[b]), dp(kR[b]), N, float(cap[b]), dp(ident_q), dp(ident_t))
            s["T_prev"] = np.array([0.0, 0, 0, 0, 0, 0, 1])
            moved = True
        s["prev"] = cap[b]
    if moved:
        assert pb.set_motion(cap, exp, t0, DT, kt, kR) == 0
    return [a.is_keyframe for a in out]


def bench(M, ctx, B, reps=10, seed=1):
    import torch
    from mba_vo_amd import synth, workloads
    capi, lib = M.capi, ctx.lib
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(seed)
    bases = [torch.from_numpy(synth.texture_image(H, W, seed=seed + i, octaves=(32, 16, 8, 4))).to(dev) for i in range(4)]

    def images(off):
        return torch.stack([torch.roll(bases[(b + off) % 4], ((7 * b + off) % H, (13 * b + 3 * off) % W), (0, 1)) for b in range(B)]).contiguous()

    sharp, blur = images(0), images(1)
    depth = (torch.rand((B, H, W), generator=g, device=dev) * 2.0 + 1.0).contiguous()
    rng = np.random.default_rng(seed)
    kt0, kR0 = np.zeros((B, N, 3)), np.zeros((B, N, 4))
    states = (capi.VoState * B)()
    for b, st in enumerate(states):
        s = (0.05, 0.4, 0.9, 1.6, 2.8)[b % 5]
        kt0[b], kR0[b] = synth.trajectory("harness", N, 0.012 * s, 0.02 * s)
        st.t0, st.dt, st.N, st.is_first, st.prev_timestamp = 0.0, DT, N, 0, 0.1
        st.knots_t[:3 * N], st.knots_R[:4 * N] = kt0[b].ravel().tolist(), kR0[b].ravel().tolist()
        st.T_keyframe[6] = st.T_prev_b2w[6] = 1.0
        st.velocity[:] = (np.r_[rng.normal(0, 0.05, 3), rng.normal(0, 0.03, 3)] * s).tolist()
    cap, exp = np.full(B, 0.1 + DT_FRAME), np.full(B, EXP)
    pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, k=K_DEG, N=N, cell=CELL, thresh=THRESH)
    o = capi.LmBatchOpts()
    o.spline_deg_k, o.max_num_iterations, o.max_consecutive_nonmonotonic_steps, o.solver_type = K_DEG, 30, 5, 0
    o.min_step_quality, o.min_abs_cost_decrease, o.max_chi_square_error = 0.5, 1e-3, 3.0
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps}

    def host_states():
        return [dict(T_keyframe=np.array(s.T_keyframe), T_prev=np.array(s.T_prev_b2w), velocity=np.array(s.velocity), prev=s.prev_timestamp) for s in states]

    def device_route():
        assert pb.set_states(states) == 0
        t = time.perf_counter()
        assert pb.predict(cap, exp) == 0
        fr = pb.commit(FLOW0, FLOW1, KERNEL)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), [f.a.is_keyframe for f in fr]

    def caller_route():
        assert pb.set_motion(cap, exp, np.zeros(B), DT, kt0, kR0) == 0
        st = host_states()
        t = time.perf_counter()
        v = host_route(lib, capi, pb, st, cap, exp)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), v

    def whole_frame():
        assert pb.set_states(states) == 0
        torch.cuda.synchronize()
        t = time.perf_counter()
        fr, _, res, _ = pb.track_frame(blur, cap, exp, o, (FLOW0, FLOW1, KERNEL))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), sum(r.iterations for r in res)

    try:
        pb.prepare(sharp, depth, blur)
        (_, vd), (_, vh), (_, iters) = device_route(), caller_route(), whole_frame()  # warm-up, all three
        out["verdicts_equal"], out["keyframes"], out["lm_iterations_per_frame"] = vd == vh, int(sum(vd)), int(iters)
        ta, tb, tf = [], [], []
        for _ in range(reps):
            for fn, ts in ((device_route, ta), (caller_route, tb), (whole_frame, tf)):
                torch.cuda.synchronize()
                ts.append(fn()[0])
        out["predict_commit"], out["caller_route"], out["track_frame"] = _stat(ta), _stat(tb), _stat(tf)
        out["track_stats"] = pb.track_stats()
    finally:
        pb.close()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "r12_pairs_track.txt")
    if "--out" in args:
        i = args.index("--out")
        path = args[i + 1]
        del args[i:i + 2]
    Bs = [int(a) for a in args] or [64, 512]
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    text, lines = ["(b) is driven from Python: its per-pair C ABI calls include ctypes call overhead."], []
    for B in Bs:
        r = bench(mbavo, ctx, B)
        lines.append(r)
        text.append("B = %d pairs, %d levels of %dx%d, %d repetitions each, interleaved; %d of %d verdicts 'keyframe' (both routes equal: %s):" % (
            B, r["L"], r["W"], r["H"], r["reps"], r["keyframes"], B, r["verdicts_equal"]))
        for name, key in (("(a) mbavo_pairs_predict + mbavo_pairs_commit", "predict_commit"),
                          ("(b) get_knots + per-pair C ABI algebra + set_motion + assess", "caller_route"),
                          ("whole frame, mbavo_pairs_track_frame (%d LM iterations over the batch)" % r["lm_iterations_per_frame"], "track_frame")):
            s = r[key]
            text.append("  %-72s min %9.3f ms  median %9.3f ms  max %9.3f ms" % (name, s["min_ms"], s["median_ms"], s["max_ms"]))
        text.append("  launches, synchronisations, D2H bytes of the last predict / commit: %s" % (list(r["track_stats"]),))
    text += [json.dumps(r) for r in lines]
    print("\n".join(text))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    # the file has a second section, the measured bounds of tests/pairs_track.py (copied by hand from the output of
    # `python -m pytest -m gpu -s tests/test_gpu_pairs_track.py`): everything from BOUNDS_MARK on is kept as it is
    kept = ""
    if os.path.exists(path):
        old = open(path).read()
        if BOUNDS_MARK in old:
            kept = old[old.index(BOUNDS_MARK):]
    open(path, "w").write("\n".join(text) + "\n" + ("\n" + kept if kept else ""))
    ctx.close()
