"""What mbavo_pairs_predict_hypotheses costs beside the calls it sits between, at 640 x 480 with 4 pyramid levels, on grid objects
(cell 30) and on every_candidate = 1 objects, costs taken at the coarsest level.  Inside one process, interleaved, `reps`
repetitions each after a warm-up, every repetition between two device synchronisations; min / median / max:
  predict   mbavo_pairs_predict, the call this one replaces
  hyp M     mbavo_pairs_predict_hypotheses with M = 1, 4, 8, 16 and the records (scales 0, 0.5, 2, -1, .. and small rotations)
  host M    the same call without records: the time until it returns, nothing waited for -- the host's share (the checks, the two
            copies, the B * M entry list and the engine's layout for it)
  eval M    the call's evaluation alone: mbavo_eval_batch(with_hessian = 0) on B * M copies of the coarsest entries
  lm        mbavo_lm_batch_levels on the object's array (3 iterations per level) behind a predict, the call that follows
`kernels M` = hyp M - eval M is the two new kernels with the copies and the synchronisation (they are not timed apart: that takes a
profiler run); `share M` = hyp M / (hyp M + lm), the call's share of predict + alignment.  Records, not gates.
Usage: python tools/pairs_hyp_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r27_pairs_hyp.txt), one JSON line per B at its end"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pairs_undistort_bench import H, L_LEVELS, THRESH, W, inputs, mmm, timed

MS = (1, 4, 8, 16)
# the default set of INTEGRATION.md first, then more of the same kind up to 15 challengers
SCALES = [0.0, 0.5, 2.0, -1.0] + [1.0] * 6 + [1.5, 0.25, -0.5, 3.0, 0.75]
ROT = 0.01
TWISTS = [None] * 4 + [(0, 0, 0, s * ROT if a == 0 else 0, s * ROT if a == 1 else 0, s * ROT if a == 2 else 0) for a in range(3) for s in (1, -1)] + [None] * 5


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import capi, workloads
    lib, k, N = ctx.lib, 2, 2
    sharp, blur, z = inputs(B)
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, k = %d, costs at level %d, min / median / max of %d, interleaved:" % (B, L_LEVELS, W, H, k, L_LEVELS - 1, reps))
    o = capi.LmBatchOpts()
    o.spline_deg_k, o.max_num_iterations, o.max_consecutive_nonmonotonic_steps = k, 3, 5
    o.min_step_quality, o.min_abs_cost_decrease, o.max_chi_square_error = 0.5, 1e-3, 3.0
    E = lib.mbavo_packed_len(k)
    for dense in (False, True):
        pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=k, N=N, cell=30, thresh=THRESH, every_candidate=dense)
        counts = pb.prepare(sharp, z, blur)
        states = pb.initial_states(0.0, 0.1)
        for st in states:  # (a velocity, so that the hypotheses differ)
            st.velocity[:] = [0.3, -0.2, 0.05, 0.02, -0.03, 0.01]
        cap, exp = np.full(B, 0.05), np.full(B, 0.02)
        res = (capi.LmBatchResult * B)()
        lvl = L_LEVELS - 1

        def fresh():
            assert pb.set_states(states) == 0

        fresh()
        assert pb.predict(cap, exp) == 0
        # B * M copies of the coarsest entries once the predict has published t0 and dt (the knots: the pair's own -- the evaluation costs the same)
        arrs = {}
        for M in MS:
            arr = (capi.Problem * (B * M))()
            for b in range(B):
                for m in range(M):
                    C.memmove(C.byref(arr[b * M + m]), C.byref(pb.array[b * pb.L + lvl]), C.sizeof(capi.Problem))
            arrs[M] = arr
        fb = torch.zeros(B * 16 * E, dtype=torch.float64, device="cuda:0")
        ev = torch.zeros(B * 16, dtype=torch.float64, device="cuda:0")
        t = {"predict": [], "lm": []}
        for M in MS:
            t["hyp %d" % M], t["host %d" % M], t["eval %d" % M] = [], [], []
        lm = lambda: capi.check(lib.mbavo_lm_batch_levels(ctx.handle, B, L_LEVELS, pb.array, C.byref(o), res, None, 0), "lm")
        winners = {}
        for rep in range(reps + 2):
            row = {}
            fresh()
            row["predict"] = timed(lambda: capi.check(pb.predict(cap, exp), "predict"))
            row["lm"] = timed(lm)
            for M in MS:
                hyp = lambda want: capi.check(pb.predict_hypotheses(cap, exp, SCALES[:M - 1], TWISTS[:M - 1], level=lvl, want_records=want)[0], "hyp")
                fresh()
                row["hyp %d" % M] = timed(lambda: hyp(True))
                fresh()
                import time
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hyp(False)
                row["host %d" % M] = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize()
                row["eval %d" % M] = timed(lambda: capi.check(lib.mbavo_eval_batch(ctx.handle, B * M, arrs[M], k, 0, fb.data_ptr(), None, ev.data_ptr()), "eval"))
            if rep >= 2:
                for key, v in row.items():
                    t[key].append(v)
        for M in MS:
            fresh()
            rc, rec = pb.predict_hypotheses(cap, exp, SCALES[:M - 1], TWISTS[:M - 1], level=lvl)
            winners[M] = (sorted(set(r.winner for r in rec)), pb.hyp_stats())
        med = {key: statistics.median(v) for key, v in t.items()}
        name = "every candidate" if dense else "grid"
        r = {key: mmm(v) for key, v in t.items()}
        r["K_level_mean"] = float(counts[:, lvl].mean())
        emit("  %-15s K at level %d: %.0f;  predict %s  lm %s ms" % (name, lvl, r["K_level_mean"], r["predict"], r["lm"]))
        for M in MS:
            r["kernels %d" % M] = round(med["hyp %d" % M] - med["eval %d" % M], 3)
            r["share %d" % M] = round(med["hyp %d" % M] / (med["hyp %d" % M] + med["lm"]), 4)
            r["stats %d" % M] = winners[M][1]
            emit("    M = %2d: call %s  (returns after %s; evaluation alone %s; kernels + copies + sync %.3f) ms; %.1f %% of call + lm; stats %s; winners %s"
                 % (M, r["hyp %d" % M], r["host %d" % M], r["eval %d" % M], r["kernels %d" % M], 100 * r["share %d" % M], winners[M][1], winners[M][0]))
        out["routes"][name] = r
        pb.close()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r27_pairs_hyp.txt")
    Bs = [int(a) for a in rest] or [64, 512]
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    text = []

    def emit(line):
        print(line)
        sys.stdout.flush()
        text.append(line)

    results = [bench(ctx, B, emit) for B in Bs]
    for r in results:
        emit(json.dumps(r))
    with open(out_path, "w") as f:
        f.write("\n".join(text) + "\n")
    ctx.close()
