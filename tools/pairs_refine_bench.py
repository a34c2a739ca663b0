"""What mbavo_pairs_refine_depths costs beside the calls it sits between, at 640 x 480 with 4 pyramid levels, on grid objects (cell 30)
and on every_candidate = 1 objects.  Inside one process, interleaved, `reps` repetitions each after a warm-up, every repetition
between two device synchronisations; min / median / max:
  lm            mbavo_lm_batch_levels on the object's array (3 iterations per level), the knots reset to the same start before each
  refine0       mbavo_pairs_refine_depths(level = 0, apply = 0) with the four per-keypoint arrays and the records
  refine0_norec the same without records (nothing waited for inside the call)
  refine_all    level = -1 with records;  refine_all_norec: without
  commit        mbavo_pairs_commit (behind a predict each time: a commit consumes one)
`share` = refine_all / (lm + refine_all + commit), the call's share of a tracked frame behind its update.  Records, not gates.
Usage: python tools/pairs_refine_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r30_pairs_refine.txt): what the file holds above the line
   "# ---- times" is kept, the times and one JSON line per B follow it"""
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

MARK = "# ---- times"
ROUTES = ("lm", "refine0", "refine0_norec", "refine_all", "refine_all_norec", "commit")


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import capi, workloads
    lib, k, N = ctx.lib, 2, 2
    sharp, blur, z = inputs(B)
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, k = %d, S = 8, P = 8, min / median / max of %d in ms, interleaved:" % (B, L_LEVELS, W, H, k, reps))
    o = capi.LmBatchOpts()
    o.spline_deg_k, o.max_num_iterations, o.max_consecutive_nonmonotonic_steps = k, 3, 5
    o.min_step_quality, o.min_abs_cost_decrease, o.max_chi_square_error = 0.5, 1e-3, 3.0
    for dense in (False, True):
        pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=k, N=N, cell=30, thresh=THRESH, every_candidate=dense)
        counts = pb.prepare(sharp, z, blur)
        states = pb.initial_states(0.0, 0.1)
        cap, exp = np.full(B, 0.05), np.full(B, 0.02)
        caps = pb.capacities()
        mk = lambda n, dt: torch.zeros((B, n), dtype=dt, device="cuda:0")
        a0 = dict(g=mk(caps[0], torch.float64), h=mk(caps[0], torch.float64), cost=mk(caps[0], torch.float64), valid=mk(caps[0], torch.int32))
        aa = {key: mk(sum(caps), v.dtype) for key, v in a0.items()}
        res = (capi.LmBatchResult * B)()

        def start():
            assert pb.set_states(states) == 0 and pb.predict(cap, exp) == 0

        def refine(level, arrays, rec):
            rc, _ = pb.refine_depths(level=level, want_records=rec, **arrays)
            assert rc == 0, rc

        calls = {"lm": lambda: capi.check(lib.mbavo_lm_batch_levels(ctx.handle, B, L_LEVELS, pb.array, C.byref(o), res, None, 0), "lm"),
                 "refine0": lambda: refine(0, a0, True), "refine0_norec": lambda: refine(0, a0, False),
                 "refine_all": lambda: refine(-1, aa, True), "refine_all_norec": lambda: refine(-1, aa, False),
                 "commit": lambda: pb.commit(1.0, 2.0, 1.0)}
        t = {key: [] for key in ROUTES}
        for rep in range(reps + 2):
            start()
            for key in ROUTES:
                v = timed(calls[key])
                if rep >= 2:
                    t[key].append(v)
        start()
        rc, rec = pb.refine_depths(level=-1)
        med = {key: statistics.median(v) for key, v in t.items()}
        name = "every candidate" if dense else "grid"
        r = {key: mmm(v) for key, v in t.items()}
        r.update(share=round(med["refine_all"] / (med["lm"] + med["refine_all"] + med["commit"]), 4), K0_mean=float(counts[:, 0].mean()),
                 stats=pb.refine_stats(), full_share=float(sum(x.num_full for x in rec)) / max(1.0, float(sum(x.num_keypoints for x in rec))))
        out["routes"][name] = r
        emit("  %-15s K0 %.0f: lm %s  level 0 %s (no records %s)  all levels %s (no records %s)  commit %s; share of the frame %.1f %%; stats %s; %.2f of the keypoints full"
             % (name, r["K0_mean"], r["lm"], r["refine0"], r["refine0_norec"], r["refine_all"], r["refine_all_norec"], r["commit"], 100 * r["share"], r["stats"], r["full_share"]))
        pb.close()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r30_pairs_refine.txt")
    Bs = [int(a) for a in rest] or [64, 512]
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    head = open(out_path).read().split(MARK)[0] if os.path.exists(out_path) else ""
    text = []

    def emit(line):
        print(line)
        sys.stdout.flush()
        text.append(line)

    results = [bench(ctx, B, emit) for B in Bs]
    for r in results:
        emit(json.dumps(r))
    with open(out_path, "w") as f:
        f.write(head + MARK + " (python tools/pairs_refine_bench.py %s, one MI355X)\n" % " ".join(str(b) for b in Bs) + "\n".join(text) + "\n")
    ctx.close()
