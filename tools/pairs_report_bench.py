"""What mbavo_pairs_report costs beside the calls it sits between, at 640 x 480 with 4 pyramid levels, on grid objects (cell 30) and
on every_candidate = 1 objects.  Inside one process, interleaved, `reps` repetitions each after a warm-up, every repetition between
two device synchronisations; min / median / max:
  lm        mbavo_lm_batch_levels on the object's array (3 iterations per level), the knots reset to the same start before each
  report    mbavo_pairs_report(chi = 3) with both optional arrays, at the knots the LM ended at
  eval      the report's evaluation alone: mbavo_eval_batch(with_hessian = 1) on the B level-0 entries
  commit    mbavo_pairs_commit (behind a predict each time: a commit consumes one)
`kernel` = report - eval is the new kernel with its copy and synchronisation; `share` = report / (lm + report + commit), the
report's share of a tracked frame behind its update.  Records, not gates.
Usage: python tools/pairs_report_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r24_pairs_report.txt), one JSON line per B at its end"""
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


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import capi, workloads
    lib, k, N = ctx.lib, 2, 2
    sharp, blur, z = inputs(B)
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, k = %d, min / median / max of %d, interleaved:" % (B, L_LEVELS, W, H, k, reps))
    o = capi.LmBatchOpts()
    o.spline_deg_k, o.max_num_iterations, o.max_consecutive_nonmonotonic_steps = k, 3, 5
    o.min_step_quality, o.min_abs_cost_decrease, o.max_chi_square_error = 0.5, 1e-3, 3.0
    for dense in (False, True):
        pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=k, N=N, cell=30, thresh=THRESH, every_candidate=dense)
        counts = pb.prepare(sharp, z, blur)
        states = pb.initial_states(0.0, 0.1)
        cap, exp = np.full(B, 0.05), np.full(B, 0.02)
        cells = (C.c_int * 8)()
        assert lib.mbavo_pairs_plan(C.byref(pb.opts), C.byref(C.c_longlong(0)), cells) == 0
        pc = torch.zeros((B, cells[0]), dtype=torch.float64, device="cuda:0")
        fl = torch.zeros((B, cells[0]), dtype=torch.uint8, device="cuda:0")
        arr = (capi.Problem * B)()
        E = lib.mbavo_packed_len(k)
        fb = torch.zeros(B * E, dtype=torch.float64, device="cuda:0")
        epc = torch.zeros(max(int(counts[:, 0].sum()), 1), dtype=torch.float64, device="cuda:0")
        ev = torch.zeros(B, dtype=torch.float64, device="cuda:0")
        res = (capi.LmBatchResult * B)()

        def start():
            assert pb.set_states(states) == 0 and pb.predict(cap, exp) == 0

        start()
        for b in range(B):  # (copied once the predict has published t0 and dt: before it the entries carry dt = 0)
            C.memmove(C.byref(arr[b]), C.byref(pb.array[b * pb.L]), C.sizeof(capi.Problem))
            assert arr[b].dt > 0
        lm = lambda: capi.check(lib.mbavo_lm_batch_levels(ctx.handle, B, L_LEVELS, pb.array, C.byref(o), res, None, 0), "lm")
        t = {"lm": [], "report": [], "eval": [], "commit": []}
        for rep in range(reps + 2):
            start()
            a = timed(lm)
            b_ = timed(lambda: pb.report(3.0, pc, fl))
            c = timed(lambda: capi.check(lib.mbavo_eval_batch(ctx.handle, B, arr, k, 1, fb.data_ptr(), epc.data_ptr(), ev.data_ptr()), "eval"))
            d = timed(lambda: pb.commit(1.0, 2.0, 1.0))
            if rep >= 2:
                for key, v in zip(("lm", "report", "eval", "commit"), (a, b_, c, d)):
                    t[key].append(v)
        rec = pb.report(3.0)
        med = {key: statistics.median(v) for key, v in t.items()}
        name = "every candidate" if dense else "grid"
        r = {key: mmm(v) for key, v in t.items()}
        r.update(kernel=round(med["report"] - med["eval"], 3), share=round(med["report"] / (med["lm"] + med["report"] + med["commit"]), 4),
                 K0_mean=float(counts[:, 0].mean()), stats=pb.report_stats(), flagged_mean=float(np.mean([rec[b].num_flagged for b in range(B)])),
                 reported=int(sum(rec[b].status == 0 for b in range(B))))
        out["routes"][name] = r
        emit("  %-15s K0 %.0f: lm %s  report %s  (eval %s, kernel + copy %.3f)  commit %s ms; share of the frame %.1f %%; stats %s; %d of %d reported, %.1f flagged per pair"
             % (name, r["K0_mean"], r["lm"], r["report"], r["eval"], r["kernel"], r["commit"], 100 * r["share"], r["stats"], r["reported"], B, r["flagged_mean"]))
        pb.close()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r24_pairs_report.txt")
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
