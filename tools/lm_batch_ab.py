"""The batched LM (mbavo_lm_batch, mbavo_lm_batch_levels) under two builds of the library, interleaved inside one process: every
repetition times one call of each library in turn, from the same initial knots, between two device synchronisations.  For a change
that must leave the loop's results and speed alone: the libraries are the parent commit's and this one's, laid out as
tools/ab_build.sh lays variants out (tools/_ab/libmbavo_<name>.so; here two whole builds, e.g. a `git worktree` of the parent built
with mba-vo_amd/build.sh).  Both are loaded by path through plain ctypes with only the entry points both have.  Inputs: the
rendered 640 x 480 pairs of tools/lm_bench.py (one level) and tools/lm_levels_bench.py (L = 4); default options, solver type 0,
10 iterations per level, min_abs_cost_decrease = 0 (every iteration runs), no trace.
Usage: python tools/lm_batch_ab.py tools/_ab/libmbavo_parent.so tools/_ab/libmbavo_this.so [CASE ...] [OUT.txt]
   CASE: batch64 batch512 levels64 (default: all three) -> appended to OUT.txt (a last argument that is no case; default
   profiles/r21_lm_batch_host.txt), a text block and one JSON line per case"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

CASES = {"batch64": (64, 1), "batch512": (512, 1), "levels64": (64, 4)}
ITERATIONS, REPS = 10, 10


class Build:
    """One library and one context of it on the given stream."""

    def __init__(self, path, stream):
        from mba_vo_amd import capi
        vp = C.c_void_p
        self.lib = lib = C.CDLL(os.path.abspath(path))
        lib.mbavo_create.argtypes = [C.POINTER(vp), C.c_int]
        lib.mbavo_set_stream.argtypes = [vp, vp]
        lib.mbavo_destroy.argtypes = [vp]
        lib.mbavo_lm_batch.argtypes = [vp, C.c_int, C.POINTER(capi.Problem), C.POINTER(capi.LmBatchOpts), C.POINTER(capi.LmBatchResult),
                                       C.POINTER(capi.TraceRec), C.c_int]
        lib.mbavo_lm_batch_levels.argtypes = [vp, C.c_int, C.c_int] + lib.mbavo_lm_batch.argtypes[2:]
        self.ctx = vp()
        assert lib.mbavo_create(C.byref(self.ctx), 0) == 0 and lib.mbavo_set_stream(self.ctx, vp(stream)) == 0

    def lm(self, B, L, array, opts, res):
        if L == 1:
            rc = self.lib.mbavo_lm_batch(self.ctx, B, array, C.byref(opts), res, None, 0)
        else:
            rc = self.lib.mbavo_lm_batch_levels(self.ctx, B, L, array, C.byref(opts), res, None, 0)
        assert rc == 0, rc

    def close(self):
        self.lib.mbavo_destroy(self.ctx)


def bench(paths, case, ctx, stream, reps=REPS):
    import torch
    from mba_vo_amd import capi, workloads
    B, L = CASES[case]
    if L == 1:
        data = workloads.RenderedPairBatch(ctx, B, S=8, k=4, seed=1)
    else:
        data = workloads.RenderedPairPyramids(ctx, B, L=L, S=8, k=4, seed=1)
    knots = lambda: [data.knots(b) for b in range(B)]
    o = capi.LmBatchOpts()
    o.spline_deg_k, o.max_num_iterations, o.max_consecutive_nonmonotonic_steps, o.solver_type = 4, ITERATIONS, 5, 0
    o.min_step_quality, o.min_abs_cost_decrease, o.max_chi_square_error = 0.5, 0.0, 3.0
    builds = {os.path.basename(p)[len("libmbavo_"):-len(".so")]: Build(p, stream) for p in paths}
    names = list(builds)
    res = {n: (capi.LmBatchResult * B)() for n in names}

    def call(n):
        data.reset_knots()  # (ends with a device synchronisation)
        t = time.perf_counter()
        builds[n].lm(B, L, data.array, o, res[n])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    final = {}
    for n in names:  # warm-up: arenas sized, layouts built; the bits each build leaves behind
        call(n)
        call(n)
        final[n] = (bytes(res[n]), b"".join(x.cpu().numpy().tobytes() for kn in knots() for x in kn))
    ts = {n: [] for n in names}
    for _ in range(reps):
        for n in names:
            ts[n].append(call(n))
    med = {n: statistics.median(v) for n, v in ts.items()}
    spread = {n: max(v) - min(v) for n, v in ts.items()}
    diff = med[names[1]] - med[names[0]]
    out = {"lm_batch_ab": names, "case": case, "B": B, "L": L, "iterations_per_level": ITERATIONS, "reps": reps,
           "rounds": int(max(r.iterations for r in res[names[0]])),
           "results_equal_bitwise": final[names[0]][0] == final[names[1]][0], "final_knots_equal_bitwise": final[names[0]][1] == final[names[1]][1],
           "second_minus_first_median_ms": round(diff, 4), "spread_ms": {n: round(spread[n], 4) for n in names},
           "within_first_builds_spread": bool(abs(diff) <= spread[names[0]])}
    out.update({"%s_min_med_max_ms" % n: [round(min(v), 4), round(med[n], 4), round(max(v), 4)] for n, v in ts.items()})
    lines = ["%s: B = %d pairs, L = %d, %d iterations per level, two builds of the library interleaved in one process, min / median / max of %d calls:"
             % (case, B, L, ITERATIONS, reps)]
    for n in names:
        lines.append("  %-8s %9.4f / %9.4f / %9.4f ms   spread %.4f ms" % ((n,) + tuple(out["%s_min_med_max_ms" % n]) + (spread[n],)))
    lines.append("  medians: %s - %s = %+.4f ms (%s the spread of %s); results equal bit for bit: %s, final knots: %s" % (
        names[1], names[0], diff, "within" if out["within_first_builds_spread"] else "OUTSIDE", names[0], out["results_equal_bitwise"],
        out["final_knots_equal_bitwise"]))
    for b in builds.values():
        b.close()
    return lines + [json.dumps(out)]


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    paths, rest = sys.argv[1:3], sys.argv[3:]
    out_path = rest.pop() if rest and rest[-1] not in CASES else os.path.join(ROOT, "profiles", "r21_lm_batch_host.txt")
    stream = torch.cuda.current_stream().cuda_stream
    ctx = mbavo.capi.Context(0, stream=stream)  # renders the inputs
    text = []
    for case in rest or list(CASES):
        for line in bench(paths, case, ctx, stream):
            print(line)
            sys.stdout.flush()
            text.append(line)
    with open(out_path, "a") as f:
        f.write("\n".join(text) + "\n")
