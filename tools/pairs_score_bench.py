"""What keypoints by corner strength cost (mbavo_pairs_set_detector), at 640 x 480 with 4 pyramid levels, for a grid-selection and
an every-candidate object.  Inside one process, interleaved, `reps` repetitions each after a warm-up, every repetition between two
device synchronisations; min / median / max:
  a parent   mbavo_pairs_prepare of the PARENT commit's library (tools/_ab/libmbavo_parent.so, a whole build of that commit, loaded
             by path through plain ctypes; left out where the file does not exist)
  a          the same object's prepare with score = 0 (after set_detector(NULL)): the default path of this library
  r1 r2 r3   the prepare with score = 1 at radius 1, 2, 3 (ONE launch more: k_pairs_score)
  s1 s2 s3   mbavo_corner_score_u8 of one 640 x 480 image at radius 1, 2, 3 (one launch)
The figure to judge by is r / a, the scored prepare against the plain prepare of the same library; a / a parent shows that the
default path did not slow down.  The camera and the images are those of tools/pairs_undistort_bench.py.  Records, not gates.
Usage: python tools/pairs_score_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r45_pairs_score.txt): what the file holds above the line
   "# ---- times" is kept, the times and one JSON line per B follow it"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pairs_photocal_bench import MARK, PARENT, ParentContext
from pairs_undistort_bench import H, INTR, L_LEVELS, THRESH, W, inputs, mmm, timed

SCORE_THR = 2.0


def make(ctx, B, dense):
    from mba_vo_amd import workloads
    return workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=2, N=2, intr=INTR, cell=30, thresh=THRESH, every_candidate=dense)


def bench(mbavo, ctx, parent, B, emit, reps=10):
    import torch
    sharp, blur, z = inputs(B)
    score = torch.empty(H * W, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "configs": {}}
    emit("B = %d pairs, %d levels of %dx%d, min / median / max of %d in ms, interleaved:" % (B, L_LEVELS, W, H, reps))
    for dense in (False, True):
        pb = make(ctx, B, dense)
        old = make(parent, B, dense) if parent else None
        state = {}

        def mode(r):
            def setup():
                if state.get("r") != r:
                    assert (pb.set_detector(1, r, SCORE_THR) if r else pb.set_detector(None)) == 0
                    state["r"] = r
            return setup

        def alone(r):
            return lambda: mbavo.capi.check(ctx.lib.mbavo_corner_score_u8(sharp.data_ptr(), H, W, r, score.data_ptr(), stream), "mbavo_corner_score_u8")

        routes = {"a": (mode(0), lambda: pb.prepare(sharp, z, blur))}
        launches, counts = {}, {}
        for r in (1, 2, 3):
            routes["r%d" % r] = (mode(r), lambda: pb.prepare(sharp, z, blur))
            routes["s%d" % r] = (None, alone(r))
        if old:
            routes["a parent"] = (None, lambda: old.prepare(sharp, z, blur))
        order = [key for key in ("a parent", "a", "r1", "r2", "r3", "s1", "s2", "s3") if key in routes]
        t = {key: [] for key in order}
        for rep in range(reps + 2):
            for key in order:
                setup, run = routes[key]
                if setup:
                    setup()
                v = timed(run)
                if rep >= 2:
                    t[key].append(v)
                if key in ("a", "r1", "r2", "r3"):
                    launches[key] = pb.stats()[0]
                    counts[key] = int(sum(pb.array[e].K for e in range(B * L_LEVELS)))
        med = {key: statistics.median(v) for key, v in t.items()}
        res = {key: mmm(v) for key, v in t.items()}
        res.update({"r%d_over_a" % r: round(med["r%d" % r] / med["a"], 3) for r in (1, 2, 3)})
        res.update(a_over_parent=round(med["a"] / med["a parent"], 3) if old else None, launches=launches, keypoints=counts,
                   bytes_held=pb.detector_stats()[2], plan_bytes=pb.stats()[3])
        name = "every candidate" if dense else "grid selection"
        out["configs"][name] = res
        emit("  %-16s %s | r / a %.3f %.3f %.3f, a / parent %s; launches %s; keypoints %s; score slices %d bytes beside %d of the plan"
             % (name, "  ".join("%s %s" % (key, res[key]) for key in order), res["r1_over_a"], res["r2_over_a"], res["r3_over_a"],
                "%.3f" % res["a_over_parent"] if old else "-", launches, counts, res["bytes_held"], res["plan_bytes"]))
        for o in (pb, old):
            if o:
                o.close()
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r45_pairs_score.txt")
    Bs = [int(a) for a in rest] or [64, 512]
    stream = torch.cuda.current_stream().cuda_stream
    ctx = mbavo.capi.Context(0, stream=stream)
    parent = ParentContext(PARENT, stream, mbavo.capi) if os.path.exists(PARENT) else None
    head = open(out_path).read().split(MARK)[0] if os.path.exists(out_path) else ""
    text = []

    def emit(line):
        print(line)
        sys.stdout.flush()
        text.append(line)

    results = [bench(mbavo, ctx, parent, B, emit) for B in Bs]
    for res in results:
        emit(json.dumps(res))
    with open(out_path, "w") as f:
        f.write(head + MARK + " (python tools/pairs_score_bench.py %s, one MI355X%s)\n" % (" ".join(str(b) for b in Bs), "" if parent else ", no parent library")
                + "\n".join(text) + "\n")
    if parent:
        parent.close()
    ctx.close()
