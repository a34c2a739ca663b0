"""The one-camera prepare of a batch of keyframe pairs (mbavo_pairs_opts.undistort = 1, mbavo_pairs_set_camera) under two builds of
the library, interleaved inside one process: every repetition times one mbavo_pairs_prepare of each library in turn, between two
device synchronisations.  For a change that must leave that route alone: the libraries are the parent commit's and this one's, as
tools/ab_build.sh lays variants out (tools/_ab/libmbavo_<name>.so; here the two are whole builds of the two commits, e.g. a
`git worktree` of the parent built with mba-vo_amd/build.sh).  Both are loaded by path through plain ctypes with only the entry
points both have, so neither needs the other's binding.  640 x 480 x 4 levels, grid selection, the inputs and the camera of
tools/pairs_undistort_bench.py.
Usage: python tools/pairs_cameras_ab.py tools/_ab/libmbavo_parent.so tools/_ab/libmbavo_this.so [B ...] [OUT.txt]  (default 64 512)
   -> appended to OUT.txt (a last argument that is no number; default profiles/r19_pairs_cameras.txt), one JSON line per B"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from pairs_undistort_bench import DIST, H, INTR, L_LEVELS, THRESH, W, inputs, mmm, timed


class Build:
    """One library, one context, one B-pair object with the one camera set."""

    def __init__(self, path, B, stream):
        from mba_vo_amd import capi, synth, workloads
        vp = C.c_void_p
        self.lib = lib = C.CDLL(os.path.abspath(path))
        lib.mbavo_create.argtypes = [C.POINTER(vp), C.c_int]
        lib.mbavo_set_stream.argtypes = [vp, vp]
        lib.mbavo_destroy.argtypes = [vp]
        lib.mbavo_pairs_create.argtypes = [vp, C.POINTER(capi.PairsOpts), C.POINTER(vp)]
        lib.mbavo_pairs_set_camera.argtypes = [vp, C.POINTER(capi.CameraRadTan)]
        lib.mbavo_pairs_prepare.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int)]
        self.ctx, self.pairs, self.B = vp(), vp(), B
        assert lib.mbavo_create(C.byref(self.ctx), 0) == 0 and lib.mbavo_set_stream(self.ctx, vp(stream)) == 0
        self.pat = np.ascontiguousarray(synth.PATTERN8, dtype=np.int32)
        o = capi.PairsOpts()
        o.B, o.L, o.H, o.W, o.spline_deg_k, o.N = B, L_LEVELS, H, W, 4, 4
        for l in range(L_LEVELS):
            o.S[l], o.P[l], o.border[l] = 8, self.pat.size // 2, max(4, 20 >> l)
            o.pattern_xy[l] = self.pat.ctypes.data_as(capi.c_ip)
        for i in range(4):
            o.intrinsics[i] = INTR[i]
        o.huber_a, o.score_threshold, o.cell_H, o.cell_W, o.undistort = 10.0, THRESH, 30, 30, 1
        assert lib.mbavo_pairs_create(self.ctx, C.byref(o), C.byref(self.pairs)) == 0
        cam = workloads.camera_radtan(H, W, INTR, DIST)
        assert lib.mbavo_pairs_set_camera(self.pairs, C.byref(cam)) == 0
        self.counts = np.zeros((B, L_LEVELS), np.int32)

    def prepare(self, sharp, z, blur):
        rc = self.lib.mbavo_pairs_prepare(self.pairs, sharp.data_ptr(), z.data_ptr(), blur.data_ptr(), self.counts.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == 0, rc

    def close(self):
        self.lib.mbavo_destroy(self.ctx)


def bench(paths, B, stream, reps=10):
    sharp, blur, z = inputs(B)
    builds = {os.path.basename(p)[len("libmbavo_"):-len(".so")]: Build(p, B, stream) for p in paths}
    ts = {n: [] for n in builds}
    for b in builds.values():  # warm-up
        b.prepare(sharp, z, blur)
    for _ in range(reps):
        for n, b in builds.items():
            ts[n].append(timed(lambda: b.prepare(sharp, z, blur)))
    names = list(builds)
    med = {n: statistics.median(v) for n, v in ts.items()}
    out = {"legacy_ab": names, "B": B, "reps": reps, "counts_equal": bool(np.array_equal(builds[names[0]].counts, builds[names[1]].counts)),
           "second_minus_first_median_ms": round(med[names[1]] - med[names[0]], 3), "spread_ms": {n: round(max(v) - min(v), 3) for n, v in ts.items()}}
    out.update({"%s_min_med_max_ms" % n: mmm(v) for n, v in ts.items()})
    lines = ["one-camera prepare (undistort = 1), B = %d, two builds of the library interleaved in one process, min / median / max of %d:" % (B, reps)]
    for n in names:
        lines.append("  %-8s %9.3f / %9.3f / %9.3f ms   spread %.3f ms" % ((n,) + tuple(out["%s_min_med_max_ms" % n]) + (out["spread_ms"][n],)))
    lines.append("  medians: %s - %s = %.3f ms; keypoint counts equal: %s" % (names[1], names[0], med[names[1]] - med[names[0]], out["counts_equal"]))
    for b in builds.values():
        b.close()
    return lines + [json.dumps(out)]


if __name__ == "__main__":
    import torch
    paths, rest = sys.argv[1:3], sys.argv[3:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r19_pairs_cameras.txt")
    Bs = [int(a) for a in rest] or [64, 512]
    stream = torch.cuda.current_stream().cuda_stream
    text = []
    for B in Bs:
        for line in bench(paths, B, stream):
            print(line)
            sys.stdout.flush()
            text.append(line)
    with open(out_path, "a") as f:
        f.write("\n".join(text) + "\n")
