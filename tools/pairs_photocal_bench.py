"""What the photometric calibration at intake costs (mbavo_pairs_set_photometric), at 640 x 480 with 4 pyramid levels, grid
selection, with undistort 0 and 1, with one camera and with G = 4 (pair b looks through camera b % 4).  Inside one process,
interleaved, `reps` repetitions each after a warm-up, every repetition between two device synchronisations; min / median / max:
  a parent   mbavo_pairs_prepare of the PARENT commit's library (tools/_ab/libmbavo_parent.so, a whole build of that commit, loaded
             by path through plain ctypes; left out where the file does not exist)
  a          mbavo_pairs_prepare of this library on an object without a calibration
  b          the calibrated prepare: a gamma-2.2 table per camera and a vignette map, the table staged in LDS
  b plain    the same with the table read by plain loads (a second object made under MBAVO_PAIRS_PHOTOCAL_LDS=0)
  b flag     the calibrated prepare after a call without a vignette: the object keeps a flag and reads no map
  b ones     the same calibration with a vignette of ones: what storing ones in place of the flag would cost
  c          (undistort 0 only) the caller-composed route: mbavo_photometric_u8_batch of the 2B images into a temporary, then (a).
             With raw images no correct composed route exists: the vignette lives in the raw geometry and the bilinear blend
             does not commute with the table, so a correction before or after the remap gives other bytes.
  e          mbavo_pairs_set_photometric itself (n tables and n vignette maps; nothing is waited for inside the call, the
             time includes the synchronisation behind it)
The camera and the images are those of tools/pairs_undistort_bench.py.  Records, not gates.
Usage: python tools/pairs_photocal_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r43_pairs_photocal.txt): what the file holds above the line
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

from pairs_undistort_bench import DIST, H, INTR, L_LEVELS, THRESH, W, inputs, mmm, timed

MARK = "# ---- times"
PARENT = os.path.join(ROOT, "tools", "_ab", "libmbavo_parent.so")
G_SET = 4


class ParentContext:
    """The parent commit's library behind the two attributes workloads.PairBatch reads of a context: only entry points both
    libraries have, with their argument types set here."""

    def __init__(self, path, stream, capi):
        vp = C.c_void_p
        self.lib = lib = C.CDLL(path)
        self.handle, self.device_id = vp(), 0
        lib.mbavo_create.argtypes = [C.POINTER(vp), C.c_int]
        lib.mbavo_set_stream.argtypes = [vp, vp]
        lib.mbavo_destroy.argtypes = [vp]
        lib.mbavo_pairs_create.argtypes = [vp, C.POINTER(capi.PairsOpts), C.POINTER(vp)]
        lib.mbavo_pairs_destroy.argtypes = [vp]
        lib.mbavo_pairs_problems.argtypes = [vp, C.POINTER(C.POINTER(capi.Problem)), C.POINTER(C.c_int)]
        lib.mbavo_pairs_set_camera.argtypes = [vp, C.POINTER(capi.CameraRadTan)]
        lib.mbavo_pairs_set_cameras.argtypes = [vp, C.c_int, C.POINTER(capi.PairsCamera), C.POINTER(C.c_int)]
        lib.mbavo_pairs_prepare.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int)]
        assert lib.mbavo_create(C.byref(self.handle), 0) == 0 and lib.mbavo_set_stream(self.handle, vp(stream)) == 0

    def close(self):
        self.lib.mbavo_destroy(self.handle)
        self.handle = C.c_void_p()


def make(ctx, B, undistort, G):
    from mba_vo_amd import workloads
    pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=2, N=2, intr=INTR, cell=30, thresh=THRESH, undistort=undistort, num_cameras=G)
    cam = workloads.camera_radtan(H, W, INTR, DIST)
    if G:
        assert pb.set_cameras([workloads.pairs_camera(cam, INTR)] * G, [b % G for b in range(B)]) == 0
    elif undistort:
        assert pb.set_camera(cam) == 0
    return pb


def bench(mbavo, ctx, parent, B, emit, reps=10):
    import torch
    from mba_vo_amd import workloads
    lib = ctx.lib
    sharp, blur, z = inputs(B)
    both = torch.cat([sharp, blur]).contiguous()
    tmp = torch.empty_like(both)
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "configs": {}}
    emit("B = %d pairs, %d levels of %dx%d, min / median / max of %d in ms, interleaved:" % (B, L_LEVELS, W, H, reps))
    yy, xx = np.meshgrid(np.arange(H) - (H - 1) / 2.0, np.arange(W) - (W - 1) / 2.0, indexing="ij")
    V1 = (1.0 - 0.5 * (xx * xx + yy * yy) / (((H - 1) / 2.0) ** 2 + ((W - 1) / 2.0) ** 2)).astype(np.float32)
    gamma = 255.0 * np.power(np.arange(256.0) / 255.0, 2.2)
    for undistort in (0, 1):
        for G in (0, G_SET):
            n = max(1, G)
            Gs = np.ascontiguousarray(np.stack([gamma] * n))
            V = torch.from_numpy(np.ascontiguousarray(np.stack([V1] * n))).to("cuda:0")
            ones = torch.ones_like(V)
            luts = np.stack([workloads.photometric_table(gamma, 0.5)[1]] * n)
            inv = (1.0 / V).contiguous()
            cal_of_image = np.array([b % n for b in range(B)] * 2, np.int32)
            plain, cal = make(ctx, B, undistort, G), make(ctx, B, undistort, G)
            os.environ["MBAVO_PAIRS_PHOTOCAL_LDS"] = "0"
            lib.mbavo_reload_env()
            cal_plain = make(ctx, B, undistort, G)
            assert cal_plain.set_photometric(Gs, V, scale=0.5) == 0  # (the switch is read here)
            del os.environ["MBAVO_PAIRS_PHOTOCAL_LDS"]
            lib.mbavo_reload_env()
            old = make(parent, B, undistort, G) if parent else None
            state = {}

            def with_cal(vig):
                def setup():
                    if state.get("cal") != vig:
                        assert cal.set_photometric(Gs, {"V": V, "ones": ones, "none": None}[vig], scale=0.5) == 0
                        state["cal"] = vig
                return setup

            def composed():
                workloads.photometric_u8_batch(ctx, both, luts, inv, cal_of_image, out=tmp)
                plain.prepare(tmp[:B], z, tmp[B:])

            routes = {"a": (None, lambda: plain.prepare(sharp, z, blur)), "b": (with_cal("V"), lambda: cal.prepare(sharp, z, blur)),
                      "b plain": (None, lambda: cal_plain.prepare(sharp, z, blur)), "b flag": (with_cal("none"), lambda: cal.prepare(sharp, z, blur)),
                      "b ones": (with_cal("ones"), lambda: cal.prepare(sharp, z, blur)),
                      "e": (None, lambda: (cal.set_photometric(Gs, V, scale=0.5), state.update(cal="V")))}
            if old:
                routes["a parent"] = (None, lambda: old.prepare(sharp, z, blur))
            if undistort == 0:
                routes["c"] = (None, composed)
            order = [key for key in ("a parent", "a", "b", "b plain", "b flag", "b ones", "c", "e") if key in routes]
            t = {key: [] for key in order}
            for rep in range(reps + 2):
                for key in order:
                    setup, run = routes[key]
                    if setup:
                        setup()
                    v = timed(run)
                    if rep >= 2:
                        t[key].append(v)
            med = {key: statistics.median(v) for key, v in t.items()}
            res = {key: mmm(v) for key, v in t.items()}
            base = med.get("a parent", med["a"])
            res.update(b_over_a=round(med["b"] / base, 3), a_over_parent=round(med["a"] / base, 3), plain_over_lds=round(med["b plain"] / med["b"], 3),
                       ones_over_flag=round(med["b ones"] / med["b flag"], 3), launches_a=plain.stats()[0], launches_b=cal.stats()[0])
            if "c" in med:
                res["c_over_b"] = round(med["c"] / med["b"], 3)
            name = "undistort %d, %s" % (undistort, "G = %d" % G if G else "one camera")
            out["configs"][name] = res
            emit("  %-24s %s | b / a%s %.3f, a / parent %.3f, plain loads / LDS %.3f, ones / flag %.3f%s; launches a %d, b %d"
                 % (name, "  ".join("%s %s" % (key, res[key]) for key in order), " parent" if old else "", res["b_over_a"], res["a_over_parent"],
                    res["plain_over_lds"], res["ones_over_flag"], ", c / b %.3f" % res["c_over_b"] if "c" in med else "", res["launches_a"], res["launches_b"]))
            for pb in (plain, cal, cal_plain, old):
                if pb:
                    pb.close()
            torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r43_pairs_photocal.txt")
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
        f.write(head + MARK + " (python tools/pairs_photocal_bench.py %s, one MI355X%s)\n" % (" ".join(str(b) for b in Bs), "" if parent else ", no parent library")
                + "\n".join(text) + "\n")
    if parent:
        parent.close()
    ctx.close()
