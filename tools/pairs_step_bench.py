"""The two device steps of a batch of keyframe pairs from frame to frame (640 x 480, 4 pyramid levels), each against the route
available without it, inside one process, interleaved, `reps` repetitions each after a warm-up, every repetition ending in a
device synchronisation:
  (a) mbavo_pairs_assess (one launch, one copy of B x 88 bytes, one synchronisation) against the host route:
      mbavo_pairs_get_knots, a read-back of every pair's level-0 keypoints (two copies per pair) and the keyframe test as a
      compiled loop -- the oracle's orc_is_keyframe (oracle/mbavo_oracle_vo.c), which is the host tracker's isKeyframe restated;
  (b) mbavo_pairs_update with new blurred frames for all pairs and new keyframes for every second pair, against a full
      mbavo_pairs_prepare of all B pairs.
Checks that both routes of (a) give the same verdicts and that (b)'s update leaves the counts a prepare of the composite inputs gives.
Usage: python tools/pairs_step_bench.py [B ...] [--out FILE]  (default 64 512 -> profiles/r11_pairs_step.txt)"""
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
_HIP = None


def _peek_into(ptr, out):
    global _HIP
    if _HIP is None:
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        _HIP = C.CDLL(path)
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    if out.nbytes:
        assert _HIP.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0


def host_route(orc, pb, intr, cap, exp):
    """(a)'s comparison: the knots, every pair's level-0 keypoints, the compiled loop; (verdict, avg_flow, avg_kernel) per pair."""
    L = orc.lib()
    kt, kR = pb.knots()
    out = []
    af, ak = np.zeros(1), np.zeros(1)
    for b in range(pb.B):
        q = pb.array[b * pb.L]
        xy, z = np.empty(2 * q.K), np.empty(q.K)
        _peek_into(q.d_kp_xy, xy)
        _peek_into(q.d_kp_z, z)
        v = L.orc_is_keyframe(orc.dp(intr), orc.dp(xy), orc.dp(z), q.K, K_DEG, 0.0, 0.5, orc.dp(kt[b]), orc.dp(kR[b]), float(cap[b]), float(exp[b]),
                              FLOW0, FLOW1, KERNEL, orc.dp(af), orc.dp(ak))
        out.append((int(v), float(af[0]), float(ak[0])))
    return out


def _stat(ts):
    return {"min_ms": round(min(ts), 3), "median_ms": round(statistics.median(ts), 3), "max_ms": round(max(ts), 3)}


def bench(M, orc, ctx, B, reps=10, seed=1):
    import torch
    from mba_vo_amd import synth, workloads
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(seed)
    bases = [torch.from_numpy(synth.texture_image(H, W, seed=seed + i, octaves=(32, 16, 8, 4))).to(dev) for i in range(4)]

    def images(off):
        return torch.stack([torch.roll(bases[(b + off) % 4], ((7 * b + off) % H, (13 * b + 3 * off) % W), (0, 1)) for b in range(B)]).contiguous()

    sharp, blur, sharp2, blur2 = images(0), images(1), images(2), images(3)
    depth = (torch.rand((B, H, W), generator=g, device=dev) * 2.0 + 1.0).contiguous()
    depth2 = (torch.rand((B, H, W), generator=g, device=dev) * 2.0 + 1.0).contiguous()
    keys = list(range(0, B, 2))
    sharp_k, depth_k = sharp2[keys].contiguous(), depth2[keys].contiguous()
    intr = np.array([W / 2.0, W / 2.0, W / 2.0, H / 2.0])
    kt, kR = np.zeros((B, N, 3)), np.zeros((B, N, 4))
    for b in range(B):
        s = (0.05, 0.4, 0.9, 1.6, 2.8)[b % 5]
        kt[b], kR[b] = synth.trajectory("harness", N, 0.012 * s, 0.02 * s)
    cap, exp = np.full(B, 0.2), np.full(B, 0.04)
    pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, k=K_DEG, N=N, cell=CELL, thresh=THRESH)
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "n_key": len(keys)}
    try:
        counts = pb.prepare(sharp, depth, blur)
        assert pb.set_motion(cap, exp, np.zeros(B), 0.5, kt, kR) == 0
        got, want = pb.assess(FLOW0, FLOW1, KERNEL), host_route(orc, pb, intr, cap, exp)  # warm-up, both routes
        out["verdicts_equal"] = [a.is_keyframe for a in got] == [w[0] for w in want]
        out["keyframes"] = int(sum(w[0] for w in want))
        out["max_avg_diff_rel"] = float(max(abs(a.avg_flow - w[1]) / w[1] for a, w in zip(got, want)))
        ta, th = [], []
        for _ in range(reps):
            for fn, ts in ((lambda: pb.assess(FLOW0, FLOW1, KERNEL), ta), (lambda: host_route(orc, pb, intr, cap, exp), th)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t))
        out["assess"], out["host_route"] = _stat(ta), _stat(th)
        out["assess_stats"] = pb.step_stats()[1]
        out["K0_mean"] = round(float(counts[:, 0].mean()), 1)
        # (b): alternate the two sets of inputs so that every update really changes what it lists
        sets = [(blur2, sharp_k, depth_k), (blur, sharp[keys].contiguous(), depth[keys].contiguous())]
        full = [(sharp.clone(), depth.clone(), blur2), (sharp, depth, blur)]
        full[0][0][keys] = sharp2[keys]
        full[0][1][keys] = depth2[keys]
        cu = pb.update(sets[0][0], keys, sets[0][1], sets[0][2])
        cp = pb.prepare(*full[0])
        out["update_counts_equal"] = bool(np.array_equal(cu, cp))
        tu, tp = [], []
        for r in range(reps):
            sb, sk, dk = sets[(r + 1) % 2]
            fs, fd, fb = full[(r + 1) % 2]
            for fn, ts in ((lambda: pb.update(sb, keys, sk, dk), tu), (lambda: pb.prepare(fs, fd, fb), tp)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t))
        out["update"], out["prepare"] = _stat(tu), _stat(tp)
        pb.update(sets[0][0], keys, sets[0][1], sets[0][2])
        out["update_stats"] = pb.step_stats()[0]
    finally:
        pb.close()
    return out


def _verdict(new, old):
    gain = old["median_ms"] - new["median_ms"]
    spread = max(new["max_ms"] - new["min_ms"], old["max_ms"] - old["min_ms"])
    return "%.2fx on the medians; the medians differ by %.3f ms, the larger spread (max - min) of the repetitions is %.3f ms: %s" % (
        old["median_ms"] / new["median_ms"], gain, spread, "faster by more than the spread" if gain > spread else "NOT faster by more than the spread")


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    from oracle import binding as orc
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "r11_pairs_step.txt")
    if "--out" in args:
        i = args.index("--out")
        path = args[i + 1]
        del args[i:i + 2]
    Bs = [int(a) for a in args] or [64, 512]
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    text, lines = [], []
    for B in Bs:
        r = bench(mbavo, orc, ctx, B)
        lines.append(r)
        text.append("B = %d pairs, %d levels of %dx%d, %d repetitions each, interleaved; level-0 keypoints per pair %.1f, %d of %d verdicts 'keyframe':" % (
            B, r["L"], r["W"], r["H"], r["reps"], r["K0_mean"], r["keyframes"], B))
        for name, key in (("(a) mbavo_pairs_assess", "assess"), ("    host route (get_knots + keypoint read-back + orc_is_keyframe)", "host_route"),
                          ("(b) mbavo_pairs_update, %d of %d keyframes new" % (r["n_key"], B), "update"), ("    mbavo_pairs_prepare, all pairs", "prepare")):
            s = r[key]
            text.append("  %-68s min %9.3f ms  median %9.3f ms  max %9.3f ms" % (name, s["min_ms"], s["median_ms"], s["max_ms"]))
        text.append("  (a): %s  (verdicts equal: %s; launches, synchronisations, D2H bytes: %s)" % (_verdict(r["assess"], r["host_route"]), r["verdicts_equal"],
                                                                                                   list(r["assess_stats"])))
        text.append("  (b): %s  (counts equal to a prepare of the composite inputs: %s; launches, synchronisations, D2H bytes: %s)" % (
            _verdict(r["update"], r["prepare"]), r["update_counts_equal"], list(r["update_stats"])))
    text += [json.dumps(r) for r in lines]
    print("\n".join(text))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(text) + "\n")
    ctx.close()
