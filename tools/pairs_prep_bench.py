"""Preparing a batch of rendered keyframe pairs (640 x 480, 4 pyramid levels) for mbavo_lm_batch_levels, two ways inside one
process, interleaved, `reps` repetitions each after a warm-up, every repetition ending in a device synchronisation:
  (a) mbavo_pairs_prepare: all pairs and levels in ceil((L-1)/3) + 3 launches and one stream synchronisation;
  (b) the per-image public calls exactly as workloads.RenderedPairPyramids issues them: per pair two mbavo_pyramid_levels_u8,
      per pair and level one gradient call (mbavo_image_gradients_u8, or mbavo_pack_keyframe_u8 for the packed format), one
      mbavo_detect_semidense (synchronous) and the border filter in torch.
Formats 0 (float gradients) and 2 (packed keyframe).  Checks that both ways find the same keypoint counts, and reports the time
of the LM call the arrays feed (tools/lm_levels_bench.py's run_levels) for scale.
Usage: python tools/pairs_prep_bench.py [B ...]  (default 64 512)      one text block per B, then one JSON line per B"""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

L_LEVELS, CELL, THRESH = 4, 30, 4.0


def per_image(ctx, capi, sharp, depth, blur, L, fmt):
    """(b): RenderedPairPyramids' loop over pairs and levels (its device work and its torch calls); the keypoint counts."""
    import torch
    lib = ctx.lib
    B, H, W = sharp.shape
    counts = np.zeros((B, L), np.int32)
    keep = []
    for b in range(B):
        refs = [sharp[b].view(-1)] + [torch.empty((H >> l) * (W >> l), dtype=torch.uint8, device=sharp.device) for l in range(1, L)]
        curs = [blur[b].view(-1)] + [torch.empty((H >> l) * (W >> l), dtype=torch.uint8, device=sharp.device) for l in range(1, L)]
        for lv in (refs, curs):
            ptrs = (C.c_void_p * L)(*[a.data_ptr() for a in lv])
            capi.check(lib.mbavo_pyramid_levels_u8(ctx.handle, ptrs, H, W, L), "mbavo_pyramid_levels_u8")
        for l in range(L):
            Hl, Wl = H >> l, W >> l
            if fmt == 2:
                grad = torch.empty(Hl * Wl, dtype=torch.int32, device=sharp.device)
                capi.check(lib.mbavo_pack_keyframe_u8(refs[l].data_ptr(), Hl, Wl, grad.data_ptr(), None), "mbavo_pack_keyframe_u8")
            else:
                grad = torch.empty(Hl * Wl * 2, dtype=torch.float32, device=sharp.device)
                capi.check(lib.mbavo_image_gradients_u8(refs[l].data_ptr(), Hl, Wl, grad.data_ptr(), None), "mbavo_image_gradients_u8")
            cl = int(CELL / 1.414 ** l)
            cap_kp = (Hl // cl + 1) * (Wl // cl + 1)
            xy = torch.empty(cap_kp * 2, dtype=torch.float64, device=sharp.device)
            kz = torch.empty(cap_kp, dtype=torch.float64, device=sharp.device)
            cnt = C.c_int(0)
            capi.check(lib.mbavo_detect_semidense(ctx.handle, refs[l].data_ptr(), Hl, Wl, l, H, W, CELL, CELL, THRESH, depth[b].data_ptr(),
                                                  xy.data_ptr(), kz.data_ptr(), cap_kp, C.byref(cnt)), "mbavo_detect_semidense")
            K = min(cnt.value, cap_kp)
            margin = max(4, 20 >> l)
            xyv = xy[:2 * K].view(K, 2)
            ok = (xyv[:, 0] >= margin) & (xyv[:, 0] < Wl - margin) & (xyv[:, 1] >= margin) & (xyv[:, 1] < Hl - margin)
            xy = xyv[ok].contiguous().view(-1)
            kz = kz[:K][ok].contiguous()
            counts[b, l] = int(kz.shape[0])
            cur_ptrs = torch.tensor([curs[l].data_ptr()], dtype=torch.int64, device=sharp.device)
            keep += [grad, xy, kz, cur_ptrs]
    return counts


def bench(M, ctx, B, reps=10, seed=1):
    import torch
    import lm_levels_bench
    from mba_vo_amd import workloads
    capi = M.capi
    L = L_LEVELS
    rpp = workloads.RenderedPairPyramids(ctx, B, L=L, S=8, k=4, seed=seed, cell=CELL, thresh=THRESH)
    H, W = rpp.H, rpp.W
    sharp, depth, blur = workloads.rendered_inputs(rpp)
    out = {"B": B, "L": L, "H": H, "W": W, "reps": reps}
    for fmt in (0, 2):
        pb = workloads.PairBatch(ctx, B, L=L, H=H, W=W, keyframe_format=fmt, cell=CELL, thresh=THRESH)
        ca = pb.prepare(sharp, depth, blur)  # warm-up, both ways
        cb = per_image(ctx, capi, sharp, depth, blur, L, fmt)
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(reps):
            for fn, ts in ((lambda: pb.prepare(sharp, depth, blur), ta), (lambda: per_image(ctx, capi, sharp, depth, blur, L, fmt), tb)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t))
        launches, syncs, d2h, held = pb.stats()
        tag = "fmt%d" % fmt
        out[tag] = {"a_min_ms": round(min(ta), 3), "a_median_ms": round(statistics.median(ta), 3), "b_min_ms": round(min(tb), 3),
                    "b_median_ms": round(statistics.median(tb), 3), "b_over_a_median": round(statistics.median(tb) / statistics.median(ta), 2),
                    "counts_equal": bool(np.array_equal(ca, cb)), "launches": launches, "synchronisations": syncs, "d2h_bytes": d2h,
                    "device_bytes": held, "K_per_level_mean": [round(float(ca[:, l].mean()), 1) for l in range(L)]}
        pb.close()
    for _ in range(2):
        rpp.reset_knots()
        lm_levels_bench.run_levels(M, ctx, rpp, trace=False)
    out["lm_batch_levels_ms"] = round(lm_levels_bench.best_ms(lambda: lm_levels_bench.run_levels(M, ctx, rpp, trace=False), rpp.reset_knots, 5), 3)
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    Bs = [int(a) for a in sys.argv[1:]] or [64, 512]
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    lines = []
    for B in Bs:
        r = bench(mbavo, ctx, B)
        lines.append(r)
        print("B = %d pairs, %d levels of %dx%d, %d repetitions each, interleaved:" % (B, r["L"], r["W"], r["H"], r["reps"]))
        for fmt, name in ((0, "float gradients"), (2, "packed keyframe")):
            f = r["fmt%d" % fmt]
            print("  format %d (%s), %.2f GB held, keypoints per level %s:" % (fmt, name, f["device_bytes"] / 1e9, f["K_per_level_mean"]))
            print("    (a) mbavo_pairs_prepare            min %9.3f ms  median %9.3f ms   %d launches, %d synchronisation, %d B D2H" % (
                f["a_min_ms"], f["a_median_ms"], f["launches"], f["synchronisations"], f["d2h_bytes"]))
            print("    (b) per-image calls, %5d x %d levels min %9.3f ms  median %9.3f ms   (b / a = %.2f on the medians; counts equal: %s)" % (
                B, r["L"], f["b_min_ms"], f["b_median_ms"], f["b_over_a_median"], f["counts_equal"]))
        print("  mbavo_lm_batch_levels on the prepared array (best of 5): %.3f ms" % r["lm_batch_levels_ms"])
        sys.stdout.flush()
    for r in lines:
        print(json.dumps(r))
    ctx.close()
