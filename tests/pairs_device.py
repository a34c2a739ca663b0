"""What the pairs tests do on the device: arrays to and from it, also at raw pointers of the library's own arrays, a batch object's
contents read back per (pair, level), the bit-for-bit comparisons of two such read-backs, and the runs of mbavo_lm_batch_levels
and mbavo_pairs_track_frame whose results come back as bytes."""
import ctypes as C

import numpy as np

import pairs_step as ps
from lm_support import lm_batch_opts

_HIP = None


def _hip():
    """The HIP runtime already loaded into the process."""
    global _HIP
    if _HIP is None:
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        _HIP = C.CDLL(path)
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _HIP


def peek(ptr, count, dtype):
    """`count` items of device memory at a raw pointer (the library's own arrays)."""
    import torch
    torch.cuda.synchronize()
    out = np.empty(count, dtype)
    if count:
        assert _hip().hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0
    return out


def poke(ptr, arr):
    """Host array -> device memory at a raw pointer."""
    import torch
    torch.cuda.synchronize()
    arr = np.ascontiguousarray(arr)
    assert _hip().hipMemcpy(C.c_void_p(ptr), arr.ctypes.data, arr.nbytes, 1) == 0


def dev(*arrays):
    import torch
    return [torch.from_numpy(a).to("cuda:0") for a in arrays]


def dev_depth(raw):
    """A stack of maps on the device; uint16 travels as int16 holding the same bits."""
    return dev(np.ascontiguousarray(raw.view(np.int16) if raw.dtype == np.uint16 else raw))[0]


def read_batch(pb, counts):
    """What the batch object holds, per (pair, level), through the pointers of its problem array."""
    out = []
    gb = 8 if pb.opts.keyframe_format == 0 else 4
    for e in range(pb.B * pb.L):
        q = pb.array[e]
        n = q.H * q.W
        assert (q.H, q.W) == (pb.H >> (e % pb.L), pb.W >> (e % pb.L)) and q.K == counts.ravel()[e] and q.F == 1 and q.kp_stride == 2
        assert q.grad_fp16 == pb.opts.keyframe_format and not q.d_outlier
        cur = int(peek(q.d_cur_imgs, 1, np.uint64)[0])
        out.append(dict(ref=peek(q.d_ref_img, n, np.uint8), cur=peek(cur, n, np.uint8), grad=peek(q.d_ref_dIxy, n * gb, np.uint8),
                        xy=peek(q.d_kp_xy, 2 * q.K, np.float64).reshape(-1, 2), z=peek(q.d_kp_z, q.K, np.float64)))
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_twins(got, want, tag):
    """Two read-backs of batch objects hold the same bits."""
    assert len(got) == len(want)
    for e, (g, w) in enumerate(zip(got, want)):
        for key in ("ref", "cur", "grad", "xy", "z"):
            assert same_bits(g[key], w[key]), (tag, e, key)


def assert_same(got, want, fmt, tag):
    """A read-back against what the per-image calls gave (gradient images in the three formats)."""
    assert len(got) == len(want)
    for e, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["ref"], w["ref"]) and np.array_equal(g["cur"], w["cur"]), (tag, e, "pyramid")
        assert np.array_equal(g["grad"], w["grads"][fmt]), (tag, e, "gradient format %d" % fmt)
        assert g["xy"].shape == w["xy"].shape and np.array_equal(g["xy"], w["xy"]) and np.array_equal(g["z"], w["z"]), (tag, e, "keypoints")


def run_lm(ctx, capi, B, L, array, k, cap=256):
    """mbavo_lm_batch_levels, at most 50 iterations: per pair the result's and the trace records' bytes; the record kinds seen."""
    import torch
    res = (capi.LmBatchResult * B)()
    trace = (capi.TraceRec * (B * cap))()
    rc = ctx.lib.mbavo_lm_batch_levels(ctx.handle, B, L, array, C.byref(lm_batch_opts(capi, k, 50)), res, trace, cap)
    assert rc == 0, rc
    torch.cuda.synchronize()
    # the structs' bytes (neither has padding): equality of bits, NaN qualities of degenerate steps included
    fields = [bytes(r) for r in res]
    recs = [[bytes(t) for t in trace[b * cap:b * cap + res[b].num_trace]] for b in range(B)]
    kinds = {t.kind for b in range(B) for t in trace[b * cap:b * cap + res[b].num_trace]}
    return fields, recs, kinds


def frames_of(gpu_ctx, capi, pb, c, blur_t, keys, sharp_t, depth_t, k):
    """One mbavo_pairs_track_frame (3 LM iterations) from the initial states: frames, counts, results and records as bytes."""
    assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0
    B = c["B"]
    out, counts, res, trace = pb.track_frame(blur_t, np.full(B, 0.1), np.full(B, 0.02), lm_batch_opts(capi, k, 3), (ps.FLOW0, ps.FLOW1, ps.KERNEL), keys,
                                             sharp_t, depth_t, trace_cap=16)
    n = [res[b].num_trace for b in range(B)]
    recs = [bytes(trace[b * 16 + i]) for b in range(B) for i in range(min(n[b], 16))]
    return [bytes(out[b]) for b in range(B)], counts, [bytes(res[b]) for b in range(B)], recs
