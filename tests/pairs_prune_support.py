"""What the GPU tests of mbavo_pairs_prune_keypoints share beside the restatement (tests/pairs_prune_ref.py) (helper, no test in
it): the flag bytes of a call from keep masks, a random filter state, the object's problems on compacted copies and one evaluation of
them; and the inputs of tests/test_gpu_pairs_prune_options.py -- the seeded keep patterns per (pair, level) of objects A - D
(tests/pairs_oracle.py) and the min_keep value of object D -- which need no device, so that
tests/test_pairs_prune_hyp_options_inputs.py can assert on the CPU what the GPU file rests on."""
import ctypes as C

import numpy as np

MASK = (1 << 3) | (1 << 5)
STAY, GO = np.array([0, 1, 2, 4, 32, 33, 77, 255], np.uint8), np.array([3, 5], np.uint8)
# the filter's tolerance after a prune: that of tests/test_gpu_pairs_filter.py, 3.23e-14 being the largest relative difference
# measured there on an MI355X (profiles/r31_pairs_filter.txt)
FILTER_BOUND = min(8 * 3.23e-14, 1e-9)
REC = 32  # bytes of one record

# ---- the option-laden objects: which pair a listed call leaves out, the seeds of the keep patterns, object D's min_keep
LEFT_OUT = 1
SEED_ALL, SEED_LEVEL, SEED_FILTER, SEED_MIN_KEEP, SEED_SLOT = 11, 23, 37, 41, 53
SHARE = 0.7      # of a (pair, level)'s keypoints a pattern keeps, on average
MIN_KEEP_D = 32  # object D, SEED_MIN_KEEP: the survivors are [53, 48, 33], [15, 14, 11], [36, 30, 17] -- pair 2 has served and skipped levels


def listed_pairs(B):
    return [b for b in range(B) if b != LEFT_OUT]


def keep_patterns(Ks, seed, levels=None):
    """{(b, l): K bools} for every pair and every level of `levels` (default: all), from the counts Ks (B x L) and the seed alone."""
    Ks = np.asarray(Ks)
    rng = np.random.default_rng(seed)
    return {(b, l): rng.uniform(size=int(Ks[b, l])) < SHARE for b in range(Ks.shape[0]) for l in (range(Ks.shape[1]) if levels is None else levels)}


def flag_bytes(B, cap, keeps, rng, level=-1):
    """The call's flag bytes from per (pair, level) keep masks, in the layout of a call on `level`: bytes that never drop where a
    keypoint stays (values of 32 and more among them), a byte of MASK where it goes, 5 -- a dropping byte -- from K on, where nothing
    may be read, and over the whole row of a pair without a mask."""
    n, off = (sum(cap), {l: sum(cap[:l]) for l in range(len(cap))}) if level < 0 else (cap[level], {level: 0})
    fl = np.full((B, n), 5, np.uint8)
    for (b, l), keep in keeps.items():
        fl[b, off[l]:off[l] + len(keep)] = np.where(keep, rng.choice(STAY, len(keep)), rng.choice(GO, len(keep)))
    return fl


def flags_of(pb, keeps, rng):
    """flag_bytes of a call on every level of the object."""
    return flag_bytes(pb.B, pb.capacities(), keeps, rng)


def random_state(pb, rng):
    """The filter's state filled with random values over its whole capacity (the arrays are the object's own, writable)."""
    import torch
    s = pb.filter_state()
    n = s["mu"].shape
    s["mu"].copy_(torch.from_numpy(rng.uniform(0.1, 2.0, n)))
    s["info"].copy_(torch.from_numpy(rng.uniform(0.0, 50.0, n)))
    s["n_obs"].copy_(torch.from_numpy(rng.integers(0, 9, n).astype(np.int32)))
    s["n_rej"].copy_(torch.from_numpy(rng.integers(0, 5, n).astype(np.int32)))
    torch.cuda.synchronize()


def patched_problems(capi, pb, snap, res):
    """The object's problems with the keypoint pointers and K of the served (pair, level)s on the test's own compacted copies."""
    import torch
    import pairs_device as dv
    arr = (capi.Problem * (pb.B * pb.L))()
    hold = []
    for e in range(pb.B * pb.L):
        C.memmove(C.byref(arr[e]), C.byref(pb.array[e]), C.sizeof(capi.Problem))
        want = res.get((e // pb.L, e % pb.L))
        if want is None:
            continue
        K = want["K"]
        xy, z = dv.dev(np.ascontiguousarray(want["xy"][:max(K, 1)]), np.ascontiguousarray(want["z"][:max(K, 1)]))
        hold += [xy, z]
        arr[e].d_kp_xy, arr[e].d_kp_z, arr[e].K = xy.data_ptr(), z.data_ptr(), K
    torch.cuda.synchronize()
    return arr, hold


def evaluate(ctx, capi, arr, n, k):
    """One evaluation with the Hessian of the n entries: (packed blocks n * E, patch costs of all entries in a row)."""
    import torch
    E = ctx.lib.mbavo_packed_len(k)
    fb = torch.zeros(n * E, dtype=torch.float64, device="cuda:0")
    pc = torch.zeros(max(sum(arr[e].K for e in range(n)), 1), dtype=torch.float64, device="cuda:0")
    assert ctx.lib.mbavo_eval_batch(ctx.handle, n, arr, k, 1, fb.data_ptr(), pc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return fb.cpu().numpy(), pc.cpu().numpy()


def object_capacities(mbavo, name):
    """The per-level keypoint capacities of an object of tests/pairs_oracle.py from mbavo_pairs_plan (host arithmetic, no device)."""
    import pairs_oracle as po
    lib, capi, o = mbavo.load(), mbavo.capi, po.OBJECTS[name]
    pat = np.ascontiguousarray(po.pattern(o), dtype=np.int32)
    q = capi.PairsOpts()
    q.B, q.L, q.H, q.W, q.spline_deg_k, q.N = o["B"], o["L"], o["H"], o["W"], o["k"], o["N"]
    for l in range(o["L"]):
        q.S[l], q.P[l], q.border[l] = o["S"], pat.size // 2, o["border"][l]
        q.pattern_xy[l] = pat.ctypes.data_as(capi.c_ip)
    intr = o["intr"] if o["intr"] is not None else po.to_intr(o, 0)
    for i in range(4):
        q.intrinsics[i] = float(intr[i])
    q.huber_a, q.score_threshold, q.cell_H, q.cell_W, q.keyframe_format = po.HUBER, o["thr"], o["cell"], o["cell"], o["fmt"]
    q.every_candidate = 1 if o["dense"] else 0
    for key, v in (o["depth"] or {}).items():
        setattr(q, key, type(getattr(q, key))(v))
    q.undistort, q.num_cameras, q.valid_radius, q.mask = o["undistort"], len(o["cams"]) if o["cam_of"] is not None else 0, o["radius"], 1 if o["masks"] else 0
    nbytes, cells = C.c_longlong(0), (C.c_int * 8)()
    assert lib.mbavo_pairs_plan(C.byref(q), C.byref(nbytes), cells) == 0
    return [int(cells[l]) for l in range(o["L"])]
