"""mbavo_pairs_filter_depths without a GPU: the entries exist in the library, the header and the binding, the structs have the sizes
the header states, NULL handles are rejected -- and the specification, restated in numpy (tests/pairs_filter_ref.py on top of
tests/pairs_refine_ref.py), is held to the properties the GPU tests rely on, on the rendered pairs of tests/pairs_refine_scene.py
(level 0: the host side has no pyramid).

The sequence setting of tests/pairs_filter_scene.py (T = 8 frames of the same keyframe at later capture times, noise 2 grey levels,
sigma_i = 2, prior_rel_sigma = 0.05; the ratios and the settings that were tried are in profiles/r31_pairs_filter.txt) is
established HERE: after T filter calls, one per frame, the median relative depth error over the keypoints fused every time is less
than HALF the error after one refinement step on the first frame from the same start -- and less than half of what T refinement
steps on that first frame alone reach, which is what tells a filter over new baselines from an iterated step -- and the median
information grows with every frame.  tests/test_gpu_pairs_filter.py asserts the inequalities without the factor.
Every test here asks the library for the call first: none passes where mbavo_pairs_filter_depths does not exist."""
import ctypes as C

import numpy as np
import pytest

import pairs_filter_ref as fref
import pairs_filter_scene as fs
import pairs_refine_ref as ref
import pairs_refine_scene as sc

E_ARG = -1
NEW = ["mbavo_pairs_filter_opts_size", "mbavo_pairs_filter_size", "mbavo_pairs_filter_depths", "mbavo_pairs_filter_state", "mbavo_pairs_filter_stats"]
GPU_OPTS = dict(prior_rel_sigma=0.1, sigma_i=2.0, gate_chi2=9.0)  # the options of test_gpu_pairs_filter.py's first test
BOUND = 1e-9


@pytest.fixture(autouse=True)
def the_call_exists(mbavo):
    """The restatement restates a call of the library: its records are the binding's."""
    assert mbavo.load().mbavo_pairs_filter_size() == C.sizeof(mbavo.capi.PairsFilter)


def test_entries_and_struct_sizes(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = open(mbavo.HEADER_PATH).read() if hasattr(mbavo, "HEADER_PATH") else None
    for name in NEW:
        assert hasattr(lib, name) and name in capi.SYMBOLS
        assert header is None or name in header
    assert lib.mbavo_pairs_filter_opts_size() == C.sizeof(capi.PairsFilterOpts) == 8 + 8 * 7 + 4 + 28
    assert lib.mbavo_pairs_filter_size() == C.sizeof(capi.PairsFilter) == 24 + 8 * 3


def test_null_handles_are_rejected(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    out = (capi.PairsFilter * 1)()
    for o in (fref.opts_struct(capi), fref.opts_struct(capi, sigma_i=-1.0), fref.opts_struct(capi, reset=2), None):
        assert fref.call(lib, None, o, out) == E_ARG
    p = [C.c_void_p() for _ in range(4)]
    assert lib.mbavo_pairs_filter_state(None, *[C.byref(x) for x in p], C.byref(C.c_longlong()), (C.c_longlong * 8)()) == E_ARG
    assert lib.mbavo_pairs_filter_stats(None, (C.c_longlong * 3)()) == E_ARG


def test_binding_methods_exist(mbavo):
    from mba_vo_amd import workloads
    assert all(callable(getattr(workloads.PairBatch, n)) for n in ("filter_depths", "filter_state", "filter_stats"))


def _measure(mbavo, b, z=None, cur=None, cap=None):
    lib, capi = mbavo.load(), mbavo.capi
    e = sc.entry(b)
    if cur is not None:
        e["curs"] = [np.ascontiguousarray(cur)]
    if cap is not None:
        e["cap"] = np.array([cap])
    if z is not None:
        e["z"] = z
    return e, ref.keypoints(e, ref.poses(lib, capi, e, e["k"]))


@pytest.mark.parametrize("b", range(sc.B))
def test_no_prior_is_the_refinement_bit_for_bit(mbavo, b):
    """prior_rel_sigma = sigma_i = gate_chi2 = 0 after a seed: the depths, the moved set and (d_rho / rho)^2 of pairs_refine_ref.step."""
    e, r = _measure(mbavo, b, z=fs.start_depths(sc.entry(b)["z"], b))
    for kw in (dict(), dict(min_info=1e-3, max_rel_step=0.02), dict(z_min=1.9, z_max=2.05)):
        moved, z_new, rel, h_rho = ref.step(e["z"], r["g"], r["h"], r["full"], **kw)
        f = fref.fuse(e["z"], r["g"], r["h"], r["full"], fref.seed(e["z"], 0.0), **kw)
        assert moved.sum() > 0 and np.array_equal(f["fused"], moved) and not f["rejected"].any()
        assert np.array_equal(f["z_new"].view(np.uint64), z_new.view(np.uint64))
        assert np.array_equal((f["rel"] * f["rel"]).view(np.uint64), (rel * rel).view(np.uint64))
        assert np.array_equal((1.0 / f["state"]["mu"][moved]).view(np.uint64), z_new[moved].view(np.uint64))  # (D_new = 1.0 / rho_n, mu = rho_n)
        assert np.array_equal(f["state"]["info"][moved].view(np.uint64), h_rho[moved].view(np.uint64))


def _sequence(mbavo, b, T, noise, **opts):
    """T filter calls with apply = 1, frame t in call t: (states after each call, depths after each, candidates per call, fused per call)."""
    truth = sc.entry(b)["z"]
    z = fs.start_depths(truth, b)
    fr, caps = fs.frames(b, T, noise), fs.caps(b, T)
    state, states, zs, cands, fused = None, [], [], [], []
    for t in range(T):
        e, r = _measure(mbavo, b, z=z, cur=fr[t], cap=caps[t])
        before = fref.seed(z, opts.get("prior_rel_sigma", 0.0)) if t == 0 else state
        f = fref.fuse(z, r["g"], r["h"], r["full"], before, **opts)
        state, z = f["state"], f["z_new"]
        states.append(state); zs.append(z); cands.append(f["cand"]); fused.append(f["fused"])
    return truth, states, zs, cands, fused


@pytest.mark.parametrize("b", range(sc.B))
def test_info_never_decreases_and_counters_count_candidates(mbavo, b):
    truth, states, zs, cands, fused = _sequence(mbavo, b, 3, fs.NOISE, **GPU_OPTS)
    seen = np.zeros(truth.size, np.int64)
    last = fref.seed(fs.start_depths(truth, b), GPU_OPTS["prior_rel_sigma"])["info"]
    for st, c, fu in zip(states, cands, fused):
        seen += c
        assert (st["info"] >= last).all() and (st["info"][fu] > last[fu]).all()
        # (a candidate that neither fuses nor is gated -- a depth outside [z_min, z_max] -- would be counted nowhere: none here)
        assert np.array_equal(st["n_obs"] + st["n_rej"], seen)
        last = st["info"]
    assert seen.max() == 3


@pytest.mark.parametrize("b", range(sc.B))
def test_the_gate_has_room_on_these_inputs(mbavo, b):
    """The decisions of the gate at gate_chi2 = 9 do not change when g moves by +-BOUND (relative): no c2 of these inputs lies
    that close to the gate, so a device within BOUND of the restatement decides alike."""
    truth = sc.entry(b)["z"]
    z = fs.start_depths(truth, b)
    e, r = _measure(mbavo, b, z=z, cur=fs.frames(b, 2)[1], cap=fs.caps(b, 2)[1])
    st = fref.seed(truth, GPU_OPTS["prior_rel_sigma"])  # (a state that disagrees with the measurement by 5 %: the gate has work)
    base = fref.fuse(z, r["g"], r["h"], r["full"], st, **GPU_OPTS)
    assert base["cand"].sum() > 0
    for s in (1.0 - BOUND, 1.0 + BOUND):
        f = fref.fuse(z, r["g"] * s, r["h"], r["full"], st, **GPU_OPTS)
        assert np.array_equal(f["rejected"], base["rejected"]) and np.array_equal(f["fused"], base["fused"])
    c2 = base["c2"][np.isfinite(base["c2"])]
    print("pair %d: %d gated candidates, %d rejected, closest c2 / gate - 1 = %.3g" % (b, c2.size, base["rejected"].sum(), np.abs(c2 / 9.0 - 1).min()))


def test_the_filter_does_what_a_filter_is_for(mbavo):
    """The setting of tests/pairs_filter_scene.py, with a margin of 2 in the error ratio."""
    opts = fs.OPTS
    for b in range(sc.B):
        truth, states, zs, cands, fused = _sequence(mbavo, b, fs.T, fs.NOISE, **opts)
        every = np.all(fused, 0)
        e, r = _measure(mbavo, b, z=fs.start_depths(truth, b), cur=fs.frames(b)[0])
        moved, z_one, rel, h_rho = ref.step(e["z"], r["g"], r["h"], r["full"])
        err_one = float(np.median(np.abs(z_one[every] / truth[every] - 1.0)))
        z_rep = z_one  # (what iterating the step on the one frame reaches: the filter must beat that too, or it is no filter)
        for _ in range(fs.T - 1):
            er, rr = _measure(mbavo, b, z=z_rep, cur=fs.frames(b)[0])
            z_rep = ref.step(er["z"], rr["g"], rr["h"], rr["full"])[1]
        err_rep = float(np.median(np.abs(z_rep[every] / truth[every] - 1.0)))
        err_T = float(np.median(np.abs(zs[-1][every] / truth[every] - 1.0)))
        infos = [float(np.median(st["info"][every])) for st in states]
        print("pair %d: %d of %d keypoints fused every time; median relative error: one refinement %.4f, %d filter calls %.4f (ratio %.2f); "
              "median info %s" % (b, every.sum(), truth.size, err_one, fs.T, err_T, err_one / err_T, " ".join("%.3g" % v for v in infos)))
        assert 2 * every.sum() >= truth.size
        print("pair %d: %d refinement steps on the first frame alone %.4f (ratio %.2f)" % (b, fs.T, err_rep, err_rep / err_T))
        assert 2.0 * err_T < err_one and 2.0 * err_T < err_rep
        assert all(i1 > i0 for i0, i1 in zip(infos, infos[1:]))
