"""Device-resident tracker state of a batch of pairs (mbavo_pairs_set_states / _get_states / _predict / _commit / _track_stats /
_track_frame, mbavo_pairs_frame_size): what can be held without a GPU.  The entry points exist in the library, the header and
the binding; the frame record's mirror has the library's size; and the six sequences the GPU file (tests/test_gpu_pairs_track.py)
tracks free-running keep every keyframe decision far enough from its thresholds that all 48 verdicts can be compared."""
import ctypes as C
import os
import re

import frontend
import pairs_step as ps
import pairs_track as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbavo_pairs_set_states", "mbavo_pairs_get_states", "mbavo_pairs_predict", "mbavo_pairs_frame_size", "mbavo_pairs_commit",
       "mbavo_pairs_track_stats", "mbavo_pairs_track_frame"]
E_ARG = -1


def test_track_entry_points_are_exported_declared_and_listed(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    assert lib.mbavo_pairs_frame_size() == C.sizeof(capi.PairsFrame) == 144
    assert capi.PairsFrame.T_world.offset == lib.mbavo_pairs_assessment_size() == 88  # (no padding)
    assert lib.mbavo_abi_version() == 3


def test_null_arguments(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    st, fr, out6 = (capi.VoState * 1)(), (capi.PairsFrame * 1)(), (C.c_longlong * 6)()
    one = (C.c_double * 1)(0.1)
    o = capi.LmBatchOpts()
    assert lib.mbavo_pairs_set_states(None, st) == E_ARG and lib.mbavo_pairs_get_states(None, st) == E_ARG
    assert lib.mbavo_pairs_predict(None, one, one) == E_ARG
    assert lib.mbavo_pairs_commit(None, 2.5, 6.0, 3.0, fr) == E_ARG
    assert lib.mbavo_pairs_track_stats(None, out6) == E_ARG
    assert lib.mbavo_pairs_track_frame(None, None, 0, None, None, None, one, one, C.byref(o), None, None, 0, 2.5, 6.0, 3.0, fr, None) == E_ARG


def test_free_running_sequences_have_margin(orc):
    """The oracle's tracker on the six sequences of pairs_step.SEQ_SEEDS, M = 8: on every one of the 48 (pair, frame) results both
    averages lie more than 8 * KNOT_TOL * fx = 0.064 px from every keyframe threshold (free-running for up to eight frames at the
    project's per-frame knot tolerance), so the GPU file compares every verdict and leaves none out.  The verdicts alternate."""
    need, smallest = None, float("inf")
    for s in ps.SEQ_SEEDS:
        seq = frontend.make_sequence(orc, M=ps.SEQ_M, seed=s)
        out = frontend.run_oracle_vo(orc, seq, frontend.DEFAULTS)
        assert len(out) == ps.SEQ_M + 1
        assert [o["is_keyframe"] for o in out[1:]] == [0, 1] * (ps.SEQ_M // 2), s
        need = ps.SEQ_M * ps.knot_pixel_bound(seq["intr"])
        m = pt.keyframe_margins(out)
        print("seed %d: smallest keyframe margin %.4f px (needed: more than %.4f)" % (s, m, need))
        assert m > need, (s, m, need)
        smallest = min(smallest, m)
    assert abs(need - 0.064) < 1e-12
    print("smallest margin over the 48 results: %.4f px" % smallest)
