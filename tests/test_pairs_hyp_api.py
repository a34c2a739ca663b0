"""mbavo_pairs_predict_hypotheses without a GPU: the entries exist in the library, the header and the binding and the two structs
have the sizes of their ctypes mirrors; the argument rules that need no device; mbavo_pairs_plan has not grown; hypothesis 0 of the
restatement (tests/pairs_hyp_ref.py) is tests/pairs_track.host_predict bit for bit; and the preconditions of the GPU winner checks,
asserted with the oracle on the inputs those checks use (tests/pairs_hyp_ref.win_case): on every pair the oracle's best and
second-best eligible scores differ by more than 1 % and hypothesis 0's score differs from the best challenger's by more than 1 %,
the flung-out hypothesis keeps no pixel, every other hypothesis keeps at least 0.6 K P, the oracle's winner is the hypothesis the
frame was rendered on, and both zero and non-zero winners occur."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_hyp_ref as hr
import pairs_step as ps
import pairs_track as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbavo_pairs_hyp_opts_size", "mbavo_pairs_hyp_size", "mbavo_pairs_predict_hypotheses", "mbavo_pairs_hyp_stats"]
E_ARG = -1


def test_symbols_and_sizes(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    assert lib.mbavo_pairs_hyp_opts_size() == C.sizeof(capi.PairsHypOpts) == 8 + 8 * (2 + 16 + 96) + 16
    assert lib.mbavo_pairs_hyp_size() == C.sizeof(capi.PairsHyp) == 16 + 8 * 32
    assert re.search(r"#define\s+MBAVO_PAIRS_MAX_HYP\s+16\b", header) and re.search(r"#define\s+MBAVO_HYP_NONE_ELIGIBLE\s+1\b", header)
    assert lib.mbavo_abi_version() == 3 and lib.mbavo_pairs_opts_size() == 272  # no existing struct has changed


def test_argument_rules_that_need_no_device(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    one, o, out = np.zeros(1), capi.PairsHypOpts(), (capi.PairsHyp * 1)()
    o.M = 1
    assert lib.mbavo_pairs_predict_hypotheses(None, capi.dp(one), capi.dp(one), C.byref(o), out) == E_ARG
    assert lib.mbavo_pairs_hyp_stats(None, (C.c_longlong * 3)()) == E_ARG
    from mba_vo_amd import workloads
    assert callable(workloads.PairBatch.predict_hypotheses) and callable(workloads.PairBatch.hyp_stats)


# mbavo_pairs_plan of the parent commit (pure host arithmetic) for the objects of tests/test_gpu_pairs_hyp.py: the hypotheses'
# scratch is made at the first call and is not part of it.  (B, H, W, k, every_candidate, num_cameras) with L = 3, N = 6, S = 8, the
# 8-pixel pattern, cell 10, border 4: bytes.
PARENT_PLAN = {(1, 120, 160, 2, 0, 0): 270080, (7, 120, 160, 4, 0, 0): 1882624, (7, 120, 160, 4, 1, 0): 6008832, (7, 120, 160, 4, 0, 2): 1882624}


def test_the_plan_has_not_grown(mbavo):
    from mba_vo_amd import synth
    lib, capi = mbavo.load(), mbavo.capi
    pat = synth.PATTERN8.copy()
    for (B, H, W, k, dense, G), want in PARENT_PLAN.items():
        o = capi.PairsOpts()
        o.B, o.L, o.H, o.W, o.spline_deg_k, o.N = B, hr.LEVELS, H, W, k, ps.N_KNOTS
        for l in range(hr.LEVELS):
            o.S[l], o.P[l], o.border[l] = hr.S, hr.P, hr.BORDER
            o.pattern_xy[l] = pat.ctypes.data_as(capi.c_ip)
        o.cell_H = o.cell_W = ps.CELL
        o.every_candidate, o.num_cameras, o.score_threshold, o.huber_a = dense, G, ps.THR, hr.HUBER
        nbytes, cells = C.c_longlong(0), (C.c_int * 8)()
        assert lib.mbavo_pairs_plan(C.byref(o), C.byref(nbytes), cells) == 0
        assert nbytes.value == want, ((B, H, W, k, dense, G), nbytes.value)


@pytest.mark.parametrize("B,H,W,k", hr.WIN_CASES)
def test_hypothesis_zero_is_host_predict(mbavo, B, H, W, k):
    lib, capi = mbavo.load(), mbavo.capi
    case = ps.assess_inputs(B, H, W, k)
    states = pt.make_states(capi, case)
    for b in range(B):
        t0, kt, kR, dt_frame = pt.host_predict(lib, capi.dp, states[b], case["cap"][b], case["exp"][b])
        ct, cR = hr.candidate(lib, capi.dp, states[b], case["cap"][b], 0)
        assert ct.tobytes() == kt.tobytes() and cR.tobytes() == kR.tobytes(), b
        # a unit scale without a twist is the same tangent, a hypothesis that differs is not the same candidate
        one = hr.candidate(lib, capi.dp, states[b], case["cap"][b], 3, 1.0, (0.0,) * 6)
        assert one[0].tobytes() == kt.tobytes() and one[1].tobytes() == kR.tobytes()
        if np.any(np.array(states[b].velocity) != 0):
            assert hr.candidate(lib, capi.dp, states[b], case["cap"][b], 1, 0.5, (0.0,) * 6)[0].tobytes() != kt.tobytes()


def test_selection_rule_on_hand_made_numbers():
    assert hr.winner([5.0, 4.0, 3.0, 3.0], [True] * 4) == (2, 0, 4)                  # the tie goes to the lowest index
    assert hr.winner([5.0, 4.0, 3.0, 3.0], [True, True, False, False]) == (1, 0, 2)
    assert hr.winner([5.0, 4.0], [True, True], min_gain=0.2) == (0, 0, 2)            # 4 is not below 5 * 0.8
    assert hr.winner([5.0, 3.9], [True, True], min_gain=0.2) == (1, 0, 2)
    assert hr.winner([5.0, 9.0], [False, True]) == (1, 0, 1)                         # hypothesis 0 ineligible: any eligible challenger
    assert hr.winner([5.0, 9.0], [False, False]) == (0, hr.NONE_ELIGIBLE, 0)
    assert hr.winner([5.0], [True]) == (0, 0, 1)
    assert not hr.eligible(hr.score(0.0, 10, 8, 0.0), 10, 8, 0.0, 0.0)               # 0 / 0: not finite
    assert hr.eligible(1.0, 10, 8, 40.0, 0.0) and not hr.eligible(1.0, 10, 8, 39.0, 0.0) and hr.eligible(1.0, 10, 8, 39.0, 0.25)
    assert not hr.eligible(1.0, 0, 8, 0.0, 0.0)
    assert hr.tangent([1.0, 2.0], 0.1, 2, 0.5, [0.25, 0.0]) == [(0.5 * 1.0) * 0.1 + 0.25, (0.5 * 2.0) * 0.1 + 0.0]


@pytest.mark.parametrize("B,H,W,k", hr.WIN_CASES)
def test_the_winner_inputs_are_good_ones(orc, mbavo, B, H, W, k):
    case = hr.win_case(orc, mbavo, B, H, W, k)
    level = hr.LEVELS - 1
    winners = []
    for b in range(B):
        e = hr.host_entry(case, b, level)
        KP = float(e["K"]) * e["P"]
        assert e["K"] > 0, b
        scores, valids, elig, _ = hr.oracle_scores(orc, e, case["cands"][b])
        w, status, n = hr.winner(scores, elig)
        print("pair %d (truth %d): K %d, winner %d, scores %s, valid / KP %s"
              % (b, case["truth"][b], e["K"], w, " ".join("%.4g" % s for s in scores), " ".join("%.2f" % (v / KP) for v in valids)))
        assert valids[hr.FLUNG] == 0 and not elig[hr.FLUNG], b
        assert all(valids[m] >= 0.6 * KP and elig[m] for m in range(len(scores)) if m != hr.FLUNG), (b, valids, KP)
        order = sorted(s for s, ok in zip(scores, elig) if ok)
        assert order[1] - order[0] > 0.01 * order[1], (b, order[:2])
        best_challenger = min(s for m, (s, ok) in enumerate(zip(scores, elig)) if ok and m >= 1)
        assert abs(scores[0] - best_challenger) > 0.01 * max(scores[0], best_challenger), (b, scores[0], best_challenger)
        assert w == case["truth"][b] and status == 0 and n == len(scores) - 1, (b, w, case["truth"][b])
        winners.append(w)
    assert B == 1 or (0 in winners and any(w != 0 for w in winners)), winners


def test_the_eligibility_inputs_are_good_ones(orc, mbavo):
    """min_valid_frac = 1: by the oracle, pair FAST loses a pixel under every hypothesis and keeps some under hypothesis 0, pair
    BLANK has no keypoint at the level, and every other pair has an eligible hypothesis."""
    case, _ = hr.elig_case(orc, mbavo)
    level = hr.LEVELS - 1
    for b in range(case["B"]):
        e = hr.host_entry(case, b, level)
        KP = float(e["K"]) * e["P"]
        scores, valids, elig, _ = hr.oracle_scores(orc, e, case["cands"][b], 1.0)
        w, status, n = hr.winner(scores, elig)
        print("pair %d: K %d, valid / KP %s, winner %d status %d eligible %d" % (b, e["K"], " ".join("%.3f" % (v / max(KP, 1)) for v in valids), w, status, n))
        if b == hr.BLANK:
            assert e["K"] == 0 and (w, status, n) == (0, hr.NONE_ELIGIBLE, 0)
        elif b == hr.FAST:
            assert e["K"] > 0 and all(v < KP for v in valids) and valids[0] > 0 and (w, status, n) == (0, hr.NONE_ELIGIBLE, 0)
        else:
            assert status == 0 and n >= 1 and w != hr.ELIG_FLUNG, b
        assert valids[hr.ELIG_FLUNG] == 0
