"""mbavo_pairs_report without a GPU: the entries exist in the library, the header and the binding and the record has the size of
its ctypes mirror; the argument rules that need no device; the shift matrix A of the numpy restatement (tests/pairs_report_ref.py)
held to the library's own spline code; and A^T g_local of the restatement held to central differences of the oracle's cost under
the rigid shift.

The shift matrix.  A xi is applied to random knots through mbavo_spline_plus (t_i += dt_i, R_i <- R_i Exp(dw_i)) and the spline is
sampled with mbavo_spline_get_pose at three times inside the segment: the pose must be (t + v + w x t, Exp(w) R).  For the spline
this is an identity (the translation basis sums to 1; dw_i = R_i^T w gives R_i Exp(dw_i) = Exp(w) R_i exactly), so what is left is
rounding; the bound allows the second-order term a first-order A would leave, eps^2 (1 + max |t_i|) for the translation and eps^2
for the quaternion -- a wrong sign or a transposed R_i in A shows as eps |t| or eps, six orders above it.

The oracle.  The cost is piecewise (the current pixel is found by integer truncation) and g uses the keyframe's gradient image, so
g is not the exact gradient of the cost: on a ramp image with the current frame equal to the keyframe, at eps = 1e-4 (the step of
the reference's harness, which reports 3-4 digits for this kind of check), the measured agreement max |fd - A^T g| / max |A^T g| is
4.3e-5 at k = 2 and 6.2e-3 at k = 4 (profiles/r24_pairs_report.txt).  The bounds are 1e-3 (three digits) and 2.5e-2 (four times the
measurement: the computation is deterministic, the margin covers another libm)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_report_ref as rr
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbavo_pairs_report_size", "mbavo_pairs_report", "mbavo_pairs_report_stats"]
E_ARG = -1


def test_symbols_and_size(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    assert lib.mbavo_pairs_report_size() == C.sizeof(capi.PairsReport) == 16 + 8 * (3 + 7 + 36 + 36)
    assert re.search(r"#define\s+MBAVO_REPORT_SINGULAR\s+1\b", header)
    assert lib.mbavo_abi_version() == 3 and lib.mbavo_pairs_opts_size() == 272  # no existing struct has changed


def test_argument_rules_that_need_no_device(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    out = (capi.PairsReport * 1)()
    assert lib.mbavo_pairs_report(None, 3.0, out, None, None) == E_ARG
    assert lib.mbavo_pairs_report_stats(None, (C.c_longlong * 3)()) == E_ARG
    from mba_vo_amd import workloads
    assert callable(workloads.PairBatch.report) and callable(workloads.PairBatch.report_stats)


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _global_step(loc, k, N, s):
    step = np.zeros(6 * N)
    for i in range(k):
        step[3 * (s + i):3 * (s + i) + 3] = loc[3 * i:3 * i + 3]
        step[3 * N + 3 * (s + i):3 * N + 3 * (s + i) + 3] = loc[3 * k + 3 * i:3 * k + 3 * i + 3]
    return step


@pytest.mark.parametrize("k,N,s", [(2, 2, 0), (4, 4, 0), (2, 4, 1), (4, 6, 1)])
def test_the_shift_matrix_against_the_spline_code(mbavo, k, N, s):
    lib, dp = mbavo.load(), mbavo.capi.dp
    rng = np.random.default_rng(10 * k + N)
    kt = rng.uniform(-2.0, 2.0, (N, 3))
    kR = rng.normal(0, 1, (N, 4))
    kR /= np.linalg.norm(kR, axis=1)[:, None]
    kR[1:] = [_qmul(kR[0], np.append(rng.normal(0, 0.05, 3), 1.0)) for _ in range(N - 1)]  # neighbours a few degrees apart
    kR /= np.linalg.norm(kR, axis=1)[:, None]
    kt, kR = np.ascontiguousarray(kt), np.ascontiguousarray(kR)
    t0, dt, eps = 0.0, 0.5, 1e-6
    A = rr.shift_matrix(kt[s:s + k], kR[s:s + k])
    assert A.shape == (6 * k, 6)
    bound_t, bound_q = eps * eps * (1.0 + np.abs(kt).max()), eps * eps
    worst_t = worst_q = 0.0

    def pose(kt_, kR_, t):
        p, q = np.zeros(3), np.zeros(4)
        assert lib.mbavo_spline_get_pose(k, t0, dt, dp(kt_), dp(kR_), N, t, dp(p), dp(q), None, None) == 0
        return p, q

    for axis in range(6):
        xi = np.zeros(6)
        xi[axis] = eps
        ct, cR = np.zeros((N, 3)), np.zeros((N, 4))
        assert lib.mbavo_spline_plus(dp(kt), dp(kR), N, dp(_global_step(A @ xi, k, N, s)), dp(ct), dp(cR)) == 0
        v, w = xi[:3], xi[3:]
        half = 0.5 * np.linalg.norm(w)
        qw = np.append(np.sin(half) * w / np.linalg.norm(w), np.cos(half)) if half > 0 else np.array([0.0, 0.0, 0.0, 1.0])
        for u in (0.1, 0.5, 0.9):
            t = t0 + (s + u) * dt
            assert lib.mbavo_segment_start_index(t, t0, dt) == s
            p0, q0 = pose(kt, kR, t)
            p1, q1 = pose(ct, cR, t)
            want_q = _qmul(qw, q0)
            worst_t = max(worst_t, float(np.abs(p1 - (p0 + v + np.cross(w, p0))).max()))
            worst_q = max(worst_q, float(min(np.abs(q1 - want_q).max(), np.abs(q1 + want_q).max())))
    print("shift matrix k=%d N=%d s=%d: translation %.3e (bound %.3e), quaternion %.3e (bound %.3e)" % (k, N, s, worst_t, bound_t, worst_q, bound_q))
    assert worst_t <= bound_t and worst_q <= bound_q


ORACLE_BOUND = {2: 1e-3, 4: 2.5e-2}  # measured 4.3e-5 and 6.2e-3: see the module docstring


@pytest.mark.parametrize("k", [2, 4])
def test_the_restatement_against_the_oracle(mbavo, orc, k):
    lib, dp = mbavo.load(), mbavo.capi.dp
    sc = scenes.Scene(H=120, W=160, S=4, F=1, k=k, P=8, K=60, seed=3, margin=24, image="ramp", cur="same")
    N, s, eps = sc.N, int(sc.start_idx[0]), 1e-4
    p, keep = sc.oracle_problem(orc)
    cost, g, H = rr.unpack(orc.evaluate(p)["frame_blocks"][0], k)
    A = rr.shift_matrix(sc.knots_t.reshape(-1, 3)[s:s + k], sc.knots_R.reshape(-1, 4)[s:s + k])
    pred = A.T @ g

    def cost_at(xi):
        ct, cR = np.zeros(3 * N), np.zeros(4 * N)
        assert lib.mbavo_spline_plus(dp(sc.knots_t), dp(sc.knots_R), N, dp(_global_step(A @ xi, k, N, s)), dp(ct), dp(cR)) == 0
        moved = scenes.Scene.__new__(scenes.Scene)
        moved.__dict__.update(sc.__dict__)
        moved.knots_t, moved.knots_R = ct, cR
        q, keep_q = moved.oracle_problem(orc)
        return orc.evaluate(q, with_hessian=False)["cost"]

    fd = np.array([(cost_at(eps * np.eye(6)[a]) - cost_at(-eps * np.eye(6)[a])) / (2 * eps) for a in range(6)])
    rel = float(np.abs(fd - pred).max() / np.abs(pred).max())
    print("A^T g against central differences of the oracle's cost, k=%d eps=%g: %.3e (bound %.1e)" % (k, eps, rel, ORACLE_BOUND[k]))
    assert np.abs(pred).max() > 1.0 and rel <= ORACLE_BOUND[k]


def test_the_statistic_and_the_inverse_on_hand_made_numbers():
    costs = np.array([1.0, 1.0, 1.0, 1.0, 1e-9, 9.0])
    mu, var, bound, flags, n = rr.statistic(costs, 1.5)
    assert n == 5 and mu == 13.0 / 5 and abs(var - ((4 * 1.6 ** 2 + 6.4 ** 2) / 5)) < 1e-12
    assert flags.tolist() == [0, 0, 0, 0, 0, 1]                       # 6.4 > 1.5 * 3.2; the cost below 1e-8 is tested too: 2.6 < 4.8
    assert rr.statistic(costs, 0.5)[3].tolist() == [0, 0, 0, 0, 1, 1]  # 1.6 = 0.5 * 3.2 is not above the bound; 2.6 is
    assert rr.statistic(np.zeros(4), 3.0)[3:] == (pytest.approx(np.zeros(4)), 0)
    info = np.diag([4.0, 1.0, 2.0, 8.0, 16.0, 0.5])
    assert np.allclose(rr.cov(info, 2.0), np.diag(2.0 / np.diag(info)), rtol=1e-15)
    assert rr.cov(np.zeros((6, 6)), 1.0) is None
    assert rr.sigma2(3.0, 10, 8, 46.0) == 2.0 * 3.0 * 80.0 / 40.0 and rr.sigma2(3.0, 10, 8, 2.0) == 480.0


# mbavo_pairs_plan of the parent commit (pure host arithmetic): the report's scratch is made at the first report and is not part
# of it.  (B, L, H, W, cell, every_candidate) with k = N = 4, S = 8, the 8-pixel pattern, border 4: bytes, capacities.
PARENT_PLAN = {(3, 3, 72, 96, 6, False): (325888, [221, 130, 63]), (3, 3, 72, 96, 0, True): (929792, [6912, 1728, 432]),
               (3, 2, 120, 160, 12, False): (752128, [154, 88]), (64, 4, 480, 640, 30, False): (263036160, [374, 192, 99, 63]),
               (64, 4, 480, 640, 0, True): (888265472, [307200, 76800, 19200, 4800])}


def test_the_plan_has_not_grown(mbavo):
    from mba_vo_amd import synth
    lib, capi = mbavo.load(), mbavo.capi
    pat = synth.PATTERN8.copy()
    for (B, L, H, W, cell, dense), (want_bytes, want_cells) in PARENT_PLAN.items():
        o = capi.PairsOpts()
        o.B, o.L, o.H, o.W, o.spline_deg_k, o.N = B, L, H, W, 4, 4
        for l in range(L):
            o.S[l], o.P[l], o.border[l] = 8, 8, 4
            o.pattern_xy[l] = pat.ctypes.data_as(capi.c_ip)
        o.cell_H = o.cell_W = cell
        o.every_candidate, o.score_threshold, o.huber_a = int(dense), 4.0, 10.0
        nbytes, cells = C.c_longlong(0), (C.c_int * 8)()
        assert lib.mbavo_pairs_plan(C.byref(o), C.byref(nbytes), cells) == 0
        assert (nbytes.value, list(cells)[:L]) == (want_bytes, want_cells), (B, L, H, W, cell, dense)
