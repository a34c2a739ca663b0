"""Cases, high-precision references and bounds for the device solvers of mba-vo_amd/csrc/lm_solvers.h (CPU only).

tests/test_gpu_solvers.py sends the cases through tests/harness/solver_check.hip (--cases IN --out OUT) and holds every result
to the reference; tests/test_solver_cases.py checks the generators, the references and the bounds without a device, against
LAPACK and a plain numpy restatement of the unpivoted LDL^T.

Every reference is computed with mpmath at 60 digits FROM THE MATRIX AS STORED IN DOUBLES: the exact solution of the stored
system is the centre of the ball any backward-stable solver lands in.  References are cached per matrix under
tests/.solver_ref_cache (kept out of the history).

The bounds (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.5 / 10.6 after van der Sluis and Demmel:
for Cholesky / LDL^T of a positive definite A = D^1/2 H D^1/2, D = diag(A), the error in the scaled coordinates D^1/2 x is
bounded by n eps kappa(H) -- independent of the grading D; Demmel and Veselic 1992 give the same kappa(H) for the eigenvalues
and vectors Jacobi's method computes with the relative stopping test, while any backward-stable solver reaches n eps kappa(A)):

    scaled:  max_i sqrt(a_ii) |x_i - x*_i|  <=  C_SCALED n eps kappa_s max_i sqrt(a_ii) |x*_i|,  kappa_s = cond(D^-1/2 A D^-1/2)
    plain :  max_i |x_i - x*_i|             <=  C_KAPPA  n eps kappa   max_i |x*_i|,             kappa = largest / smallest KEPT eigenvalue

The constants are 8x the largest ratio error / (n eps kappa |x|) that LAPACK and the numpy restatement reach over all cases
below (tests/test_solver_cases.py recomputes those maxima and asserts the 8x; profiles/r08_solver_accuracy.txt records them
next to the device's own).  They are not tuned on the device's errors.
"""
import hashlib
import os

import numpy as np

EPS = float(np.finfo(np.float64).eps)
FORMS = {"regs": 0, "coop64": 1, "coop256": 2, "svd": 3, "eig": 4, "ldlt": 5}
STANDINS = ("regs", "coop64", "coop256")
REG_SIZES = (12, 18, 24)
COOP_SIZES = (30, 36, 42, 48, 54, 60)        # 5 .. 10 control knots: lm_batch.hip takes spd_solve_coop for n <= 64
STANDIN_SIZES = REG_SIZES + COOP_SIZES
LARGE_SIZES = (66, 72, 78, 84, 90, 96)       # up to the reference's max_num_ctrl_knots = 16
EIG_MAX_N = 48                               # lm_solvers.h: kEigMaxN
FAST_RATIO, REFINED_RATIO = 1e8, 1e13        # the production gates (lm_batch: fast_ratio, refined_ratio)
REFINE_STEPS = 4                             # lm_solvers.h: kRefineSteps
REFINED_TOL = 1e-12                          # the bar solver_check.hip states for an accepted refined result
GATE_MARGIN = 1e-6                           # dense cases whose pivot ratio is this close to a gate have no required verdict
DECADES = ((1e2, 1e8), (1e8, 1e10), (1e10, 1e12), (1e12, 1e13))
MAGIC = 0x3130565F434C4F53                   # "SOLC_V01"
CACHE = os.path.join(os.path.dirname(os.path.abspath(__file__)), ".solver_ref_cache")
MP_DIGITS = 60

# 8 x the CPU maxima (see the module docstring; measured values in profiles/r08_solver_accuracy.txt): 2.62 is numpy.linalg.solve
# on lm_r1_n18 (LU with row pivoting is not invariant under the symmetric scaling; LAPACK's Cholesky and the numpy LDL^T stay
# below 0.11), 0.438 is pinv(hermitian) on neardep_d2_n60
C_SCALED = 21.0
C_KAPPA = 3.5


class System:
    """One linear system and what is known about it by construction."""

    def __init__(self, name, family, A, b, kind="spd", **meta):
        self.name, self.family, self.kind = name, family, kind
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.b = np.ascontiguousarray(b, dtype=np.float64)
        self.n = self.A.shape[0]
        self.meta = meta

    def key(self):
        h = hashlib.sha1()
        h.update(self.kind.encode())
        h.update(self.A.tobytes())
        h.update(self.b.tobytes())
        return h.hexdigest()


class Run:
    """One launch: a system through one form with one pair of gates."""

    def __init__(self, system, form, max_ratio=0.0, max_ratio_refined=0.0):
        self.system, self.form, self.max_ratio, self.max_ratio_refined = system, form, float(max_ratio), float(max_ratio_refined)

    def __repr__(self):
        return "%s[%s n=%d %g/%g]" % (self.system.name, self.form, self.system.n, self.max_ratio, self.max_ratio_refined)


# ---------------------------------------------------------------------------------------------------------------- numpy restatements
def ldlt_unpivoted(A):
    """Unpivoted LDL^T in float64 as spd_solve_regs_impl / spd_solve_coop do it (right-looking, the update a_ij -= l_ik (d_k l_jk)).
    Returns (L unit lower, d)."""
    M = np.array(A, dtype=np.float64)
    n = M.shape[0]
    L = np.eye(n)
    d = np.zeros(n)
    with np.errstate(all="ignore"):
        for k in range(n):
            d[k] = M[k, k]
            l = M[k + 1:, k] * (1.0 / d[k])
            M[k + 1:, k + 1:] -= np.outer(l, M[k, k + 1:])
            L[k + 1:, k] = l
    return L, d


def ldlt_apply(L, d, r):
    n = len(d)
    y = np.array(r, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            y[k + 1:] -= L[k + 1:, k] * y[k]
        w = y / d
        for k in range(n - 1, 0, -1):
            w[:k] -= L[k, :k] * w[k]
    return w


def pivot_ratio(A):
    _, d = ldlt_unpivoted(A)
    return float(d.max() / d.min()) if np.all(d > 0) else float("inf")


def exact_residual(A, b, x):
    """b - A x, every product and sum exact (mpmath), rounded once."""
    import mpmath as mp
    with mp.workdps(400):  # doubles scaled by 2^+-200 included: exact
        n = len(b)
        out = np.zeros(n)
        xs = [mp.mpf(float(v)) for v in x]
        for i in range(n):
            out[i] = float(mp.mpf(float(b[i])) - mp.fsum(mp.mpf(float(A[i, j])) * xs[j] for j in range(n)))
    return out


def refine_rule(A, b, max_ratio, max_ratio_refined, steps=REFINE_STEPS):
    """The acceptance rule of spd_solve_regs_impl<NN, true> restated in float64, the residual of every step exact.
    Returns (accepted, corrections taken, x)."""
    L, d = ldlt_unpivoted(A)
    pos = bool(np.all(d > 0))
    x = ldlt_apply(L, d, b)
    if not pos:
        return False, 0, x
    dmax, dmin = d.max(), d.min()
    if dmax <= max_ratio * dmin:
        return True, 0, x
    if not dmax <= max_ratio_refined * dmin:
        return False, 0, x
    rho = 1.0
    for step in range(steps):
        dv = ldlt_apply(L, d, exact_residual(A, b, x))
        x = x + dv
        dn, xn = np.abs(dv).max(), np.abs(x).max()
        if step == 0:
            with np.errstate(all="ignore"):
                q = 10.0 * dn / xn
            rho = min(1.0, max(q, (dmax / dmin) * EPS) if q == q else (dmax / dmin) * EPS)
        if dn * rho <= 1e-13 * xn:
            return True, step + 1, x
    return False, steps, x


# ---------------------------------------------------------------------------------------------------------------- references (mpmath)
def _mp_ldlt(A, b):
    """Unpivoted LDL^T of the stored matrix at MP_DIGITS: (pivots until the first non-positive one, x or None)."""
    import mpmath as mp
    n = A.shape[0]
    with mp.workdps(MP_DIGITS):
        M = [[mp.mpf(float(A[i, j])) for j in range(i + 1)] for i in range(n)]  # lower triangle, M[i][j], j <= i
        y = [mp.mpf(float(v)) for v in b]
        piv = []
        for k in range(n):
            d = M[k][k]
            piv.append(d)
            if not d > 0:
                return [float(p) for p in piv], None
            raw = [M[i][k] for i in range(k + 1, n)]  # d_k l_ik
            for a, i in enumerate(range(k + 1, n)):
                l = raw[a] / d
                if l != 0:
                    Mi = M[i]
                    for j in range(k + 1, i + 1):
                        Mi[j] -= l * raw[j - k - 1]
                    y[i] -= l * y[k]
                M[i][k] = l
        w = [y[k] / piv[k] for k in range(n)]
        for k in range(n - 1, 0, -1):
            wk = w[k]
            for j in range(k):
                w[j] -= M[k][j] * wk
        # the reference checks itself: the residual of the stored system at working precision
        res = max(abs(mp.mpf(float(b[i])) - mp.fsum(mp.mpf(float(A[i, j])) * w[j] for j in range(n))) for i in range(n))
        scale = max(abs(mp.mpf(float(v))) for v in b)
        assert scale == 0 or res <= scale * mp.mpf(10) ** (-(MP_DIGITS - 20)), (float(res), float(scale))
        return [float(p) for p in piv], np.array([float(v) for v in w])


def _mp_solve(A, b):
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        x = mp.lu_solve(mp.matrix(A.tolist()), mp.matrix([float(v) for v in b]))
        return np.array([float(v) for v in x])


def _mp_min_norm(J, x0):
    """J^T (J J^T)^-1 J x0 for an integer J of full row rank: the minimum-norm solution of (J^T J) x = (J^T J) x0."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        Jm = mp.matrix(J.tolist())
        z = mp.lu_solve(Jm * Jm.T, Jm * mp.matrix([float(v) for v in x0]))
        x = Jm.T * z
        return np.array([float(v) for v in x])


def _mp_spectral(Q, lam, b, thr):
    """sum over |lam_j| >= thr of q_j (q_j . b) / (lam_j |q_j|^2) for exactly orthogonal columns q_j (not normalised)."""
    import mpmath as mp
    n = Q.shape[0]
    with mp.workdps(MP_DIGITS):
        x = [mp.mpf(0)] * n
        for j in range(n):
            if abs(lam[j]) >= thr and lam[j] != 0:
                q = [mp.mpf(float(v)) for v in Q[:, j]]
                c = mp.fsum(q[i] * mp.mpf(float(b[i])) for i in range(n)) / (mp.mpf(float(lam[j])) * mp.fsum(v * v for v in q))
                x = [x[i] + q[i] * c for i in range(n)]
        return np.array([float(v) for v in x])


def _mp_eigsy_truncated(A, b):
    """Truncated pseudo-inverse solution from mpmath's eigendecomposition of the stored matrix; also the eigenvalues."""
    import mpmath as mp
    n = A.shape[0]
    with mp.workdps(MP_DIGITS):
        E, Q = mp.eigsy(mp.matrix(A.tolist()))
        lam = [E[j] for j in range(n)]
        thr = n * mp.mpf(EPS) * max(abs(v) for v in lam)
        x = [mp.mpf(0)] * n
        for j in range(n):
            if abs(lam[j]) >= thr:
                c = mp.fsum(Q[i, j] * mp.mpf(float(b[i])) for i in range(n)) / lam[j]
                x = [x[i] + Q[i, j] * c for i in range(n)]
        return np.array([float(v) for v in x]), np.array([float(v) for v in lam])


def reference(s):
    """dict: x (None where the system has no solution to claim), pivots, pos, ratio, kappa, kappa_s, and for positive definite
    systems the restated refinement rule's verdict for the gates (0, 1e13).  Cached per matrix."""
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, s.key() + ".npz")
    if os.path.exists(path):
        z = np.load(path, allow_pickle=False)
        out = {k: z[k] for k in z.files}
        out["x"] = out["x"] if out["has_x"] else None
        for k in ("pos", "ratio", "kappa", "kappa_s", "refine_ok", "refine_steps", "has_x"):
            out[k] = out[k].item()
        return out
    A, b, n = s.A, s.b, s.n
    out = dict(pivots=np.zeros(0), pos=False, ratio=float("inf"), kappa=float("nan"), kappa_s=float("nan"), refine_ok=False, refine_steps=0)
    x = None
    if s.kind == "spd":
        piv, x = _mp_ldlt(A, b)
        assert x is not None, s.name
        out.update(pivots=np.array(piv), pos=True, ratio=max(piv) / min(piv))
    elif s.kind == "refuse":  # no solution to claim: the pivots up to the first non-positive one
        if np.all(np.isfinite(A)):
            piv, xx = _mp_ldlt(A, b)
            assert xx is None, s.name
            out.update(pivots=np.array(piv))
    elif s.kind == "general":  # nonsingular, not positive definite
        x = _mp_solve(A, b)
    elif s.kind == "min_norm":
        x = _mp_min_norm(s.meta["J"], s.meta["x0"])
    elif s.kind == "spectral":
        x = _mp_spectral(s.meta["Q"], s.meta["lam"], b, n * EPS * np.abs(s.meta["lam"]).max())
    elif s.kind == "eigsy":
        x, lam = _mp_eigsy_truncated(A, b)
        out["lam"] = lam
        thr = n * EPS * np.abs(lam).max()  # the rank of the matrix AS STORED is unambiguous: nothing within 100x of the threshold
        assert all(abs(v) >= 100 * thr or abs(v) <= thr / 100 for v in lam), (s.name, sorted(np.abs(lam) / thr)[:4])
        assert sum(abs(v) >= thr for v in lam) == s.meta["rank"], s.name
    else:
        raise ValueError(s.kind)
    if s.kind in ("spd", "general", "min_norm", "spectral", "eigsy") and np.all(np.isfinite(A)):
        # kappa: largest / smallest kept eigenvalue (float64 eigvalsh: the smallest one is good to ~n eps kappa relative, 13 % at
        # the far end of the families here -- a bound, not a measurement); families with a known spectrum use it
        lam = np.abs(s.meta["lam"]) if "lam" in s.meta else np.abs(out["lam"]) if "lam" in out else np.abs(np.linalg.eigvalsh(A))
        keep = lam[lam >= n * EPS * lam.max()]
        if s.kind == "min_norm":
            keep = np.sort(lam)[::-1][:s.meta["rank"]]
        out["kappa"] = float(keep.max() / keep.min())
    if s.kind == "spd":
        dd = np.sqrt(np.diag(A))
        # (scaled by powers of two or not: the same H up to rounding)
        out["kappa_s"] = float(np.linalg.cond(A / np.outer(dd, dd)))
        ok, steps, _ = refine_rule(A, b, 0.0, REFINED_RATIO)
        out.update(refine_ok=ok, refine_steps=steps)
    out["has_x"] = x is not None
    out["x"] = x if x is not None else np.zeros(n)
    np.savez(path, **{k: np.asarray(v) for k, v in out.items()})
    out["x"] = x
    return out


# ---------------------------------------------------------------------------------------------------------------- generators
def hadamard(n):
    """A Hadamard matrix of order 12 * 2^k (Paley's construction for q = 11, Sylvester's doubling): H H^T = n I, entries +-1."""
    q = 11
    res = {(i * i) % q for i in range(1, q)}
    chi = lambda a: 0 if a % q == 0 else (1 if a % q in res else -1)
    S = np.zeros((12, 12))
    S[0, 1:] = 1
    S[1:, 0] = -1
    for i in range(q):
        for j in range(q):
            S[1 + i, 1 + j] = chi(i - j)
    H = S + np.eye(12)
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    assert H.shape[0] == n and np.array_equal(H @ H.T, n * np.eye(n))
    return H


def _tune(make, lo, hi, target, iters=60):
    """Bisect the family parameter until the float64 pivot ratio meets the target (the ratio grows with the parameter)."""
    if not pivot_ratio(make(hi)) >= target:
        return None  # the family does not reach this ratio at this size (recorded in profiles/r08_solver_accuracy.txt)
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        if pivot_ratio(make(mid)) < target:
            lo = mid
        else:
            hi = mid
    return make(0.5 * (lo + hi))


def _decade_target(dec):
    return float(np.sqrt(dec[0] * dec[1])) if dec[0] > 1e2 else 1e6


UNPOPULATED = []  # family / decade / size combinations the generators cannot reach


def dense_systems():
    """The dense positive definite families at every stand-in size."""
    out = []
    for n in STANDIN_SIZES:
        m = n + 8
        rng = np.random.default_rng(1000 + n)
        J0 = rng.uniform(-0.5, 0.5, (m, n))
        x0 = rng.uniform(-1, 1, n)
        out.append(System("well_n%d" % n, "well", J0.T @ J0, (J0.T @ J0) @ x0, decade=None))
        perm = (7 * np.arange(n)) % n / (n - 1.0)
        u = rng.integers(-7, 8, m).astype(float)
        small = rng.integers(-7, 8, (m, n)).astype(float)
        Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
        for di, dec in enumerate(DECADES):
            tgt = _decade_target(dec)

            def graded(g):
                J = J0 * 10.0 ** (-g * perm)
                return J.T @ J

            def neardep(t):
                J = np.outer(u, np.ones(n)) * 2.0 ** t + small
                return J.T @ J

            def spectrum(p):
                A = (Q * np.logspace(0, -p, n)) @ Q.T
                return 0.5 * (A + A.T)

            for fam, make, hi in (("graded", graded, 8.0), ("neardep", neardep, 24.0), ("spectrum", spectrum, 15.0)):
                A = _tune(make, 0.0, hi, tgt)
                if A is None:
                    UNPOPULATED.append("%s_d%d_n%d" % (fam, di, n))
                    continue
                out.append(System("%s_d%d_n%d" % (fam, di, n), fam, A, A @ x0, decade=di))
        # LM-shaped: translation block ~1e1, rotation block ~1e4, the diagonal damped by (1 + 1 / radius)
        Jl = rng.normal(size=(400, n)) * np.where(np.arange(n) % 6 < 3, 1.0, 60.0)
        g = Jl.T @ rng.normal(size=400)
        for radius in (1e4, 1.0, 1e-4):
            Hd = Jl.T @ Jl
            Hd[np.diag_indices(n)] *= 1 + 1 / radius
            out.append(System("lm_r%g_n%d" % (radius, n), "lm", Hd, g, decade=None))
    return out


def rank_deficient_systems():
    """A = J^T J, J integer with m < n rows, b = A x0: exact in doubles; reference J^T (J J^T)^-1 J x0.  And systems with knots no
    frame touches (zero rows and columns)."""
    out = []
    for n in (12, 24, 36, 48, 72, 96):
        for defect in (1, 6, n // 2):
            rng = np.random.default_rng(2000 + 10 * n + defect)
            m = n - defect
            J = rng.integers(-3, 4, (m, n)).astype(float)
            assert np.linalg.matrix_rank(J) == m
            x0 = rng.integers(-3, 4, n).astype(float)
            A = J.T @ J
            out.append(System("rankdef_n%d_k%d" % (n, defect), "rankdef", A, A @ x0, kind="min_norm", J=J, x0=x0, rank=m))
    for n, free in ((24, 6), (36, 12), (48, 6), (96, 12)):
        rng = np.random.default_rng(2500 + n)
        k = n - free
        # the untouched knot sits in the middle (rows / columns k0 .. k0 + free - 1)
        k0 = 6 * ((n // 6) // 2)
        idx = np.r_[0:k0, k0 + free:n]
        J = np.zeros((k - 6, n))
        J[:, idx] = rng.integers(-3, 4, (k - 6, k)).astype(float)
        assert np.linalg.matrix_rank(J) == k - 6
        x0 = np.zeros(n)
        x0[idx] = rng.integers(-3, 4, k)
        A = J.T @ J
        out.append(System("untouched_rankdef_n%d" % n, "untouched", A, A @ x0, kind="min_norm", J=J, x0=x0, rank=k - 6,
                          untouched=np.arange(k0, k0 + free)))
    return out


def untouched_spd_systems(dense):
    """An LM-shaped positive definite block with an untouched knot: full rank on its block, zero rows and columns elsewhere."""
    out = []
    by_name = {s.name: s for s in dense}
    for nb, n in ((18, 24), (30, 36), (42, 48)):
        blk = by_name["lm_r1_n%d" % nb]
        k0 = 6
        idx = np.r_[0:k0, k0 + n - nb:n]
        A = np.zeros((n, n))
        A[np.ix_(idx, idx)] = blk.A
        b = np.zeros(n)
        b[idx] = blk.b
        out.append(System("untouched_lm_n%d" % n, "untouched", A, b, kind="embedded", block=blk, idx=idx,
                          untouched=np.arange(k0, k0 + n - nb)))
    return out


def threshold_systems():
    """Prescribed spectra around the rank threshold n eps lambda_max, exact in doubles: A = H diag(s) H^T with H a Hadamard
    matrix (eigenvalues n s_j, eigenvectors the columns of H) and s_j on a dyadic grid coarse enough for every sum to be exact.
    The nearest eigenvalue is >= 100x above the threshold or exactly zero; `eigsy` cases follow the host test's pattern
    (random Q, 1e-12 / 1e-18) and take their reference and their separation from mpmath.eigsy on the stored matrix."""
    out = []
    for n in (12, 24, 48, 96):
        H = hadamard(n)
        rng = np.random.default_rng(3000 + n)
        grid = 2.0 ** -44
        above = 2.0 ** np.ceil(np.log2(100 * n * EPS))  # relative to the largest eigenvalue (s = 1)
        assert above >= 100 * n * EPS and above % grid == 0
        for lows in ((above,), (above, 0.0), (above, 2 * above, 0.0, 0.0)):
            s = np.r_[np.round(np.logspace(0, -6, n - len(lows)) / grid) * grid, lows]
            lam = n * s
            A = (H * s) @ H.T
            import mpmath as mp
            with mp.workdps(MP_DIGITS):  # the construction is exact: every entry equals the sum in exact arithmetic
                i, j = int(rng.integers(n)), int(rng.integers(n))
                assert mp.fsum(mp.mpf(float(H[i, k])) * mp.mpf(float(s[k])) * mp.mpf(float(H[j, k])) for k in range(n)) == mp.mpf(float(A[i, j]))
            assert np.array_equal(A, A.T)
            thr = n * EPS * lam.max()
            assert all(v == 0 or v >= 100 * thr for v in lam)
            b = rng.integers(-8, 9, n).astype(float)
            out.append(System("threshold_n%d_z%d" % (n, lows.count(0.0)), "threshold", A, b, kind="spectral", Q=H, lam=lam,
                              rank=int(np.count_nonzero(lam))))
    for n, lows in ((24, (1e-12, 1e-18)), (24, (1e-12, 1e-18, 1e-19)), (48, (1e-11, 1e-18))):
        rng = np.random.default_rng(3500 + n + len(lows))
        Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
        s = np.r_[np.logspace(0, -6, n - len(lows)), lows] * 37.0
        A = (Q * s) @ Q.T
        A = 0.5 * (A + A.T)
        out.append(System("threshold_eigsy_n%d_%d" % (n, len(lows)), "threshold", A, rng.uniform(-1, 1, n), kind="eigsy",
                          rank=n - len(lows) + 1))
    return out


def _diag_system(name, d, b=None, blocks=(), kind="spd", **meta):
    n = len(d)
    A = np.diag(np.asarray(d, dtype=np.float64))
    for i, blk in blocks:
        A[i:i + 2, i:i + 2] = blk
    return System(name, "gate", A, np.ones(n) if b is None else b, kind=kind, **meta)


def gate_systems():
    """Diagonal and block-diagonal systems whose unpivoted pivots are exact: the verdict of the gates is known, not computed."""
    out = []
    up = lambda v: float(np.nextafter(v, np.inf))
    for n in STANDIN_SIZES:
        rng = np.random.default_rng(4000 + n)

        def diag(dmin, dmax, where):
            d = dmin * np.exp2(rng.integers(0, 20, n).astype(float))  # between the two ends, exact
            d[where % n] = dmin
            d[(where + n // 2) % n] = dmax
            return d

        for tag, gate in (("fast", FAST_RATIO), ("refined", REFINED_RATIO)):
            for dmin in (1.0, 0.75):
                # gate * dmin is exact (0.75 = 3/4: 3e8 / 4 and 3e13 / 4 are integers below 2^53)
                out.append(_diag_system("gate_%s_at_%g_n%d" % (tag, dmin, n), diag(dmin, gate * dmin, n // 3), exact_ratio=gate, side="at", gate=tag))
                out.append(_diag_system("gate_%s_above_%g_n%d" % (tag, dmin, n), diag(dmin, up(gate * dmin), n // 3 + 1), exact_ratio=up(gate), side="above", gate=tag))
        # a 2 x 2 block [[4, 2], [2, 2]]: pivots 4 and 2 - 2 (2 / 4) = 1, every step exact
        d = diag(1.0, FAST_RATIO, 0)
        d[2] = d[3] = 1.0
        out.append(_diag_system("gate_block_at_n%d" % n, d, blocks=((2, [[4.0, 2.0], [2.0, 2.0]]),), exact_ratio=FAST_RATIO, side="at", gate="fast"))
        ones = np.exp2(rng.integers(0, 10, n).astype(float))
        for tag, i, blk in (("zero_pivot", n - 2, [[1.0, 1.0], [1.0, 1.0]]), ("indefinite_block", n - 2, [[1.0, 2.0], [2.0, 1.0]]),
                            ("zero_diagonal", n // 2, [[0.0, 0.0], [0.0, 1.0]]), ("negative_diagonal", n // 2, [[-1.0, 0.0], [0.0, 1.0]])):
            out.append(_diag_system("gate_%s_n%d" % (tag, n), ones, blocks=((i, blk),), kind="refuse", side="refuse"))
        for tag, (i, j) in (("nan_diagonal", (n - 1, n - 1)), ("nan_offdiagonal", (n - 1, 1))):
            s = _diag_system("gate_%s_n%d" % (tag, n), ones, kind="refuse", side="refuse")
            s.A[i, j] = s.A[j, i] = np.nan
            out.append(s)
        # pivot_reciprocal's contract: 1 / d correctly rounded -- x_i = 1 / d_i to the bit on a diagonal system
        d = rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-12, 13, n).astype(float))
        out.append(_diag_system("gate_reciprocal_n%d" % n, d, exact_ratio=float(d.max() / d.min()), side="below", gate="fast", bitwise=1.0 / d))
    return out


def zero_rhs_and_scaled(dense):
    """b = 0, and the whole system times 2^+-200."""
    out = []
    by_name = {s.name: s for s in dense}
    for n in STANDIN_SIZES:
        for base in ("lm_r1_n%d" % n, "graded_d1_n%d" % n):
            s = by_name[base]
            out.append(System("zero_rhs_" + base, "zero_rhs", s.A, np.zeros(n), decade=s.meta["decade"]))
        for base in ("well_n%d" % n, "lm_r1_n%d" % n, "graded_d1_n%d" % n):
            s = by_name[base]
            for e in (200, -200):
                out.append(System("scaled_%+d_%s" % (e, base), "scaled", np.ldexp(s.A, e), np.ldexp(s.b, e), base=s, decade=s.meta["decade"]))
    return out


def general_systems():
    """Nonsingular but indefinite: eig_solve's plain path (x = A^-1 b, every |eigenvalue| far above the threshold)."""
    out = []
    for n in (12, 24, 48):
        rng = np.random.default_rng(5000 + n)
        Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
        lam = np.linspace(1.0, 4.0, n) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
        A = (Q * lam) @ Q.T
        out.append(System("indefinite_n%d" % n, "indefinite", 0.5 * (A + A.T), rng.uniform(-1, 1, n), kind="general"))
    return out


def large_systems():
    """Well conditioned and graded (cond ~1e9) positive definite systems at the sizes only the Jacobi SVD and the pivoted LDL^T
    take: 11 .. 16 control knots."""
    out = []
    for n in LARGE_SIZES:
        rng = np.random.default_rng(6000 + n)
        J0 = rng.uniform(-0.5, 0.5, (n + 8, n))
        x0 = rng.uniform(-1, 1, n)
        out.append(System("well_n%d" % n, "well", J0.T @ J0, (J0.T @ J0) @ x0, decade=None))
        J = J0 * 10.0 ** (-4.5 * ((7 * np.arange(n)) % n) / (n - 1.0))
        out.append(System("graded_n%d" % n, "graded", J.T @ J, (J.T @ J) @ x0, decade=None))
    return out


_ALL = None


def all_systems():
    global _ALL
    if _ALL is None:
        dense = dense_systems()
        _ALL = dict(dense=dense, rankdef=rank_deficient_systems(), untouched_spd=untouched_spd_systems(dense), threshold=threshold_systems(),
                    gate=gate_systems(), extra=zero_rhs_and_scaled(dense), general=general_systems(), large=large_systems())
    return _ALL


def standin_forms(n):
    return ("regs",) if n in REG_SIZES else ("coop64", "coop256")


GATE_PAIRS = ((FAST_RATIO, 0.0), (FAST_RATIO, REFINED_RATIO), (0.0, REFINED_RATIO))  # plain, production, refinement of everything


def all_runs():
    S = all_systems()
    runs = []
    for s in S["dense"] + S["gate"] + S["extra"]:
        for form in standin_forms(s.n):
            for mr, mrr in GATE_PAIRS:
                runs.append(Run(s, form, mr, mrr))
    for s in S["dense"] + S["extra"]:
        if s.family == "zero_rhs" or (s.family != "scaled" and s.meta.get("decade") == 3):
            continue  # (the Jacobi forms: up to a pivot ratio of 1e12 -- kappa itself is known to 13 % there)
        for form in ("svd", "eig", "ldlt"):
            if form != "eig" or s.n <= EIG_MAX_N:
                runs.append(Run(s, form))
    for s in S["rankdef"] + S["untouched_spd"] + S["threshold"]:
        for form in ("svd", "eig"):
            if form != "eig" or s.n <= EIG_MAX_N:
                runs.append(Run(s, form))
    for s in S["large"]:
        runs.append(Run(s, "svd"))
        runs.append(Run(s, "ldlt"))
    for s in S["general"]:
        runs.append(Run(s, "eig"))
        runs.append(Run(s, "ldlt"))
    return runs


# ---------------------------------------------------------------------------------------------------------------- file format
def write_cases(path, runs):
    with open(path, "wb") as f:
        np.array([MAGIC, len(runs)], dtype="<i8").tofile(f)
        for r in runs:
            s = r.system
            np.array([s.n, FORMS[r.form]], dtype="<i8").tofile(f)
            np.array([r.max_ratio, r.max_ratio_refined], dtype="<f8").tofile(f)
            np.asfortranarray(s.A).ravel(order="F").astype("<f8").tofile(f)
            s.b.astype("<f8").tofile(f)


def read_results(path, runs):
    """list of dict(x, ok, info, err) per run that was started, and the header (cases run, stopping error, its case)."""
    w = np.fromfile(path, dtype="<i8")
    assert w[0] == MAGIC, "not a result file"
    head = dict(done=int(w[1]), error=int(w[2]), error_case=int(w[3]))
    out, p = [], 4
    for r in runs[:head["done"]]:
        n = r.system.n
        assert w[p] == n
        out.append(dict(ok=bool(w[p + 1]), info=int(w[p + 2]), err=int(w[p + 3]), x=w[p + 4:p + 4 + n].view("<f8").copy()))
        p += 4 + n
    assert p == len(w)
    return out, head


# ---------------------------------------------------------------------------------------------------------------- bounds and verdicts
def system_reference(s):
    """reference() with the derived kinds resolved: an embedded block's reference spread over its rows, a scaled system's from
    its base (x is the same, the pivots scale exactly)."""
    if s.kind == "embedded":
        ref = dict(reference(s.meta["block"]))
        x = np.zeros(s.n)
        x[s.meta["idx"]] = ref["x"]
        ref["x"] = x
        return ref
    if s.family == "scaled":
        return reference(s.meta["base"])
    return reference(s)


def scaled_error_ratio(s, ref, x):
    """max_i sqrt(a_ii) |x_i - x*_i| / (n eps kappa_s max_i sqrt(a_ii) |x*_i|); 0 where both sides vanish."""
    A = s.meta["block"].A if s.kind == "embedded" else s.A
    xs, xr = (x[s.meta["idx"]], ref["x"][s.meta["idx"]]) if s.kind == "embedded" else (x, ref["x"])
    dd = np.sqrt(np.diag(A))
    num, den = np.abs(dd * (xs - xr)).max(), A.shape[0] * EPS * ref["kappa_s"] * np.abs(dd * xr).max()
    return 0.0 if num == 0 else float(num / den)


def kappa_error_ratio(s, ref, x):
    """max |x - x*| / (n eps kappa max |x*|), kappa = largest / smallest kept eigenvalue."""
    num, den = np.abs(x - ref["x"]).max(), s.n * EPS * ref["kappa"] * np.abs(ref["x"]).max()
    return 0.0 if num == 0 else float(num / den)


def expected_plain_verdict(s, ref, max_ratio):
    """True / False: the verdict `every pivot positive and dmax <= max_ratio dmin` is required; None: the ratio sits next to the gate."""
    if s.meta.get("side") == "refuse":
        return False
    if "exact_ratio" in s.meta:  # exactly known pivots: the verdict at the gate itself is required (<=)
        return s.meta["exact_ratio"] <= max_ratio
    if not ref["pos"]:
        return False
    if max_ratio > 0 and abs(ref["ratio"] / max_ratio - 1.0) <= GATE_MARGIN:
        return None
    return ref["ratio"] <= max_ratio


def must_accept_refined(s, ref):
    """The refinement must converge: pivot ratio in (1e8, 1e12] and the float64 restatement of the rule, its residuals exact, accepts."""
    return bool(s.kind == "spd" and "exact_ratio" not in s.meta and ref["pos"] and FAST_RATIO < ref["ratio"] <= 1e12 and ref["refine_ok"])


def decade_of(ratio):
    for i, (lo, hi) in enumerate(DECADES):
        if lo < ratio <= hi:
            return i
    return None
