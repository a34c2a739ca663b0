"""numpy restatement of mbavo_pairs_report (include/mbavo.h): the shift matrix A, info_unit, sigma2, cov, the chi statistic and the
flags, from a packed frame block, the pair's knots, its level-0 patch costs and its in-bounds pixel count.  Every step is written
as the header states it; where the header fixes an order of operations (the rotation matrix of a knot, (K P) as a double product,
((2 cost) (K P)) / max(..)) the same order is used here, so A and sigma2 can be held to the device tightly."""
import numpy as np

E_RANGE, SINGULAR = -2, 1
U = 2.0 ** -53


def packed_len(k):
    nd = 6 * k + 1
    return nd * (nd + 1) // 2


def rotation(q):
    """Rotation matrix of the quaternion (x, y, z, w) divided by its norm."""
    q = np.asarray(q, np.float64)
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    x, y, z, w = q[0] / n, q[1] / n, q[2] / n, q[3] / n
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                     [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                     [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]])


def hat(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def shift_matrix(kt, kR):
    """A (6k x 6): the local parameters [dt_0 .. dt_{k-1} | dw_0 .. dw_{k-1}] of the rigid shift xi = (v, w) of the k knots
    (kt k x 3, kR k x 4): dt_i = v - [t_i]x w, dw_i = R_i^T w."""
    kt, kR = np.asarray(kt, np.float64).reshape(-1, 3), np.asarray(kR, np.float64).reshape(-1, 4)
    k = len(kt)
    A = np.zeros((6 * k, 6))
    for i in range(k):
        A[3 * i:3 * i + 3, :3] = np.eye(3)
        A[3 * i:3 * i + 3, 3:] = -hat(kt[i])
        A[3 * k + 3 * i:3 * k + 3 * i + 3, 3:] = rotation(kR[i]).T
    return A


def unpack(block, k):
    """(cost, g_local, H_local both triangles) of a packed frame block [cost | g | upper(H)]."""
    m = 6 * k
    block = np.asarray(block, np.float64)
    H = np.zeros((m, m))
    iu = np.triu_indices(m)
    H[iu] = block[1 + m:]
    H = H + np.triu(H, 1).T
    return float(block[0]), block[1:1 + m].copy(), H


def info_unit(H, A, K, P):
    return (float(K) * float(P)) * (A.T @ (H @ A))


def info_bound(H, A, K, P):
    """Elementwise bound on the rounding error of info_unit: a dot product of 6k terms inside one of 6k terms and the scale, n =
    2 6k + 2 roundings at most per entry: gamma_n (|A|^T |H| |A|) (K P)."""
    n = 2 * A.shape[0] + 2
    gamma = n * U / (1.0 - n * U)
    return gamma * (np.abs(A).T @ (np.abs(H) @ np.abs(A))) * (float(K) * float(P))


def sigma2(cost, K, P, valid):
    return ((2.0 * cost) * (float(K) * float(P))) / max(valid - 6.0, 1.0)


def cov(info, s2, dtype=np.float64):
    """sigma2 info^-1 through a Cholesky factorisation in `dtype` (np.longdouble: the high-precision reference; numpy's linalg
    does not take it, so the factorisation is written out).  None where a pivot is not finite or <= 0."""
    a = np.asarray(info, dtype)
    n = a.shape[0]
    L = np.zeros((n, n), dtype)
    for j in range(n):
        d = a[j, j] - (L[j, :j] * L[j, :j]).sum(dtype=dtype)
        if not (d > 0) or not np.isfinite(d):
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (a[i, j] - (L[i, :j] * L[j, :j]).sum(dtype=dtype)) / L[j, j]
    Li = np.zeros((n, n), dtype)
    for c in range(n):
        Li[c, c] = dtype(1) / L[c, c]
        for i in range(c + 1, n):
            Li[i, c] = -(L[i, c:i] * Li[c:i, c]).sum(dtype=dtype) / L[i, i]
    return dtype(s2) * (Li.T @ Li)


def statistic(costs, chi):
    """(mu, var, bound, flags, num_stat) of detectOutliersAndUploadToGpu on the patch costs."""
    c = np.asarray(costs, np.float64)
    keep = ~(c < 1e-8)
    n = int(keep.sum())
    if n == 0:
        return float("nan"), float("nan"), float("nan"), np.zeros(len(c), np.uint8), 0
    mu = c[keep].sum() / n
    var = ((c[keep] - mu) ** 2).sum() / n
    bound = chi * float(np.sqrt(np.float32(var)))
    return mu, var, bound, (np.abs(c - mu) > bound).astype(np.uint8), n


def near_the_bound(costs, mu, bound, K):
    """Keypoints whose |cost - mu| lies within K 2^-52 relative of the bound: the only ones whose flag may depend on the order the
    sums ran in."""
    c = np.asarray(costs, np.float64)
    return np.abs(np.abs(c - mu) - bound) <= K * 2.0 ** -52 * bound


def report(block, kt, kR, costs, valid, K, P, k, chi):
    """The record of one pair with its capture time on the knots kt, kR (the k knots of its segment)."""
    cost, g, H = unpack(block, k)
    A = shift_matrix(kt, kR)
    info = info_unit(H, A, K, P)
    s2 = sigma2(cost, K, P, valid)
    c = cov(info, s2) if K > 0 else None
    mu, var, bound, flags, n = statistic(costs, chi)
    return dict(status=0 if c is not None else SINGULAR, A=A, H=H, g=g, cost=cost, info_unit=info, sigma2=s2,
                cov=np.full((6, 6), np.nan) if c is None else c, mu=mu, var=var, bound=bound, flags=flags, num_stat=n,
                num_flagged=int(flags.sum()))
