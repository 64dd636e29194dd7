"""fp64 restatement of ZoomOut (Melzi et al. 2019; pyFM's zoomout_refine) in the project's
convention (fmap2pointmap_solvers/naive.py:6-34: X the CAD, Y the crop), the parity target of
ops.zoomout, and a fixed generator of analytic test shapes.

    k = 30
    1. E = Phi_x[:n1, :k] C^T;  p[j] = argmin_{i < n1} (|E_i|^2 - 2 E_i . Phi_y[j, :k]), ties lowest i
    2. k == k_final: stop; else k <- min(k + step, k_final)
    3. C = Phi_y[:n2, :k]^T diag(mass_y) Phi_x[p, :k];  go to 1.
"""
import numpy as np

K0 = 30
U32 = 2.0 ** -24  # unit roundoff of f32


def scores(ex, ey, C, n1, n2, k):
    """fp64 [n1, n2]: |E_i|^2 - 2 E_i . y_j (the squared distance without its |y_j|^2)."""
    E = np.asarray(ex, np.float64)[:n1, :k] @ np.asarray(C, np.float64)[:k, :k].T
    return (E * E).sum(1)[:, None] - 2.0 * (E @ np.asarray(ey, np.float64)[:n2, :k].T)


def point_map(ex, ey, C, n1, n2, k):
    if n2 == 0:
        return np.zeros(0, np.int64)
    return scores(ex, ey, C, n1, n2, k).argmin(0)  # the first minimal i


def project(ex, ey, mass, p, n2, k):
    ex, ey, mass = (np.asarray(a, np.float64) for a in (ex, ey, mass))
    return (ey[:n2, :k] * mass[:n2, None]).T @ ex[p[:n2], :k]


def schedule(k_final, step):
    ks = [K0]
    while ks[-1] < k_final:
        ks.append(min(ks[-1] + step, k_final))
    return ks


def zoomout(ex, ey, mass, C0, n1, n2, k_final=64, step=1):
    """(C [k_final, k_final], p [n2]) of the loop above in fp64."""
    C = np.asarray(C0, np.float64)
    ks = schedule(k_final, step)
    for it, k in enumerate(ks):
        p = point_map(ex, ey, C, n1, n2, k)
        if it + 1 < len(ks):
            C = project(ex, ey, mass, p, n2, ks[it + 1])
    return C, p


# ---------------------------------------------------------------- the rectangle [0, 1] x [0, H]
H = 0.7
NMODE = 12


def rect_modes(n=64):
    """(a, b) of the first n Neumann modes cos(pi a u) cos(pi b v / H), by a^2 + (b / H)^2."""
    ab = [(a, b) for a in range(NMODE) for b in range(NMODE)]
    ab.sort(key=lambda t: t[0] ** 2 + (t[1] / H) ** 2)  # (stable: ties keep the (a, b) order)
    return np.array(ab[:n])


def rect_eigenfunctions(P, n=64):
    """fp64 [len(P), n]: the modes at the points P, orthonormal under the area measure."""
    ab = rect_modes(n)
    c = lambda m: np.where(m == 0, 1.0, 0.5)  # noqa: E731
    nrm = 1.0 / np.sqrt(c(ab[:, 0]) * c(ab[:, 1]) * H)
    return np.cos(np.pi * P[:, :1] * ab[None, :, 0]) * np.cos(np.pi * P[:, 1:] * ab[None, :, 1] / H) * nrm


def rect_case(seed, n1, n2):
    """dict of f32 inputs: X / Y independent uniform samples of the rectangle, Y's columns under
    random signs s, mass_y = H / n2, C0 = diag(s[:30]) + 0.15 N(0, 1); drawn from
    default_rng(seed) in the order X, Y, s, noise."""
    rng = np.random.default_rng(seed)
    X = rng.random((n1, 2)) * np.array([1.0, H])
    Y = rng.random((n2, 2)) * np.array([1.0, H])
    s = rng.integers(0, 2, 64) * 2.0 - 1.0
    noise = rng.standard_normal((K0, K0))
    return dict(X=X, Y=Y, s=s,
                ex=rect_eigenfunctions(X).astype(np.float32),
                ey=(rect_eigenfunctions(Y) * s[None]).astype(np.float32),
                mass=np.full(n2, H / max(n2, 1), np.float32),
                C0=(np.diag(s[:K0]) + 0.15 * noise).astype(np.float32))


def map_error(case, p):
    """mean |X[p[j]] - Y[j]|"""
    return float(np.linalg.norm(case["X"][p] - case["Y"], axis=1).mean())


# ---------------------------------------------------------------- acceptance bound of the f32 argmin
def tau(ex, ey, C, n1, n2, k):
    """tau_j (fp64 [n2]): how far above the fp64 minimum of column j the score of an f32
    evaluation's pick may lie. All quantities are fp64 functions of the (f32) inputs.

    With u = 2^-24, x_i / y_j the rows' first k entries, E = x C^T exact, A_ia = sum_b |x_ib| |C_ab|
    (|A_i| >= |E_i|: the embedding's cancellation), and the evaluation (csrc/zoomout.hip)
    E^_ia = an fmaf chain over b (on the f32 MFMA, which accumulates as one); n^_i = sum of E^_ia^2 (fmaf chains of <= 16 terms and three adds);
    s^_ij = an fmaf chain started at n^_i over the k products (-2 E^_ia) y_ja (-2 E^ is exact; the
    zero columns past k add nothing), to first order in u:
      |E^_i - E_i|            <= k u |A_i|
      |n^_i - |E^_i|^2|       <= (k / 4 + 4) u |E_i|^2
      ||E^_i|^2 - |E_i|^2|    <= 2 k u |A_i| |E_i|
      |2 (E^_i - E_i) . y_j|  <= 2 k u |A_i| |y_j|
      the score's chain       <= k u (|E_i|^2 + 2 |E_i| |y_j|)
    so |s^_ij - s_ij| <= u [((1.25 k + 4) |E_i|^2 + 2 k |A_i| |E_i|) + 2 k (|A_i| + |E_i|) |y_j|]
                      <= (k + 3) u [alpha Emax^2 + beta Emax |y_j|],   Emax = max_i |E_i|,
      alpha = max_i ((1.25 k + 4) |E_i|^2 + 2 k |A_i| |E_i|) / ((k + 3) Emax^2),
      beta  = max_i 2 k (|A_i| + |E_i|) / ((k + 3) Emax).
    The pick i' has s^_i'j <= s^_i*j for the fp64 minimiser i*, hence s_i'j - s_i*j <= the two errors:
      tau_j = c (k + 3) u (Emax^2 + Emax |y_j|),   c = 2 max(alpha, beta) * 1.01
    (the 1.01 covers the dropped second-order terms: (k + 3) u < 5e-6)."""
    x = np.asarray(ex, np.float64)[:n1, :k]
    Ck = np.asarray(C, np.float64)[:k, :k]
    y = np.asarray(ey, np.float64)[:n2, :k]
    if n1 == 0:
        return np.zeros(n2)
    En = np.linalg.norm(x @ Ck.T, axis=1)
    An = np.linalg.norm(np.abs(x) @ np.abs(Ck).T, axis=1)
    Emax = max(float(En.max()), 1e-300)
    alpha = float((((1.25 * k + 4) * En ** 2 + 2 * k * An * En) / ((k + 3) * Emax ** 2)).max())
    beta = float((2 * k * (An + En) / ((k + 3) * Emax)).max())
    c = 2.0 * max(alpha, beta) * 1.01
    return c * (k + 3) * U32 * (Emax ** 2 + Emax * np.linalg.norm(y, axis=1))


def f32_point_map(ex, ey, C, n1, n2, k):
    """numpy f32 emulation of the device's evaluation order up to summation order (f32 matmuls)."""
    E = np.asarray(ex, np.float32)[:n1, :k] @ np.asarray(C, np.float32)[:k, :k].T
    s = (E * E).sum(1, dtype=np.float32)[:, None] - np.float32(2) * (E @ np.asarray(ey, np.float32)[:n2, :k].T)
    return s.argmin(0)
