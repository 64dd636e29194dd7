"""numpy restatement of TEASER++ with scale estimation (steps 1-4 of the scale feature), the
reference of test_teaser_scale_cpu.py / test_teaser_scale_gpu.py. Sums run sequentially in sweep
order (np.cumsum), as TEASER's ScalarTLSEstimator does; the GNC-TLS rotation, the per-axis voting and
the clique tools are the oracle's."""
import math

import numpy as np

from oracle import dpfm_oracle as O


def planted_scaled(rng, n, inlier_frac, s, noise=0.01):
    """planted() of test_teaser_cpu.py (the same draws in the same order) with a scale:
    b = s (a R^T) + t + noise, outliers at spread 5 s around t. -> (a, b, T rigid, s)."""
    from dpfm_amd.dataset.synthetic import random_rotation
    R = random_rotation(rng)
    t = rng.normal(size=3) * 10 + np.array([0, 0, 80.0])
    a = rng.normal(size=(n, 3)) * 5
    b = s * (a @ R.T) + t + rng.normal(size=(n, 3)) * noise
    out = rng.random(n) >= inlier_frac
    b[out] = rng.normal(size=(out.sum(), 3)) * 5 * s + t
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return a, b, T, s


def _norms(x):
    d = x[None, :, :] - x[:, None, :]  # [i, j] = x_j - x_i
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def tim_matrices(a, b, beta):
    """(X [n,n], alpha [n,n], usable [n,n]) of step 1 (usable is False on the diagonal)."""
    va, vb = _norms(a), _norms(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        X = vb / va
        al = beta / va
    usable = (va != 0) & np.isfinite(X)
    return X, al, usable


def scale_vote(a, b, beta):
    """Step 2 -> dict(scale, status, card, and the per-position xh / cost / candidate mask)."""
    n = a.shape[0]
    none = dict(scale=1.0, status=0, card=0, xh=np.zeros(0), cost=np.zeros(0), cand=np.zeros(0, bool))
    if n < 2:
        return none
    Xm, am, um = tim_matrices(a, b, beta)
    iu = np.triu_indices(n, 1)  # row-major: i ascending, then j ascending
    use = um[iu]
    X, al = Xm[iu][use], am[iu][use]
    K = X.shape[0]
    if K == 0:
        return none
    keys = np.empty(2 * K)
    keys[0::2], keys[1::2] = X - al, X + al
    eps = np.empty(2 * K)
    eps[0::2], eps[1::2] = 1.0, -1.0
    Xe, ae = np.repeat(X, 2), np.repeat(al, 2)
    order = np.argsort(keys, kind="stable")
    eps, Xe, ae = eps[order], Xe[order], ae[order]
    w = 1.0 / (ae * ae)
    card = np.cumsum(eps)
    dw = np.cumsum(eps * w)
    dxw = np.cumsum(eps * w * Xe)
    rsum = np.cumsum(np.concatenate([[al.sum()], -(eps * ae)]))[1:]
    sx = np.cumsum(eps * Xe)
    sx2 = np.cumsum(eps * Xe * Xe)
    with np.errstate(divide="ignore", invalid="ignore"):
        xh = dxw / dw
        cost = (card * xh * xh + sx2 - 2 * sx * xh) + rsum
    cand = (card > 0) & np.isfinite(cost)
    if not cand.any():
        return none
    k = int(np.argmin(np.where(cand, cost, np.inf)))  # first minimum
    return dict(scale=float(xh[k]), status=1, card=int(card[k]), xh=xh, cost=cost, cand=cand, best=k)


def vote_margin(v):
    """The smallest relative cost gap between the winner and any candidate whose xh differs from
    the winner's by more than 1e-9 relative (inf when there is none)."""
    k = v["best"]
    far = v["cand"] & (np.abs(v["xh"] - v["xh"][k]) > 1e-9 * abs(v["xh"][k]))
    if not far.any():
        return math.inf
    return float((v["cost"][far].min() - v["cost"][k]) / abs(v["cost"][k]))


def scaled_graph(a, b, beta, s):
    """Step 3: edge (i, j) iff the pair is usable and |X - s| <= alpha."""
    if a.shape[0] == 0:
        return np.zeros((0, 0), bool)
    X, al, usable = tim_matrices(a, b, beta)
    with np.errstate(invalid="ignore"):
        e = usable & (np.abs(X - s) <= al)
    np.fill_diagonal(e, False)
    return e


def from_clique_scaled(a, b, clique, s, noise_bound=0.05, cbar2=1.0, gnc_factor=1.4, max_iterations=100,
                       cost_threshold=1e-12):
    """Step 4 given the sorted clique: chain TIMs, d <- d (1 / s), GNC-TLS with noise bound
    2 noise / s, translation voted over b - s (R a) -> (T rigid, rot_inl, trans_inl)."""
    C = np.asarray(clique)
    leaf = np.roll(C, -1)
    sv, d = a[leaf] - a[C], (b[leaf] - b[C]) * (1.0 / s)
    R, w = O.gnc_tls_rotation(sv, d, 2 * noise_bound / s, gnc_factor, max_iterations, cost_threshold)
    raw = b[C] - s * (a[C] @ R.T)
    t = np.zeros(3)
    inl = np.ones(C.size, bool)
    for r in range(3):
        t[r], ii = O.scalar_tls(raw[:, r], noise_bound * math.sqrt(cbar2))
        inl &= ii
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T, int((w >= 0.5).sum()), int(inl.sum())
