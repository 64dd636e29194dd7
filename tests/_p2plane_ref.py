"""fp64 numpy restatement of the opt-in normal estimation and point-to-plane ICP (csrc/icp.hip:
pk_estimate_normals, pk_icp_plane_*), i.e. of Open3D 0.17 estimate_normals(KDTreeSearchParamKNN)
+ orient_normals_towards_camera_location and registration_icp(...,
TransformationEstimationPointToPlane()). Open3D is not installed here: parity unpinned against
Open3D, like the rest of the f4 row; this file pins the semantics the kernels implement.

  * neighbours: brute force, stable argsort on d^2 = (dx dx + dy dy) + dz dz, so ties go to the
    lowest index and the order is (d^2, index); the point itself is its first neighbour;
  * covariance: of the neighbours minus the query point, C = S2 / m - mean mean^T, summed in
    neighbour order (order="rev": reversed — the second summation order the tolerances are
    measured with; in icp_ref it reverses every sum: over the pairs, in T s and in U T); normal = eigh's eigenvector of the smallest eigenvalue, flipped so that
    n . (viewpoint - p) >= 0; fewer than 3 neighbours: (0, 0, 1), not flipped;
  * ICP: the loop of csrc/icp.hip (evaluate, stop test, update, T <- U T with the accumulated T
    applied to the source), nearest target by exact distance (ties: lowest index), pair iff
    d^2 < r^2, rows J = [p x n, n], r = (p - q) . n in coordinates shifted by the first target
    point, J^T J x = -J^T r by Cholesky (a non-positive pivot: U = I),
    U = [Rz(x2) Ry(x1) Rx(x0) | x3..5], conjugated back.
"""
import numpy as np


def knn_brute(P, k):
    """[n,3] -> int32 [n,k]: the k nearest points of each point, itself included, ordered by
    (d^2, index); -1 past the cloud's size."""
    n = P.shape[0]
    out = np.full((n, k), -1, np.int32)
    if n == 0:
        return out
    d = P[:, None, :] - P[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    kk = min(k, n)
    out[:, :kk] = np.argsort(d2, axis=1, kind="stable")[:, :kk]
    return out


def cov_ref(P, k=30, order="seq", knn=None):
    """[n,3,3]: the covariance of each point's min(k, n) neighbours about the point itself,
    C = S2 / m - mean mean^T, summed in neighbour order (order="rev": reversed)."""
    kk = min(k, P.shape[0])
    nb = (knn_brute(P, k) if knn is None else knn)[:, :kk]
    E = P[nb] - P[:, None, :]                      # [n, kk, 3]
    if order == "rev":
        E = E[:, ::-1]
    s = np.cumsum(E, axis=1)[:, -1]                # sequential sums
    S2 = np.cumsum(E[:, :, :, None] * E[:, :, None, :], axis=1)[:, -1]
    m = s / kk
    return S2 / kk - m[:, :, None] * m[:, None, :]


def normals_ref(P, k=30, viewpoint=(0.0, 0.0, 0.0), order="seq", knn=None):
    """-> (normals [n,3], gap [n] = (l1 - l0) / l2 of the covariance's ascending eigenvalues;
    inf where the normal is the fixed (0,0,1))."""
    n = P.shape[0]
    nrm = np.zeros((n, 3))
    nrm[:, 2] = 1.0
    gap = np.full(n, np.inf)
    if min(k, n) < 3:
        return nrm, gap
    w, V = np.linalg.eigh(cov_ref(P, k, order, knn))
    nrm = V[:, :, 0].copy()
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    flip = np.einsum("nc,nc->n", nrm, np.asarray(viewpoint, np.float64)[None] - P) < 0
    nrm[flip] *= -1
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
    return nrm, gap


def _nearest(p, tgt, chunk=1024):
    """nearest target index (ties: lowest) and its d^2 per row of p."""
    idx = np.zeros(p.shape[0], np.int64)
    d2 = np.zeros(p.shape[0])
    for a in range(0, p.shape[0], chunk):
        d = p[a:a + chunk, None, :] - tgt[None, :, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        j = np.argmin(dd, axis=1)
        idx[a:a + chunk] = j
        d2[a:a + chunk] = dd[np.arange(j.shape[0]), j]
    return idx, d2


def _seq_sum(x, order):
    """sum over axis 0, one row after the other (order="rev": from the last row)."""
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:])
    return np.cumsum(x[::-1] if order == "rev" else x, axis=0)[-1]


def _rot_zyx(a, b, g):
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _cholesky_solve(A, b):
    """x with A x = b, or None at a non-positive pivot."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0.0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


def _update_plane(p, q, n, c, order):
    a, b = p - c, q - c
    J = np.concatenate([np.cross(a, n), n], axis=1)
    r = np.einsum("nc,nc->n", a - b, n)
    A = _seq_sum(J[:, :, None] * J[:, None, :], order)
    g = _seq_sum(J * r[:, None], order)
    U = np.eye(4)
    x = _cholesky_solve(A, -g) if p.shape[0] else None
    if x is None:
        return U
    R = _rot_zyx(x[0], x[1], x[2])
    U[:3, :3] = R
    U[:3, 3] = x[3:] + c - R @ c
    return U


def _update_point(p, q, c, order):
    U = np.eye(4)
    if p.shape[0] == 0:
        return U
    a, b = p - c, q - c
    m = p.shape[0]
    ma, mb = _seq_sum(a, order) / m, _seq_sum(b, order) / m
    S = _seq_sum(a[:, :, None] * b[:, None, :], order) / m - ma[:, None] * mb[None, :]  # source x target
    Us, _, Vt = np.linalg.svd(S.T)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Us @ Vt))])
    R = Us @ D @ Vt
    t = mb - R @ ma
    U[:3, :3] = R
    U[:3, 3] = t + c - R @ c
    return U


def icp_ref(src, tgt, T0, r, max_it, estimation="point_to_plane", tgt_normals=None, rel_fit=1e-6, rel_rmse=1e-6,
            order="seq"):
    """-> (T [4,4], stats [4] = fitness, inlier rmse, updates, converged)."""
    T = np.array(T0, np.float64)
    ns, nt = src.shape[0], tgt.shape[0]
    fit_prev = rmse_prev = 0.0
    e, conv = 0, 0
    while True:
        if order == "rev":
            p = T[:3, 3] + (T[:3, 2] * src[:, 2:3] + (T[:3, 1] * src[:, 1:2] + T[:3, 0] * src[:, :1]))
        else:
            p = ((T[:3, 0] * src[:, :1] + T[:3, 1] * src[:, 1:2]) + T[:3, 2] * src[:, 2:3]) + T[:3, 3]
        if nt and ns:
            j, d2 = _nearest(p, tgt)
            ok = d2 < r * r
        else:
            j, d2, ok = np.zeros(ns, np.int64), np.zeros(ns), np.zeros(ns, bool)
        cnt = int(ok.sum())
        fit = cnt / ns if cnt and ns else 0.0
        rmse = np.sqrt(_seq_sum(d2[ok][:, None], order)[0] / cnt) if cnt else 0.0
        if e > 0 and abs(fit_prev - fit) < rel_fit and abs(rmse_prev - rmse) < rel_rmse:
            conv = 1
            break
        fit_prev, rmse_prev = fit, rmse
        if e >= max_it:
            break
        c = tgt[0] if nt else np.zeros(3)
        if estimation == "point_to_plane":
            U = _update_plane(p[ok], tgt[j[ok]], tgt_normals[j[ok]], c, order)
        else:
            U = _update_point(p[ok], tgt[j[ok]], c, order)
        terms = U[:, :, None] * T[None, :, :]            # [row, k, column]: T <- U T, summed over k
        T = _seq_sum(np.moveaxis(terms, 1, 0), order)
        e += 1
    return T, np.array([fit, rmse, float(e), float(conv)])


def pose_error(T, T_true):
    """(rotation angle in degrees, translation distance) between two poses."""
    R = T[:3, :3] @ T_true[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


def perturb(rng, T, deg, shift, center):
    """T turned by `deg` degrees about a random axis through `center` and shifted by `shift` in a
    random direction."""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    dR = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    sh = rng.normal(size=3)
    D = np.eye(4)
    D[:3, :3] = dR
    D[:3, 3] = center - dR @ center + sh / np.linalg.norm(sh) * shift
    return D @ T


def ellipsoid_case(seed=10, ns=2000, nt=1500, noise=0.02):
    """The partial-view case: source = an ellipsoid (semi-axes 5 / 3 / 2.5, object frame), target =
    its camera-facing part under the true pose (z about 90, the camera at the origin) with noise,
    start = the true pose turned by 5 degrees and shifted by 0.2; radius 0.5. The default seed is
    one where point-to-plane meets the relative stop criteria (7 updates, 0.29 degrees / 0.011 from
    the truth; point-to-point: 41 updates, 2.4 degrees / 0.12) with the same update count under
    both summation orders; on about half of the seeds 0-23 the pairs at the rim of the view keep
    flipping and point-to-plane runs to max_iteration instead.
    -> dict(src, tgt, T_true, T0, r)."""
    rng = np.random.default_rng(seed)
    axes = np.array([5.0, 3.0, 2.5])

    def surface(n):
        u = rng.normal(size=(n, 3))
        return u / np.linalg.norm(u, axis=1, keepdims=True) * axes

    from dpfm_amd.dataset.synthetic import random_rotation
    R = random_rotation(rng)
    T_true = np.eye(4)
    T_true[:3, :3] = R
    T_true[:3, 3] = np.array([0.5, -0.3, 90.0])
    src = surface(ns)
    cand = surface(6 * nt)
    nrm = cand / axes ** 2                                 # outward normal direction (object frame)
    cam = cand @ R.T + T_true[:3, 3]
    facing = np.einsum("nc,nc->n", nrm @ R.T, -cam) > 0    # the surface the camera sees
    tgt = cam[facing][:nt] + rng.normal(size=(nt, 3)) * noise
    assert tgt.shape[0] == nt
    T0 = perturb(rng, T_true, 5.0, 0.2, T_true[:3, 3])
    return dict(src=np.ascontiguousarray(src), tgt=np.ascontiguousarray(tgt), T_true=T_true, T0=T0, r=0.5)
