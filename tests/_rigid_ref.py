"""fp64 numpy reference of the 4-point rigid fit shared by RANSAC, ICP and TEASER (csrc/rigid.hpp:
rigid_fit4 / rigid_from_cov), the draw families on which a closed-form eigen solve goes wrong,
and the per-draw checks the CPU test applies to the reference itself and the GPU test to the
device fit.

The fit is the rotation R in SO(3) maximising sum_k (d_k - md) . R (s_k - ms), and t = md - R ms.
With S = sum_k (d_k - md)(s_k - ms)^T = U diag(sigma) V^T the maximiser is R = U diag(1, 1, sign)
V^T, sign = det(U) det(V), and the maximum is opt = sigma_1 + sigma_2 + sign sigma_3. The rotation
is determined as far as mu = (sigma_2 + sign sigma_3) / sigma_1 is away from 0: mu is half the
relative gap between the two largest eigenvalues of Horn's 4x4 N(S).

Bars (eps = 2^-52), per draw:
  1. structure: R R^T = I and det R = 1 to 64 eps, R ms + t = md to 64 eps (|ms| + |md| + 1);
  2. optimality: opt - sum_k (d_k - md) . R (s_k - ms) <= 256 eps Q,
     Q = sum_k (|s_k - ms| + u)(|d_k - md| + u), u = eps max |coordinate| (the centring rounding);
  3. rotation, families that determine it (mu >= 1e-6 on every draw): |R - R_ref| <= 1024 eps / mu,
     about 7x the reference's own sensitivity to a one-ulp change of its inputs;
  4. residual on exact data: rms |R s + t - d| <= sqrt(2 * 256 eps Q / 4) + the structural term
     (for exact data sum |R s' - d'|^2 = 2 (opt - objective), so this is 2. in RANSAC's units).
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
MU_MIN = 1e-6
PER_FAMILY = 256
# families whose d is not an exact rigid image of s (criterion 4 does not apply)
INEXACT = frozenset(["noisy", "outlier", "mirrored", "coplanar_noisy", "one_repeat_noisy"])


def _centre(s, d):
    ms, md = s.mean(1), d.mean(1)
    return ms, md, s - ms[:, None, :], d - md[:, None, :]


def umeyama_ref(s, d):
    """s, d [n,k,3] -> R [n,3,3], t [n,3], S [n,3,3], sigma [n,3], opt [n], mu [n]."""
    s = np.asarray(s, np.float64)
    d = np.asarray(d, np.float64)
    ms, md, sc, dc = _centre(s, d)
    S = np.einsum("nkr,nkc->nrc", dc, sc)
    U, sig, Vt = np.linalg.svd(S)
    sign = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0)
    D = np.ones_like(sig)
    D[:, 2] = sign
    R = np.einsum("nij,nj,njk->nik", U, D, Vt)
    t = md - np.einsum("nij,nj->ni", R, ms)
    opt = sig[:, 0] + sig[:, 1] + sign * sig[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.where(sig[:, 0] > 0, (sig[:, 1] + sign * sig[:, 2]) / sig[:, 0], 0.0)
    return R, t, S, sig, opt, mu


def sensitivity(s, d, trials=8, seed=0, centred=False):
    """[n]: max |R_ref(s~, d~) - R_ref(s, d)| over `trials` random one-ulp (relative, either
    sign) perturbations of every coordinate: the reference's own conditioning.

    centred=True perturbs the coordinates after their centroid is taken off. That is the
    yardstick for `far_centroid` only: an ulp of a coordinate near 1e6 is 2e5 ulps of the centred
    one, so the raw perturbation measures the input's quantisation (4e5 eps / mu), which a fit
    that reads the same quantised input never sees — the common offset cancels exactly in
    s_k - ms (both within a factor 2 of each other)."""
    rng = np.random.default_rng(seed)
    if centred:
        s, d = _centre(s, d)[2:]
    R0 = umeyama_ref(s, d)[0]
    worst = np.zeros(s.shape[0])
    for _ in range(trials):
        sp = s * (1.0 + EPS * rng.choice([-1.0, 1.0], size=s.shape))
        dp = d * (1.0 + EPS * rng.choice([-1.0, 1.0], size=d.shape))
        worst = np.maximum(worst, np.abs(umeyama_ref(sp, dp)[0] - R0).reshape(-1, 9).max(1))
    return worst


def quat_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def _pose(rng, n):
    return quat_rotations(rng, n), rng.normal(size=(n, 3)) * 40 + np.array([0.0, 0.0, 90.0])


def _apply(R, t, s):
    return np.einsum("nij,nkj->nki", R, s) + t[:, None, :]


def families(rng, n):
    """name -> (s [n,4,3], d [n,4,3], unique): `unique` says that every draw of the family
    determines the rotation (mu >= MU_MIN). Coordinates ~ N(0, 5^2), poses as in
    test_corr_pose_gpu.py::test_ransac_matches_c_oracle."""
    out = {}

    def pts():
        return rng.normal(size=(n, 4, 3)) * 5

    def add(name, s, unique, noise=0.0, d=None, post=None):
        R, t = _pose(rng, n)
        dd = _apply(R, t, s) if d is None else d
        if noise:
            dd = dd + rng.normal(size=dd.shape) * noise
        if post is not None:
            s, dd = post(s, dd)
        out[name] = (np.ascontiguousarray(s), np.ascontiguousarray(dd), unique)

    add("generic", pts(), True)
    add("noisy", pts(), True, noise=0.01)
    add("outlier", pts(), True, d=pts() + _pose(rng, n)[1][:, None, :])

    def mirror(s, d):
        d = d.copy()
        d[..., 0] *= -1
        return s, d
    add("mirrored", pts(), True, post=mirror)

    # 180 degrees: R = 2 a a^T - I, the first three about the coordinate axes
    a = rng.normal(size=(n, 3))
    a[:3] = np.eye(3)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    s = pts()
    R180 = 2 * a[:, :, None] * a[:, None, :] - np.eye(3)
    out["rot180"] = (s, np.ascontiguousarray(_apply(R180, _pose(rng, n)[1], s)), True)
    s = pts()
    out["identity"] = (s, s.copy(), True)
    s = pts()
    out["identity_shift"] = (s, s + _pose(rng, n)[1][:, None, :], True)

    def plane():
        p = pts()
        p[..., 2] = 0.0
        return _apply(quat_rotations(rng, n), np.zeros((n, 3)), p)
    add("coplanar", plane(), True)
    add("coplanar_noisy", plane(), True, noise=0.01)
    s = np.round(rng.normal(size=(n, 4, 3)) * 50)
    s[..., 2] = 900.0   # a fronto-parallel surface in integer-millimetre depth
    add("integer_plane", s, True)

    def repeat(pairs):
        p = pts()
        for a_, b_ in pairs:
            p[:, a_] = p[:, b_]
        return p
    add("one_repeat", repeat([(1, 0)]), True)
    add("one_repeat_noisy", repeat([(1, 0)]), True, noise=0.01)

    def thin(e):
        p = pts()
        p[..., 1:] *= e
        return p
    add("near_collinear_1e-1", thin(1e-1), True)
    add("near_collinear_1e-2", thin(1e-2), True)
    for name, f in (("scale_1e-3", 1e-3), ("scale_1e3", 1e3)):
        add(name, pts(), True, post=lambda s_, d_, f=f: (s_ * f, d_ * f))
    add("far_centroid", pts() + 1e6, True)

    add("two_distinct", repeat([(1, 0), (3, 2)]), False)
    add("all_same", repeat([(1, 0), (2, 0), (3, 0)]), False)
    u = rng.normal(size=(n, 1, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    add("collinear", rng.normal(size=(n, 1, 3)) * 5 + rng.normal(size=(n, 4, 1)) * 5 * u, False)
    add("near_collinear_1e-3", thin(1e-3), False)
    add("near_collinear_1e-6", thin(1e-6), False)
    add("near_collinear_1e-10", thin(1e-10), False)
    return out


def fit_figures(s, d, R, t):
    """Per-draw figures of a fit (R [n,3,3], t [n,3]) against the reference, with their bars:
    name -> (value [n], bar [n])."""
    Rr, tr, S, sig, opt, mu = umeyama_ref(s, d)
    ms, md, sc, dc = _centre(s, d)
    n = s.shape[0]
    eye = np.eye(3)
    orth = np.abs(np.einsum("nij,nkj->nik", R, R) - eye).reshape(n, 9).max(1)
    det = np.abs(np.linalg.det(R) - 1.0)
    cen = np.abs(np.einsum("nij,nj->ni", R, ms) + t - md).max(1)
    cen_bar = 64 * EPS * (np.abs(ms).max(1) + np.abs(md).max(1) + 1.0)
    u = EPS * np.maximum(np.abs(s).reshape(n, -1).max(1), np.abs(d).reshape(n, -1).max(1))
    Q = ((np.linalg.norm(sc, axis=2) + u[:, None]) * (np.linalg.norm(dc, axis=2) + u[:, None])).sum(1)
    obj = np.einsum("nki,nij,nkj->n", dc, R, sc)
    res = np.sqrt((((np.einsum("nij,nkj->nki", R, s) + t[:, None, :]) - d) ** 2).sum(2).mean(1))
    with np.errstate(divide="ignore"):
        rot_bar = np.where(mu > 0, 1024 * EPS / np.where(mu > 0, mu, 1.0), np.inf)
    return dict(orth=(orth, np.full(n, 64 * EPS)), det=(det, np.full(n, 64 * EPS)), centroid=(cen, cen_bar),
                gap=(opt - obj, 256 * EPS * Q), rot=(np.abs(R - Rr).reshape(n, 9).max(1), rot_bar),
                residual=(res, np.sqrt(2 * 256 * EPS * Q / 4) + cen_bar), mu=(mu, None), sigma1=(sig[:, 0], None))


def check_fits(name, s, d, R, t, unique, report=print):
    """Criteria 1-4 of the module docstring on every draw of a family; returns the list of
    failures (empty = pass), each with the worst value, its draw index and mu there."""
    fails = []
    finite = np.isfinite(R).reshape(len(R), -1).all(1) & np.isfinite(t).all(1)
    if not finite.all():
        return [f"{name}: non-finite fit at draw {int(np.argmin(finite))} ({int((~finite).sum())} draws)"]
    f = fit_figures(s, d, R, t)
    mu = f["mu"][0]
    keys = ["orth", "det", "centroid", "gap"] + (["rot"] if unique else []) + ([] if name in INEXACT else ["residual"])
    line = [f"{name:22s}"]
    for k in keys:
        v, bar = f[k]
        ratio = v / bar
        i = int(np.argmax(ratio))
        line.append(f"{k} {v[i]:.2e}/{bar[i]:.2e}")
        if not (v <= bar).all():
            fails.append(f"{name}: {k} {v[i]:.3e} > {bar[i]:.3e} at draw {i} (mu {mu[i]:.3e}); "
                         f"{int((v > bar).sum())} of {len(v)} draws over")
    if unique:
        i = int(np.argmax(f["rot"][0] * mu))
        line.append(f"|dR| mu/eps {f['rot'][0][i] * mu[i] / EPS:.1f}")
    i = int(np.argmax(f["gap"][0] / np.maximum(f["sigma1"][0], 1e-300)))
    line.append(f"gap/(eps s1) {f['gap'][0][i] / max(f['sigma1'][0][i], 1e-300) / EPS:.1f}")
    report(" | ".join(line))
    return fails


SEED = 2034
_DRAWS = None


def draws():
    """The PER_FAMILY draws of every family that the CPU and GPU tests share (computed once)."""
    global _DRAWS
    if _DRAWS is None:
        _DRAWS = families(np.random.default_rng(SEED), PER_FAMILY)
    return _DRAWS


def family_sensitivity(name, s, d):
    return sensitivity(s, d, centred=name == "far_centroid")


PLANAR_TRIALS = ((31, 199), (32, 200), (33, 201))   # (data seed, hypothesis seed) per trial
PLANAR_H = 512
PLANAR_MAX_DIST = 0.05


def planar_ransac_case(data_seed):
    """test_corr_pose_gpu.py::test_ransac_matches_c_oracle's layout on a flat CAD: 200 points of a
    plane under a random rotation, a crop of 150 of them + N(0, 0.01^2) under a random pose, 128
    correspondences of which 35 % are inliers. Every 4-point draw is coplanar.
    -> cad [200,3], pc [150,3], corres int32 [128,2], R, t."""
    rng = np.random.default_rng(data_seed)
    flat = rng.normal(size=(200, 3)) * 5
    flat[:, 2] = 0.0
    cad = np.ascontiguousarray(flat @ quat_rotations(rng, 1)[0].T)
    R, t = _pose(rng, 1)
    R, t = R[0], t[0]
    pc_obj = cad[rng.integers(0, 200, 150)] + rng.normal(size=(150, 3)) * 0.01
    pc = np.ascontiguousarray(pc_obj @ R.T + t)
    n = 128
    src_idx = rng.integers(0, 200, n)
    dst_idx = rng.integers(0, 150, n)
    good = rng.random(n) < 0.35
    src_idx[good] = np.argmin(((cad[None, :, :] - pc_obj[dst_idx[good], None, :]) ** 2).sum(-1), axis=1)
    corres = np.ascontiguousarray(np.stack([src_idx, dst_idx], 1).astype(np.int32))
    return cad, pc, corres, R, t


# the same repeats expressed through the hypothesis row on generic crops: name -> (row, unique)
ROWS = {"row_0012": ((0, 0, 1, 2), True), "row_0011": ((0, 0, 1, 1), False), "row_0000": ((0, 0, 0, 0), False)}


def row_draws():
    """name -> (s, d, unique) as the fit sees them: the generic crops' points taken by ROWS."""
    s, d, _ = draws()["generic"]
    return {name: (np.ascontiguousarray(s[:, row]), np.ascontiguousarray(d[:, row]), unique)
            for name, (row, unique) in ROWS.items()}


def all_draws():
    return {**draws(), **row_draws()}
