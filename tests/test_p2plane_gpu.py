"""(f4, opt-in) Normal estimation and point-to-plane ICP on the GPU (csrc/icp.hip:
pk_estimate_normals, pk_icp_plane_*) against the fp64 numpy restatement tests/_p2plane_ref.py
(parity unpinned against Open3D, which is absent; the restatement's own CPU test is
test_p2plane_cpu.py).

Bars, all measured on the restatement itself under a second summation order (order="rev") and
recorded in DESIGN.md §4:
  * neighbour indices: bit-exact;
  * normals: angle to the restatement's normal (sign included) over the points whose eigen-gap
    (l1 - l0) / l2 is >= 1e-3. The restatement against itself: 1.13e-15 rad on the ellipsoid
    target, 1.22e-14 rad on the blob; the bar is 100x the larger one, 1.22e-12 rad. Left out
    below the gap: none of the 1500 ellipsoid points (smallest gap 0.16), none of the 1500 blob
    points (smallest gap 0.018);
  * normals where the covariance's smallest eigenvalue is exactly 0 or repeated (derived bars, see
    test_normals_on_degenerate_neighbourhoods): exact on an integer-millimetre plane, 64 eps
    lmax / lmid on its tilt, the Rayleigh quotient on a line, one point and an octahedron;
  * point-to-plane ICP with the restatement's normals passed in: update count, converged flag
    and fitness equal, rmse and T within 1e-9 (the restatement against itself, every sum
    reversed: at most 1.1e-13 in T and 1.8e-15 in rmse over the cases below, same update counts);
  * the same with the normals estimated on the device end to end (ellipsoid case): the
    restatement with reversed covariance sums and every ICP sum reversed differs from itself by
    1.42e-14 in T (one ulp of the translation's z, about 90) and 1.7e-15 in rmse; bar 100x,
    1.42e-12.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _p2plane_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
KNN_SIZES = (0, 1, 2, 3, 29, 30, 31, 257, 1500, 1700)  # both sides of the 1024-point LDS window
NORMAL_BAR = 1.22e-12  # rad
GAP_MIN = 1e-3
ESTIMATED_BAR = 1.42e-12  # |dT|, |drmse| with device-estimated normals


def _pack(arrs, device):
    off = np.concatenate([[0], np.cumsum([a.shape[0] for a in arrs])]).astype(np.int64)
    cat = np.concatenate(arrs, 0) if sum(a.shape[0] for a in arrs) else np.zeros((1, 3))
    return (torch.from_numpy(np.ascontiguousarray(cat, dtype=np.float64)).to(device),
            torch.from_numpy(off).to(device))


def knn_crops():
    """Ragged crops with continuous random coordinates (no exact tie), one crop of 40 points
    repeated twice (every distance ties once: the index tie-break), and one 1700-point crop of
    almost constant x, whose every walk crosses the whole crop (past the LDS window)."""
    rng = np.random.default_rng(11)
    crops = [rng.normal(size=(n, 3)) * np.array([5.0, 3.0, 2.5]) + np.array([0, 0, 90.0]) for n in KNN_SIZES]
    dup = rng.normal(size=(40, 3)) * 2 + np.array([1.0, 2.0, 90.0])
    crops.append(np.concatenate([dup, dup]))
    flat = rng.normal(size=(1700, 3)) * np.array([1e-9, 3.0, 2.5]) + np.array([4.0, 0, 90.0])
    crops.append(flat)
    return [np.ascontiguousarray(c) for c in crops]


def blob():
    rng = np.random.default_rng(5)
    return np.ascontiguousarray(rng.normal(size=(1500, 3)) * np.array([5.0, 3.0, 0.4]) + np.array([1.0, -2.0, 90.0]))


def ragged_cases(seed=0):
    """Six crops, 200-2000 source points: a noisy ellipsoid surface as the target, a noisy
    subset of it as the source in its own frame, perturbed starts (the layout of
    test_icp_gpu.py::test_icp_ragged_batch_matches_oracle on a surface)."""
    from dpfm_amd.dataset.synthetic import random_rotation
    rng = np.random.default_rng(seed)
    out = []
    for b, ns in enumerate([200, 731, 1024, 1999, 2000, 357]):
        nt = int(ns * rng.uniform(1.0, 1.2)) + 100
        u = rng.normal(size=(nt, 3))
        tgt = u / np.linalg.norm(u, axis=1, keepdims=True) * np.array([5.0, 3.0, 2.5]) + np.array([0, 0, 90.0])
        tgt = tgt + rng.normal(size=(nt, 3)) * 0.02
        src = tgt[rng.permutation(nt)[:ns]] + rng.normal(size=(ns, 3)) * 0.03
        Rm = random_rotation(rng)
        tt = rng.normal(size=3) * 10
        Tg = np.eye(4)
        Tg[:3, :3] = Rm
        Tg[:3, 3] = tt
        out.append(dict(src=np.ascontiguousarray((src - tt) @ Rm), tgt=np.ascontiguousarray(tgt),
                        T0=R.perturb(rng, Tg, 3.0 + b, 0.2, src.mean(0)), r=0.5))
    return out


def real_cases():
    g = np.load(os.path.join(GOLD, "real_crops.npz"))
    rng = np.random.default_rng(3)
    out = []
    for i in (0, 4):
        cad = g[f"cad_{int(g[f'{i}_obj_id'])}"]
        tgt = g[f"{i}_pc"]
        out.append(dict(src=np.ascontiguousarray(cad), tgt=np.ascontiguousarray(tgt),
                        T0=R.perturb(rng, g[f"{i}_T_gt"], 2.0, 0.1, tgt.mean(0)), r=0.2))
    return out


MAX_IT = 60


@pytest.fixture(scope="module")
def icp_cases():
    """Every ICP case with the restatement's normals and results, computed once."""
    cases = ragged_cases() + [R.ellipsoid_case()] + real_cases()
    for c in cases:
        c["nrm"], _ = R.normals_ref(c["tgt"], 30)
        c["T"], c["st"] = R.icp_ref(c["src"], c["tgt"], c["T0"], c["r"], MAX_IT, "point_to_plane", c["nrm"])
    return cases


def _run(cases, device, max_it=MAX_IT, normals=True, **kw):
    from dpfm_amd import ops
    s, so = _pack([c["src"] for c in cases], device)
    t, to = _pack([c["tgt"] for c in cases], device)
    n = _pack([c["nrm"] for c in cases], device)[0] if normals else None
    T0 = torch.from_numpy(np.stack([c["T0"] for c in cases])).to(device)
    T, st = ops.icp(s, so, t, to, T0, cases[0]["r"], max_it, estimation="point_to_plane", tgt_normals=n, **kw)
    return T.cpu().numpy(), st.cpu().numpy()


def _compare(T, st, cases, tol):
    for b, c in enumerate(cases):
        print(f"crop {b}: gpu {st[b].tolist()} ref {c['st'].tolist()} |dT| {np.abs(T[b] - c['T']).max():.3e} "
              f"|drmse| {abs(st[b, 1] - c['st'][1]):.3e}")
    for b, c in enumerate(cases):
        assert st[b, 2] == c["st"][2] and st[b, 3] == c["st"][3], (b, st[b], c["st"])
        assert st[b, 0] == c["st"][0], (b, st[b], c["st"])
        assert abs(st[b, 1] - c["st"][1]) <= tol, (b, st[b], c["st"])
        np.testing.assert_allclose(T[b], c["T"], rtol=0, atol=tol, err_msg=f"crop {b}")


@pytest.fixture(scope="module")
def knn_ref():
    crops = knn_crops()
    return crops, [R.knn_brute(c, 32) for c in crops]


@pytest.mark.parametrize("k", [30, 3, 32])
def test_neighbour_indices_bit_exact(device, knn_ref, k):
    from dpfm_amd import ops
    crops, ref = knn_ref
    p, off = _pack(crops, device)
    nrm, knn = ops.estimate_normals(p, off, k=k, return_knn=True)
    knn = knn.cpu().numpy()
    o = off.cpu().numpy()
    assert knn.dtype == np.int32 and knn.shape == (int(o[-1]), k)
    for b, c in enumerate(crops):
        # the (d^2, index) order makes the k-list a prefix of the 32-list
        np.testing.assert_array_equal(knn[o[b]:o[b + 1]], ref[b][:, :k], err_msg=f"crop {b} (n = {c.shape[0]})")
    assert torch.isfinite(nrm).all()


def _angles(n, ref):
    """angle (rad) between unit vectors, sign included: atan2(|n x ref|, n . ref)."""
    return np.arctan2(np.linalg.norm(np.cross(n, ref), axis=1), np.einsum("nc,nc->n", n, ref))


def test_normals_match_restatement(device):
    from dpfm_amd import ops
    from dpfm_amd.pose.icp import estimate_normals
    clouds = [R.ellipsoid_case()["tgt"], blob()]
    tiny = [clouds[0][:2], clouds[0][:1]]
    p, off = _pack(clouds + tiny, device)
    nrm = ops.estimate_normals(p, off, k=30).cpu().numpy()
    o = off.cpu().numpy()
    for b, c in enumerate(clouds):
        ref, gap = R.normals_ref(c, 30)
        keep = gap >= GAP_MIN
        got = nrm[o[b]:o[b + 1]]
        ang = _angles(got[keep], ref[keep])
        print(f"cloud {b}: left out {int((~keep).sum())} of {c.shape[0]}, smallest gap {gap.min():.3g}, "
              f"max angle {ang.max():.3e} rad, max | |n| - 1 | {np.abs(np.linalg.norm(got, axis=1) - 1).max():.3e}")
        assert (~keep).sum() <= 0.01 * c.shape[0]
        assert ang.max() <= NORMAL_BAR
        assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 1e-15  # unit up to the division's rounding
        assert (np.einsum("nc,nc->n", got, -c) >= 0).all()  # towards the camera at the origin
    # fewer than 3 points: exactly (0, 0, 1)
    np.testing.assert_array_equal(nrm[o[2]:], np.tile([0.0, 0.0, 1.0], (3, 1)))
    # another viewpoint only changes signs; the one-cloud numpy entry point is the same kernel
    vp = np.array([3.0, -40.0, 100.0])
    far = ops.estimate_normals(p, off, k=30, viewpoint=vp).cpu().numpy()[:o[2]]
    pts = np.concatenate(clouds)
    sgn = np.where(np.einsum("nc,nc->n", nrm[:o[2]], vp - pts) < 0, -1.0, 1.0)
    assert (sgn < 0).any() and (sgn > 0).any()
    np.testing.assert_array_equal(far, nrm[:o[2]] * sgn[:, None])
    np.testing.assert_array_equal(estimate_normals(clouds[1], device=device), nrm[o[1]:o[2]])


EPS = float(np.finfo(np.float64).eps)


def degenerate_crops():
    """Neighbourhoods whose covariance has an exactly zero or a repeated smallest eigenvalue:
    (a) a fronto-parallel plane in integer-millimetre depth, z = 900 (what every real frame holds);
    (b) the same plane tilted by a random rotation;
    (c) points on a line; (d) 64 copies of one point;
    (e) an octahedron: 6 copies of a centre and 4 of each vertex centre +- e_i, the 30 nearest
        neighbours of a centre copy (C = (8/30) I exactly at k = 30), and 34 points far outside.
    -> crops, the tilted plane's unit normal."""
    from dpfm_amd.dataset.synthetic import random_rotation
    rng = np.random.default_rng(31)   # a seed whose plane has no collinear 3-neighbourhood
    plane = np.concatenate([np.round(rng.uniform(-300, 300, size=(400, 2))), np.full((400, 1), 900.0)], 1)
    Rm = random_rotation(rng)
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    line = np.array([10.0, -20.0, 900.0]) + rng.uniform(-300, 300, size=(100, 1)) * u
    same = np.tile(np.array([[12.5, -7.25, 903.0]]), (64, 1))
    c = np.array([3.0, 4.0, 900.0])
    far = rng.normal(size=(34, 3))
    octa = np.concatenate([np.tile(c, (6, 1))] + [np.tile(c + sg * e, (4, 1)) for e in np.eye(3) for sg in (1.0, -1.0)] +
                          [c + 50.0 * far / np.linalg.norm(far, axis=1, keepdims=True)])
    crops = [plane, plane @ Rm.T, line, same, octa[rng.permutation(64)]]
    return [np.ascontiguousarray(x) for x in crops], Rm[:, 2].copy()


@pytest.mark.parametrize("k", [30, 3])
def test_normals_on_degenerate_neighbourhoods(device, k):
    """min_eigvec3 where the smallest eigenvalue is exactly 0 or not simple (one call for all crops).
    Planes: the normal itself — exactly (0, 0, -1) on the integer plane (every ez is exactly 0, so
    the covariance's z row is exactly 0 and no Jacobi rotation touches it), within 64 eps lmax /
    lmid of the true normal on the tilted one. Line, one point, octahedron: the normal is not
    unique; it is a unit vector towards the viewpoint whose Rayleigh quotient is the smallest
    eigenvalue."""
    from dpfm_amd import ops
    crops, tilt = degenerate_crops()
    p, off = _pack(crops, device)
    nrm, knn = ops.estimate_normals(p, off, k=k, return_knn=True)
    nrm, knn, o = nrm.cpu(), knn.cpu().numpy(), off.cpu().numpy()
    # (a)
    flat = nrm[o[0]:o[1]]
    gap = R.normals_ref(crops[0], k)[1]
    assert gap.min() > 1e-6   # no neighbourhood of the seed's plane is collinear: the in-plane eigenvalues are > 0
    assert torch.equal(flat, torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64).expand(400, 3))
    nrm = nrm.numpy()
    # (b)
    gap = R.normals_ref(crops[1], k)[1]
    true = np.tile(tilt if tilt @ -crops[1][0] > 0 else -tilt, (400, 1))
    ang = _angles(nrm[o[1]:o[2]], true)
    bar = 64 * EPS / gap + 1e-15
    i = int(np.argmax(ang / bar))
    print(f"k = {k}: tilted plane: angle {ang[i]:.3e} / {bar[i]:.3e} at point {i} (lmid / lmax {gap[i]:.3e})")
    assert gap.min() > 1e-6 and (ang <= bar).all()
    # (c) - (e)
    for b, what in ((2, "line"), (3, "one point"), (4, "octahedron")):
        P, n = crops[b], nrm[o[b]:o[b + 1]]
        C = R.cov_ref(P, k)
        w = np.linalg.eigvalsh(C)
        assert np.isfinite(n).all(), what
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 8 * EPS, what
        ray = np.einsum("ni,nij,nj->n", n, C, n)
        i = int(np.argmax(ray - w[:, 0] - 64 * EPS * w[:, 2]))
        print(f"k = {k}: {what}: Rayleigh {ray[i]:.3e}, lmin {w[i, 0]:.3e}, lmax {w[i, 2]:.3e} at point {i}")
        assert (ray <= w[:, 0] + 64 * EPS * w[:, 2]).all(), what
        assert (np.einsum("nc,nc->n", n, -P) >= -8 * EPS * np.linalg.norm(P, axis=1)).all(), what
    # equal distances: the (d^2, index) order
    np.testing.assert_array_equal(knn[o[3]:o[4]], R.knn_brute(crops[3], k))
    if k == 30:   # the octahedron's centre copies see the isotropic neighbourhood
        centre = np.nonzero((crops[4] == np.array([3.0, 4.0, 900.0])).all(1))[0]
        C = R.cov_ref(crops[4], 30)[centre]
        assert centre.size == 6 and (C == np.eye(3) * C[0, 0, 0]).all() and C[0, 0, 0] > 0


def test_plane_icp_matches_restatement(device, icp_cases):
    ragged, ell, real = icp_cases[:6], icp_cases[6:7], icp_cases[7:]
    for group in (ragged, ell, real):
        T, st = _run(group, device)
        _compare(T, st, group, 1e-9)
    assert all(c["st"][3] == 1 for c in ragged + ell)  # these stop on the relative criteria
    assert ell[0]["st"][2] <= 10


def test_plane_icp_estimated_normals_end_to_end(device, icp_cases):
    from dpfm_amd.pose.icp import registration_icp
    ell = icp_cases[6:7]
    T, st = _run(ell, device, normals=False)
    _compare(T, st, ell, ESTIMATED_BAR)
    c = ell[0]
    r = registration_icp(c["src"], c["tgt"], c["r"], c["T0"], max_iteration=MAX_IT, device=device,
                         estimation="point_to_plane")
    np.testing.assert_array_equal(r.transformation, T[0])
    assert r.iterations == st[0, 2] and r.converged


def _plane_case():
    """An exact plane z = 90 with the source on it, shifted in the plane: the in-plane motion is
    unobservable, the third pivot of the normal equations is exactly 0 and U = I."""
    rng = np.random.default_rng(8)
    tgt = np.concatenate([rng.uniform(-3, 3, size=(400, 2)), np.full((400, 1), 90.0)], 1)
    nrm = np.tile([0.0, 0.0, -1.0], (400, 1))
    T0 = np.eye(4)
    T0[:2, 3] = [0.015625, -0.03125]
    return dict(src=np.ascontiguousarray(tgt[:250]), tgt=np.ascontiguousarray(tgt), nrm=nrm, T0=T0, r=0.5)


def test_plane_icp_edge_cases(device, icp_cases):
    from dpfm_amd import ops
    base = icp_cases[0]
    away = np.eye(4)
    away[:3, 3] = 1000.0
    far = dict(base, T0=away)
    empty = dict(base, tgt=np.zeros((0, 3)), nrm=np.zeros((0, 3)))
    flat = _plane_case()
    cases = [far, empty, flat, base]
    for c in cases[:3]:
        c["T"], c["st"] = R.icp_ref(c["src"], c["tgt"], c["T0"], 0.5, 50, "point_to_plane", c["nrm"])
    cases[3] = dict(base)
    cases[3]["T"], cases[3]["st"] = R.icp_ref(base["src"], base["tgt"], base["T0"], 0.5, 50, "point_to_plane", base["nrm"])
    T, st = _run(cases, device, max_it=50)
    _compare(T, st, cases, 1e-9)
    # no pair / empty target: one identity update, then the unchanged evaluation stops the loop
    for b in (0, 1):
        assert st[b].tolist() == [0.0, 0.0, 1.0, 1.0]
        np.testing.assert_array_equal(T[b], cases[b]["T0"])
    # singular system: the non-positive pivot gives U = I at the first update; the second
    # evaluation repeats the first and stops the loop: 1 update, converged, T = T_init
    assert st[2, 2] == 1 and st[2, 3] == 1 and st[2, 0] == 1.0
    np.testing.assert_array_equal(T[2], flat["T0"])
    # max_iteration 0: the initial evaluation only
    c0 = dict(base)
    c0["T"], c0["st"] = R.icp_ref(base["src"], base["tgt"], base["T0"], 0.5, 0, "point_to_plane", base["nrm"])
    T, st = _run([c0], device, max_it=0)
    _compare(T, st, [c0], 1e-9)
    assert st[0, 2] == 0 and st[0, 3] == 0
    np.testing.assert_array_equal(T[0], base["T0"])
    # poll granularity does not change the result
    Ta, sa = _run([base], device, max_it=50, poll=1)
    Tb, sb = _run([base], device, max_it=50, poll=64)
    assert np.array_equal(Ta, Tb) and np.array_equal(sa, sb)
    s, so = _pack([base["src"]], device)
    t, to = _pack([base["tgt"]], device)
    n = torch.from_numpy(base["nrm"]).to(device)
    T0 = torch.from_numpy(base["T0"][None]).to(device)
    a = ops.icp(s, so, t, to, T0, 0.5, 50, poll=1, estimation="point_to_plane", tgt_normals=n)
    b = ops.icp(s, so, t, to, T0, 0.5, 50, poll=64, estimation="point_to_plane", tgt_normals=n)
    f = ops.icp_fixed(s, so, t, to, T0, 0.5, 51, base["src"].shape[0], base["tgt"].shape[0],
                      estimation="point_to_plane", tgt_normals=n)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], f[0]) and torch.equal(a[1], f[1])


def test_capacity_overflow_is_flagged(device, icp_cases):
    """A crop above nsrc_max / ntgt_max is not refined (converged = -1, T = T_init) and the
    other crops are refined as alone; estimate_normals flags a crop above nmax with NaN normals
    and -1 neighbours and leaves the rows of the other crops as they are without it."""
    from dpfm_amd import ops
    cases = [icp_cases[0], icp_cases[1], icp_cases[5]]  # 200, 731, 357 source points
    s, so = _pack([c["src"] for c in cases], device)
    t, to = _pack([c["tgt"] for c in cases], device)
    n = _pack([c["nrm"] for c in cases], device)[0]
    T0 = torch.from_numpy(np.stack([c["T0"] for c in cases])).to(device)
    cap_t = cases[2]["tgt"].shape[0]   # crop 1's target (and source) exceed the capacities
    assert cases[0]["tgt"].shape[0] <= cap_t < cases[1]["tgt"].shape[0]
    T, st = ops.icp(s, so, t, to, T0, 0.5, MAX_IT, nsrc_max=400, ntgt_max=cap_t, estimation="point_to_plane",
                    tgt_normals=n)
    T, st = T.cpu().numpy(), st.cpu().numpy()
    assert st[1, 3] == -1 and st[1, 2] == 0
    np.testing.assert_array_equal(T[1], cases[1]["T0"])
    _compare(T[[0, 2]], st[[0, 2]], [cases[0], cases[2]], 1e-9)
    full, knn_full = ops.estimate_normals(t, to, k=30, return_knn=True)
    nrm, knn = ops.estimate_normals(t, to, k=30, nmax=cap_t, return_knn=True)
    o = to.cpu().numpy()
    assert torch.isnan(nrm[o[1]:o[2]]).all() and (knn[o[1]:o[2]] == -1).all()
    for a, b in ((o[0], o[1]), (o[2], o[3])):
        assert torch.equal(nrm[a:b], full[a:b]) and torch.equal(knn[a:b], knn_full[a:b])


def test_deterministic_and_independent_of_scratch(device, icp_cases):
    """The C entry points on a work buffer pre-filled with 0xFF bytes (twice) and with zeros:
    equal results, and the guard bytes past the sized work buffer stay as they were."""
    from dpfm_amd import _lib
    cases = [icp_cases[1], icp_cases[6]]
    s, so = _pack([c["src"] for c in cases], device)
    t, to = _pack([c["tgt"] for c in cases], device)
    T0 = torch.from_numpy(np.stack([c["T0"] for c in cases])).to(device).contiguous()
    B = 2
    nsm = max(c["src"].shape[0] for c in cases)
    ntm = max(c["tgt"].shape[0] for c in cases)
    lib = _lib.lib()
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    st = _lib.stream(device)
    guard = 4096
    outs = []
    for fill in (0xFF, 0xFF, 0x00):
        nb = int(lib.pk_normals_work_size(B, ntm))
        wn = torch.full((nb + guard,), fill, dtype=torch.uint8, device=device)
        nrm = torch.empty((t.shape[0], 3), dtype=torch.float64, device=device)
        knn = torch.empty((t.shape[0], 30), dtype=torch.int32, device=device)
        assert lib.pk_estimate_normals(p(t), p(to), B, ntm, 30, 0.0, 0.0, 0.0, p(nrm), p(knn), p(wn), nb, st) == 0
        nbytes = int(lib.pk_icp_plane_work_size(B, nsm, ntm))
        work = torch.full((nbytes + guard,), fill, dtype=torch.uint8, device=device)
        assert lib.pk_icp_plane_init(p(s), p(so), p(t), p(to), p(nrm), p(T0), B, nsm, ntm, p(work), nbytes, st) == 0
        assert lib.pk_icp_plane_iterate(p(s), p(so), p(t), p(to), 0.5, 20, 1e-6, 1e-6, B, nsm, ntm, 21, p(work), nbytes,
                                        None, st) == 0
        T = torch.empty((B, 4, 4), dtype=torch.float64, device=device)
        stats = torch.empty((B, 4), dtype=torch.float64, device=device)
        assert lib.pk_icp_result(p(work), B, p(T), p(stats), st) == 0
        torch.cuda.synchronize()
        assert (wn[nb:] == fill).all() and (work[nbytes:] == fill).all()
        outs.append((nrm, knn, T, stats))
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert torch.equal(x, y)
    assert (outs[0][3][:, 2] > 0).all()


def test_infer_step_point_to_plane_graphed_matches_eager(device):
    from dpfm_amd import ops
    from dpfm_amd.dataset.object import CropFormation
    from dpfm_amd.models.dpfm import DPFMNet
    from dpfm_amd.pipeline import GraphedInfer, InferStep, make_frame_batch
    torch.manual_seed(0)
    F, N, E = 4, 512, 8
    fb, op = make_frame_batch(F, N, N, seed=72, device=device)
    model = DPFMNet().to(device).eval()
    crops = CropFormation(n1=N, npoint=N, seed=2)(fb)
    out = InferStep(model, hypotheses=256, icp_evaluations=E, icp_estimation="point_to_plane")(fb, op, crops)
    out = {k: out[k].clone() for k in ("T", "T_icp", "icp", "metrics_icp")}
    assert torch.isfinite(out["metrics_icp"]).all()
    # the step's ICP is the host-polled point-to-plane ICP with normals estimated from the crops
    T, st = ops.icp(fb.cad64, fb.cad_off, crops.pc64, crops.off, out["T"], 0.2, E - 1, nsrc_max=N, ntgt_max=N,
                    estimation="point_to_plane")
    assert torch.equal(out["T_icp"], T) and torch.equal(out["icp"], st)
    g = GraphedInfer(CropFormation(n1=N, npoint=N, seed=2),
                     InferStep(model, hypotheses=256, icp_evaluations=E, icp_estimation="point_to_plane"), fb, op)
    o2 = g()
    torch.cuda.synchronize()
    for key in ("T_icp", "icp", "metrics_icp"):
        assert torch.equal(o2[key], out[key]), key
    # the default estimator is the constructor call without the keyword
    a = InferStep(model, hypotheses=256, icp_evaluations=E, icp_estimation="point_to_point")(fb, op, crops)
    b = InferStep(model, hypotheses=256, icp_evaluations=E)(fb, op, crops)
    for key in ("T_icp", "icp", "metrics_icp"):
        assert torch.equal(a[key], b[key]), key
