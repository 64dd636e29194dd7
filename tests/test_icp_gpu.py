"""(f4) ICP after RANSAC on the GPU (csrc/icp.hip) against the C oracle oc_icp, which the CPU
suite pins against the numpy restatement of Open3D's loop (test_oracle_cpu.py::test_icp_*).

  * ragged synthetic batch (200-2000 source points, 300-2400 target points), perturbed
    initial poses, 2000-iteration budget: same update count and convergence flag per crop,
    fitness equal, rmse and T within 1e-9 (the GPU sums pairs in a block tree, the oracle
    sequentially; no pair decision flips on these inputs);
  * the reference's own setting on its real data (tests/golden/real_crops.npz): source = CAD
    (~5000 vertices), target = the CAD under T_gt (test_RANSAC.py:426-436), threshold 0.2,
    init = T_gt perturbed; and the build's crop-target variant (CAD against the observed crop);
  * exact planes (an integer-millimetre fronto-parallel plane, and the same plane tilted): every
    update's cross-covariance has rank 2; source and target on one line (rank 1): the rotation is
    not unique, so fitness and rmse are compared and T only has to be rigid;
  * edge cases: no pair within the radius, an empty target, max_iteration 0, and the blocking
    C entry point pk_icp against the host-polled loop.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from _util import cp

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _perturb(rng, T, deg, shift, center):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    dR = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    D = np.eye(4)
    D[:3, :3] = dR
    D[:3, 3] = center - dR @ center + rng.normal(size=3) * shift
    return D @ T


def _oracle(coracle, src, tgt, T0, r, max_it):
    T = np.zeros(16)
    st = np.zeros(4)
    coracle.oc_icp(cp(np.ascontiguousarray(src)), src.shape[0], cp(np.ascontiguousarray(tgt)), tgt.shape[0],
                   cp(np.ascontiguousarray(T0)), r, max_it, 1e-6, 1e-6, cp(T), cp(st))
    return T.reshape(4, 4), st


def _pack(arrs, device):
    off = np.concatenate([[0], np.cumsum([a.shape[0] for a in arrs])]).astype(np.int64)
    cat = np.concatenate(arrs, 0) if sum(a.shape[0] for a in arrs) else np.zeros((1, 3))
    return (torch.from_numpy(np.ascontiguousarray(cat, dtype=np.float64)).to(device),
            torch.from_numpy(off).to(device))


def _check(coracle, srcs, tgts, T0s, r, max_it, device, **kw):
    from dpfm_amd import ops
    s, so = _pack(srcs, device)
    t, to = _pack(tgts, device)
    T0 = torch.from_numpy(np.stack(T0s)).to(device)
    T, st = ops.icp(s, so, t, to, T0, r, max_it, **kw)
    T = T.cpu().numpy()
    st = st.cpu().numpy()
    for b in range(len(srcs)):
        To, sto = _oracle(coracle, srcs[b], tgts[b], T0s[b], r, max_it)
        assert st[b, 2] == sto[2] and st[b, 3] == sto[3], (b, st[b], sto)
        assert st[b, 0] == sto[0], (b, st[b], sto)
        assert abs(st[b, 1] - sto[1]) <= 1e-9, (b, st[b], sto)
        np.testing.assert_allclose(T[b], To, atol=1e-9, err_msg=f"crop {b}")
    return T, st


def test_icp_ragged_batch_matches_oracle(coracle, device):
    rng = np.random.default_rng(0)
    srcs, tgts, T0s = [], [], []
    for b, ns in enumerate([200, 731, 1024, 1999, 2000, 357]):
        nt = int(ns * rng.uniform(1.0, 1.2)) + 100
        tgt = rng.normal(size=(nt, 3)) * np.array([5.0, 3.0, 2.5]) + np.array([0, 0, 90.0])
        src = tgt[rng.permutation(nt)[:ns]] + rng.normal(size=(ns, 3)) * 0.03
        # source in its own frame: undo a random pose, then start ICP near it
        from dpfm_amd.dataset.synthetic import random_rotation
        R = random_rotation(rng)
        tt = rng.normal(size=3) * 10
        src_obj = (src - tt) @ R  # src = R src_obj + tt
        Tg = np.eye(4)
        Tg[:3, :3] = R
        Tg[:3, 3] = tt
        T0s.append(_perturb(rng, Tg, 3.0 + b, 0.2, src.mean(0)))
        srcs.append(np.ascontiguousarray(src_obj))
        tgts.append(np.ascontiguousarray(tgt))
    T, st = _check(coracle, srcs, tgts, T0s, 0.5, 2000, device)
    assert (st[:, 3] == 1).all() and (st[:, 0] > 0.8).all()


@pytest.mark.parametrize("target", ["gt_cad", "crop"])
def test_icp_real_crops_matches_oracle(coracle, device, target):
    g = np.load(os.path.join(GOLD, "real_crops.npz"))
    rng = np.random.default_rng(3)
    srcs, tgts, T0s = [], [], []
    for i in (0, 4):
        cad = g[f"cad_{int(g[f'{i}_obj_id'])}"]
        Tg = g[f"{i}_T_gt"]
        if target == "gt_cad":  # test_RANSAC.py:426-436 (the reference's ICP target)
            tgt = cad @ Tg[:3, :3].T + Tg[:3, 3]
        else:
            tgt = g[f"{i}_pc"]
        srcs.append(np.ascontiguousarray(cad))
        tgts.append(np.ascontiguousarray(tgt))
        T0s.append(_perturb(rng, Tg, 2.0, 0.1, tgt.mean(0)))
    _check(coracle, srcs, tgts, T0s, 0.2, 2000, device)


def integer_plane(rng, n=400):
    """A fronto-parallel surface in integer-millimetre depth: x, y = round(U(-300, 300)), z = 900."""
    return np.ascontiguousarray(np.concatenate([np.round(rng.uniform(-300, 300, size=(n, 2))), np.full((n, 1), 900.0)], 1))


def test_icp_exact_planes_match_oracle(coracle, device):
    """Every update's cross-covariance has rank 2 exactly (rigid_from_cov on coplanar pairs): the
    integer plane, and the same plane tilted; source = 250 of the target's points, started 2
    degrees / 3 mm off, radius 20."""
    from dpfm_amd.dataset.synthetic import random_rotation
    rng = np.random.default_rng(12)
    flat = integer_plane(rng)
    tilted = np.ascontiguousarray(flat @ random_rotation(rng).T)
    srcs, tgts, T0s = [], [], []
    for tgt in (flat, tilted):
        src = np.ascontiguousarray(tgt[rng.permutation(400)[:250]])
        srcs.append(src)
        tgts.append(tgt)
        T0s.append(_perturb(rng, np.eye(4), 2.0, 3.0, src.mean(0)))
    T, st = _check(coracle, srcs, tgts, T0s, 20.0, 100, device)
    assert (st[:, 3] == 1).all() and (st[:, 0] == 1.0).all()


def test_icp_collinear_points_match_oracle_stats(coracle, device):
    """Source and target on one line: every update's cross-covariance has rank 1, the rotation
    about the line is free (T is not compared), and neither the fitness nor the inlier rmse depends
    on it. T stays a rigid transform (R R^T = I and det R = 1 to 64 eps; the oracle stops after 9
    updates with 3 eps)."""
    from dpfm_amd import ops
    rng = np.random.default_rng(13)
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    tgt = np.ascontiguousarray(np.array([10.0, -20.0, 900.0]) + rng.uniform(-300, 300, size=(400, 1)) * u)
    src = np.ascontiguousarray(tgt[rng.permutation(400)[:250]])
    T0 = _perturb(rng, np.eye(4), 2.0, 3.0, src.mean(0))
    s, so = _pack([src], device)
    t, to = _pack([tgt], device)
    T, st = ops.icp(s, so, t, to, torch.from_numpy(T0[None]).to(device), 20.0, 30)
    T, st = T.cpu().numpy()[0], st.cpu().numpy()[0]
    To, sto = _oracle(coracle, src, tgt, T0, 20.0, 30)
    print(f"device {st.tolist()} oracle {sto.tolist()}")
    assert abs(st[0] - sto[0]) <= 1e-9 and abs(st[1] - sto[1]) <= 1e-9 and st[0] > 0.9
    eps = np.finfo(np.float64).eps
    Rm = T[:3, :3]
    assert np.isfinite(T).all() and (T[3] == [0, 0, 0, 1]).all()
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 64 * eps and abs(np.linalg.det(Rm) - 1) <= 64 * eps


def test_icp_edge_cases(coracle, device):
    from dpfm_amd import ops
    rng = np.random.default_rng(9)
    tgt = rng.normal(size=(500, 3)) * 3
    src = np.ascontiguousarray(tgt[:300] + 0.01)
    far = np.eye(4)
    far[:3, 3] = 100.0
    near = np.eye(4)
    # no pairs / empty target / normal crop in one batch
    _check(coracle, [src, src, src], [tgt, np.zeros((0, 3)), tgt], [far, near, near], 0.2, 50, device)
    # max_iteration 0: the initial evaluation only
    _check(coracle, [src], [tgt], [near], 0.2, 0, device)
    # poll granularity does not change the result
    s, so = _pack([src], device)
    t, to = _pack([tgt], device)
    T0 = torch.from_numpy(near[None]).to(device)
    Ta, sa = ops.icp(s, so, t, to, T0, 0.2, 100, poll=1)
    Tb, sb = ops.icp(s, so, t, to, T0, 0.2, 100, poll=64)
    assert torch.equal(Ta, Tb) and torch.equal(sa, sb)


def test_pk_icp_blocking_entry_matches_polled(device):
    from dpfm_amd import _lib, ops
    rng = np.random.default_rng(4)
    tgts = [rng.normal(size=(n, 3)) * 4 for n in (800, 1200)]
    srcs = [np.ascontiguousarray(t[: n // 2] + rng.normal(size=(n // 2, 3)) * 0.02) for t, n in zip(tgts, (800, 1200))]
    s, so = _pack(srcs, device)
    t, to = _pack(tgts, device)
    T0 = torch.eye(4, dtype=torch.float64, device=device).repeat(2, 1, 1)
    T0[:, :3, 3] = 0.1
    Ta, sa = ops.icp(s, so, t, to, T0, 0.3, 200)
    B, nsm, ntm = 2, 600, 1200
    nbytes = int(_lib.lib().pk_icp_work_size(B, nsm, ntm))
    work = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    cnt = torch.zeros((1,), dtype=torch.int32, device=device)
    Tb = torch.empty((B, 4, 4), dtype=torch.float64, device=device)
    sb = torch.empty((B, 4), dtype=torch.float64, device=device)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = _lib.lib().pk_icp(p(s), p(so), p(t), p(to), p(T0.contiguous()), 0.3, 200, 1e-6, 1e-6, B, nsm, ntm, 8, p(work),
                           nbytes, p(cnt), p(Tb), p(sb), _lib.stream(device))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(Ta, Tb) and torch.equal(sa, sb)


def test_icp_and_metrics_capacity_overflow(device, coracle):
    """A crop whose source or target exceeds the capacities the caller sized the scratch for
    (nsrc_max / ntgt_max) is not refined and flagged (converged = -1, T = T_init) instead of
    writing past its rows; the other crops are refined as the oracle does. pk_pose_metrics
    reports NaN for a crop above its capacity."""
    from dpfm_amd import ops
    rng = np.random.default_rng(77)
    srcs = [rng.normal(size=(n, 3)) * 3 for n in (300, 700, 300)]
    tgts = [s + rng.normal(size=s.shape) * 0.01 for s in srcs]
    tgts[2] = np.concatenate([tgts[2], rng.normal(size=(500, 3)) * 3])   # 800 target points
    T0s = [_perturb(rng, np.eye(4), 2.0, 0.02, s.mean(0)) for s in srcs]
    s, so = _pack(srcs, device)
    t, to = _pack(tgts, device)
    T0 = torch.from_numpy(np.stack(T0s)).to(device)
    T, st = ops.icp(s, so, t, to, T0, 0.2, 50, nsrc_max=400, ntgt_max=400)
    T, st = T.cpu().numpy(), st.cpu().numpy()
    assert st[1, 3] == -1 and st[2, 3] == -1 and st[1, 2] == 0 and st[2, 2] == 0
    np.testing.assert_array_equal(T[1], T0s[1])
    np.testing.assert_array_equal(T[2], T0s[2])
    To, sto = _oracle(coracle, srcs[0], tgts[0], T0s[0], 0.2, 50)
    assert st[0, 2] == sto[2] and st[0, 3] == sto[3] and st[0, 0] == sto[0]
    np.testing.assert_allclose(T[0], To, atol=1e-9)
    m = ops.pose_metrics(s, so, 400, T0, T0).cpu().numpy()
    assert np.isnan(m[1]).all() and not np.isnan(m[0]).any() and not np.isnan(m[2]).any()
    assert (m[0] == 0).all()


def _pin():
    g = dict(np.load(os.path.join(GOLD, "icp_pin.npz")))
    rc = np.load(os.path.join(GOLD, "real_crops.npz"))
    cads = {int(o): rc[f"cad_{int(o)}"] for o in np.unique(g["obj_id"])}
    return g, cads


def test_icp_pinned_by_reference_outputs(device):
    """f4 (and the PointToPoint / Umeyama estimator H13 shares) pinned by the reference's own
    Open3D results: for 512 published crops of results_on_{pbr,real}/results_poses_{RANSAC,
    TEASER} (tests/golden/icp_pin.npz), ICP exactly as test_RANSAC.py:424-446 runs it — source =
    the decimated CAD, target = transform(CAD, T_gt) (test_RANSAC.py:154-160), threshold 0.2,
    init = T_pred (the solver's pose as the txt printed it, 9 digits), max_iteration 2000,
    Open3D's default relative criteria 1e-6 — all crops in one batched launch sequence, vs the
    reference's T_pred_ICP (fitted from cad_i_pose_est.ply). Bar: max |dT| <= 1e-6 per crop (the
    printed init perturbs the start by ~1e-9 relative; the C oracle lands within 1.3e-8 of the
    reference on these crops)."""
    from dpfm_amd.pose.icp import gt_posed_target, icp_batched, registration_icp
    g, cads = _pin()
    n = g["obj_id"].shape[0]
    srcs = [cads[int(o)] for o in g["obj_id"]]
    tgts = [np.ascontiguousarray(c @ T[:3, :3].T + T[:3, 3]) for c, T in zip(srcs, g["T_gt"])]
    s, so = _pack(srcs, device)
    t, to = _pack(tgts, device)
    T0 = torch.from_numpy(np.ascontiguousarray(g["T_pred"])).to(device)
    T, st = icp_batched(s, so, t, to, T0, 0.2, 2000)
    T, st = T.cpu().numpy(), st.cpu().numpy()
    err = np.abs(T - g["T_icp"]).reshape(n, -1).max(1)
    bad = np.nonzero(err > 1e-6)[0]
    assert bad.size == 0, [(int(k), float(err[k]), st[k].tolist()) for k in bad[:10]]
    assert (st[:, 3] == 1).all()  # every published crop stopped on the relative criteria
    # the device-side target (pipeline path) and the one-crop Open3D-shaped entry point
    t_dev = gt_posed_target(s, so, torch.from_numpy(np.ascontiguousarray(g["T_gt"])).to(device))
    T2, _ = icp_batched(s, so, t_dev, to, T0, 0.2, 2000)
    assert np.abs(T2.cpu().numpy() - g["T_icp"]).max() <= 1e-6
    for k in (0, n - 1):
        r = registration_icp(srcs[k], tgts[k], 0.2, g["T_pred"][k], max_iteration=2000, device=device)
        np.testing.assert_allclose(r.transformation, g["T_icp"][k], atol=1e-6)
        np.testing.assert_array_equal(r.transformation, T[k])
