"""CPU: the numpy restatement of normal estimation and point-to-plane ICP (tests/_p2plane_ref.py)
on cases with a known answer, and the argument checks of the Python surface (no device needed).
The header / ctypes agreement of the new entry points is test_capi.py's."""
import numpy as np
import pytest

import _p2plane_ref as R


def test_normals_of_a_noiseless_plane():
    rng = np.random.default_rng(1)
    n0 = np.array([0.3, -0.2, -0.9])
    n0 /= np.linalg.norm(n0)
    e1 = np.cross(n0, [1.0, 0, 0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n0, e1)
    uv = rng.uniform(-4, 4, size=(300, 2))
    P = np.array([1.0, -2.0, 90.0]) + uv[:, :1] * e1 + uv[:, 1:] * e2
    for order in ("seq", "rev"):
        nrm, gap = R.normals_ref(P, 30, order=order)
        # oriented towards the origin: n0 . (0 - p) > 0 for this plane
        assert (np.einsum("nc,nc->n", nrm, -P) > 0).all()
        assert np.linalg.norm(np.cross(nrm, n0), axis=1).max() < 1e-7 and (nrm @ n0 > 0).all()
        assert gap.min() > 0.1
    # fewer than three neighbours: the fixed normal
    nrm, _ = R.normals_ref(P[:2], 30)
    np.testing.assert_array_equal(nrm, [[0, 0, 1.0], [0, 0, 1.0]])
    # neighbours: itself first, (d^2, index) order, -1 past the cloud's size
    knn = R.knn_brute(np.concatenate([P[:5], P[:5]]), 12)
    assert (knn[:, 0] == np.r_[0:5, 0:5]).all() and (knn[:, 1] == np.r_[5:10, 5:10]).all()
    assert (knn[:, 10:] == -1).all() and (knn[:, :10] >= 0).all()


def test_point_to_plane_beats_point_to_point_on_a_partial_view():
    """The ellipsoid partial-view case: point-to-plane stops on the relative criteria within 10
    updates and ends closer to the true pose, in angle and in translation, than point-to-point
    (measured: 7 updates, 0.29 degrees / 0.011 against 41 updates, 2.4 degrees / 0.12)."""
    c = R.ellipsoid_case()
    nrm, gap = R.normals_ref(c["tgt"], 30)
    assert gap.min() >= 1e-3
    Tp, sp = R.icp_ref(c["src"], c["tgt"], c["T0"], c["r"], 100, "point_to_plane", nrm)
    Tq, sq = R.icp_ref(c["src"], c["tgt"], c["T0"], c["r"], 100, "point_to_point")
    ep, eq = R.pose_error(Tp, c["T_true"]), R.pose_error(Tq, c["T_true"])
    assert sp[3] == 1 and sp[2] <= 10, sp
    assert sq[3] == 1 and sq[2] > sp[2], sq
    assert ep[0] < eq[0] and ep[1] < eq[1], (ep, eq)
    assert ep[0] < 0.5 and ep[1] < 0.02, ep
    # the summation order changes neither the update count nor (to 1e-12) the pose
    Tr, sr = R.icp_ref(c["src"], c["tgt"], c["T0"], c["r"], 100, "point_to_plane", nrm, order="rev")
    assert sr[2] == sp[2] and np.abs(Tr - Tp).max() < 1e-12


def test_singular_system_gives_identity_update():
    tgt = np.concatenate([np.random.default_rng(0).uniform(-3, 3, size=(100, 2)), np.full((100, 1), 90.0)], 1)
    nrm = np.tile([0.0, 0.0, -1.0], (100, 1))
    T0 = np.eye(4)
    T0[0, 3] = 0.015625
    T, st = R.icp_ref(tgt[:60], tgt, T0, 0.5, 30, "point_to_plane", nrm)
    np.testing.assert_array_equal(T, T0)
    assert st[2] == 1 and st[3] == 1


def test_argument_errors():
    from dpfm_amd import ops
    from dpfm_amd.pipeline import InferStep
    from dpfm_amd.pose.icp import registration_icp
    import torch
    src, tgt = np.zeros((10, 3)), np.zeros((12, 3))
    with pytest.raises(ValueError, match="estimation"):
        registration_icp(src, tgt, 0.2, estimation="bogus")
    with pytest.raises(ValueError, match="shape"):
        registration_icp(src, tgt, 0.2, estimation="point_to_plane", tgt_normals=np.zeros((10, 3)))
    with pytest.raises(ValueError, match="point_to_plane"):
        registration_icp(src, tgt, 0.2, tgt_normals=np.zeros((12, 3)))
    off = torch.tensor([0, 12])
    t = torch.zeros((12, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="estimation"):
        ops.icp(t, off, t, off, torch.eye(4)[None], 0.2, estimation="bogus", nsrc_max=12, ntgt_max=12)
    with pytest.raises(ValueError, match="tgt_normals"):
        ops.icp(t, off, t, off, torch.eye(4)[None], 0.2, estimation="point_to_plane", nsrc_max=12, ntgt_max=12,
                tgt_normals=torch.zeros((11, 3), dtype=torch.float64))
    for k in (2, 33):
        with pytest.raises(ValueError, match="k must be"):
            ops.estimate_normals(t, off, k=k)
    with pytest.raises(ValueError, match="icp_estimation"):
        InferStep(None, icp_estimation="bogus")
