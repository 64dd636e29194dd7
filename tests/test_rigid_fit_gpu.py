"""The device's 4-point rigid fit (csrc/rigid.hpp: rigid_fit4 -> top_eigvec4_qcp, Jacobi fallback)
against the fp64 SVD reference tests/_rigid_ref.py, draw by draw, on the inputs where a closed-form
eigen solve goes wrong: coplanar draws, repeated correspondences, near-collinear draws, mirrored
draws, 180 degree rotations, far centroids, scales 1e-3 .. 1e3 (the families and the bars are in
_rigid_ref.py's docstring; test_rigid_ref_cpu.py pins the reference).

One pk_ransac launch fits them all: every draw is a crop of 4 points with the 4 crop-local
correspondences (k, k), one explicit hypothesis row and a distance threshold nothing depends on, so
ransac_final_kernel returns hypothesis 0's [R | t] of every crop. The rows (0,0,1,2), (0,0,1,1) and
(0,0,0,0) on the generic crops express the repeats through the draw instead of the points.
"""
import numpy as np
import pytest
import torch

import _rigid_ref as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_fits(device):
    """name -> (R [n,3,3], t [n,3]) of every family and row parametrisation, one launch."""
    from dpfm_amd import ops
    fam = RR.draws()
    crops = [(name, s, d, (0, 1, 2, 3)) for name, (s, d, _) in fam.items()]
    crops += [(name, fam["generic"][0], fam["generic"][1], row) for name, (row, _) in RR.ROWS.items()]
    src = np.concatenate([s.reshape(-1, 3) for _, s, _, _ in crops])
    dst = np.concatenate([d.reshape(-1, 3) for _, _, d, _ in crops])
    B = src.shape[0] // 4
    hyps = np.concatenate([np.tile(np.array(row, np.int32), (s.shape[0], 1)) for _, s, _, row in crops])
    off = torch.arange(B + 1, dtype=torch.int64, device=device) * 4
    corres = torch.arange(4, dtype=torch.int32, device=device).repeat(B)[:, None].repeat(1, 2).contiguous()
    T, st = ops.ransac(torch.from_numpy(src).to(device), off, torch.from_numpy(dst).to(device), off, corres, off, 1,
                       max_dist=1e30, hyps=torch.from_numpy(hyps).to(device),
                       hyp_off=torch.arange(B + 1, dtype=torch.int64, device=device), nmax=4)
    T, st = T.cpu().numpy(), st.cpu().numpy()
    assert (st[:, 2] == 0).all() and (st[np.isfinite(T).reshape(B, -1).all(1), 0] == 1.0).all()
    out, a = {}, 0
    for name, s, _, _ in crops:
        out[name] = (T[a:a + s.shape[0], :3, :3].copy(), T[a:a + s.shape[0], :3, 3].copy())
        a += s.shape[0]
    return out


@pytest.mark.parametrize("name", list(RR.all_draws()))
def test_device_fit_matches_reference(device_fits, name):
    s, d, unique = RR.all_draws()[name]
    R, t = device_fits[name]
    if unique:
        # the rotation bar is never tighter than the problem: 4x the reference's own sensitivity
        mu = RR.umeyama_ref(s, d)[5]
        assert mu.min() >= RR.MU_MIN
        assert (1024 * RR.EPS / mu >= 4 * RR.family_sensitivity(name, s, d)).all()
    fails = RR.check_fits(name, s, d, R, t, unique)
    assert not fails, "\n".join(fails)
