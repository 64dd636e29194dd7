"""ICP refinement after RANSAC — the (f4) row: scripts/test_RANSAC.py:436-446 runs Open3D
0.17 `registration_icp(source = CAD, target = CAD posed by T_gt, threshold = 0.2, trans_init =
T_RANSAC, TransformationEstimationPointToPoint(), ICPConvergenceCriteria(max_iteration=2000))`.

`registration_icp` keeps that signature (numpy or tensors in, a RegistrationResult out);
`refine_to_crop` is the variant the reference does not offer: ICP of the CAD against the
OBSERVED crop (camera frame), which needs no ground truth. The reference's target (the
GT-posed CAD) makes its "after ICP" numbers an upper bound; see DESIGN.md §7.

Semantics (csrc/icp.hip, parity unpinned against Open3D): nearest target point by exact fp64
distance (ties: lowest index), pair iff d^2 < threshold^2, Umeyama without scaling, stop on
|dfitness| < 1e-6 and |drmse| < 1e-6 or after max_iteration updates.

Opt-in (`estimation="point_to_plane"`): Open3D's TransformationEstimationPointToPlane in the same
loop — the update minimises sum ((T s - q) . n_q)^2 over the pairs — with the target's normals
passed by the caller (`tgt_normals`) or estimated as `estimate_normals` does (Open3D's
estimate_normals(KDTreeSearchParamKNN(normals_k)) oriented towards the origin). This is the
estimator for `refine_to_crop`: on a partial, noisy depth crop point-to-point pairs hold the CAD
back along the surface, point-to-plane pairs let it slide."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import ops


@dataclass
class ICPResult:
    """The fields of open3d.pipelines.registration.RegistrationResult the reference reads,
    plus the iteration count and whether the relative criteria stopped the loop."""
    transformation: np.ndarray
    fitness: float
    inlier_rmse: float
    iterations: int
    converged: bool


def _dev(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _f64(x, dev):
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.asarray(x, dtype=np.float64), device=dev).contiguous()


def estimate_normals(points, k: int = 30, viewpoint=None, device=None) -> np.ndarray:
    """Open3D `estimate_normals(KDTreeSearchParamKNN(knn=k))` + `orient_normals_towards_camera_location(
    viewpoint)` (the origin if None) of one cloud [N,3] -> unit normals f64 [N,3] (numpy)."""
    dev = _dev(device)
    pts = _f64(points, dev).reshape(-1, 3)
    off = torch.tensor([0, pts.shape[0]], dtype=torch.int64, device=dev)
    return ops.estimate_normals(pts, off, k=k, viewpoint=viewpoint, nmax=pts.shape[0]).cpu().numpy()


def _check_estimation(estimation, target_shape, tgt_normals):
    """Argument errors before any device work (ops.icp checks the same on tensors)."""
    if estimation not in ops.ICP_ESTIMATIONS:
        raise ValueError(f"estimation must be one of {ops.ICP_ESTIMATIONS}, got {estimation!r}")
    if tgt_normals is not None:
        if estimation != "point_to_plane":
            raise ValueError("tgt_normals are read by estimation='point_to_plane' only")
        if tuple(np.shape(tgt_normals)) != tuple(target_shape):
            raise ValueError(f"tgt_normals must have the target's shape {tuple(target_shape)}, got "
                             f"{tuple(np.shape(tgt_normals))}")


def registration_icp(source, target, max_correspondence_distance, init=None, max_iteration: int = 30,
                     relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, device=None,
                     estimation: str = "point_to_point", tgt_normals=None, normals_k: int = 30) -> ICPResult:
    """source [Ns,3], target [Nt,3], init 4x4 (identity if None) -> ICPResult (one crop).
    estimation="point_to_plane" reads tgt_normals [Nt,3] (estimated from the target if None)."""
    _check_estimation(estimation, np.shape(target), tgt_normals)
    dev = _dev(device)
    src = _f64(source, dev).reshape(-1, 3)
    tgt = _f64(target, dev).reshape(-1, 3)
    T0 = _f64(np.eye(4) if init is None else init, dev).reshape(1, 4, 4)
    so = torch.tensor([0, src.shape[0]], dtype=torch.int64, device=dev)
    to = torch.tensor([0, tgt.shape[0]], dtype=torch.int64, device=dev)
    T, st = ops.icp(src, so, tgt, to, T0, max_correspondence_distance, max_iteration, relative_fitness,
                    relative_rmse, nsrc_max=src.shape[0], ntgt_max=tgt.shape[0], estimation=estimation,
                    tgt_normals=None if tgt_normals is None else _f64(tgt_normals, dev).reshape(-1, 3),
                    normals_k=normals_k)
    st = st[0].cpu().numpy()
    return ICPResult(T[0].cpu().numpy(), float(st[0]), float(st[1]), int(st[2]), bool(st[3]))


def icp_batched(src, src_off, tgt, tgt_off, T_init, max_dist: float = 0.2, max_iter: int = 2000,
                rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, nsrc_max=None, ntgt_max=None, poll: int = 8,
                estimation: str = "point_to_point", tgt_normals=None, normals_k: int = 30):
    """All crops at once (device tensors, packed layout): (T f64 [B,4,4], stats f64 [B,4])."""
    return ops.icp(src, src_off, tgt, tgt_off, T_init, max_dist, max_iter, rel_fitness, rel_rmse,
                   nsrc_max=nsrc_max, ntgt_max=ntgt_max, poll=poll, estimation=estimation, tgt_normals=tgt_normals,
                   normals_k=normals_k)


def gt_posed_target(cad, off, T_gt):
    """The reference's ICP target (test_RANSAC.py:426-427, 436): every crop's CAD under T_gt,
    packed like `cad` (f64 [T,3]); `transform` of test_RANSAC.py:154-160 (pcd @ R^T + t)."""
    B = off.numel() - 1
    counts = (off[1:] - off[:-1])
    crop = torch.repeat_interleave(torch.arange(B, device=cad.device), counts)
    R = T_gt[:, :3, :3].to(torch.float64)[crop]
    t = T_gt[:, :3, 3].to(torch.float64)[crop]
    return (torch.einsum("nc,nrc->nr", cad.to(torch.float64), R) + t).contiguous()


def refine_to_crop(cad, cad_off, crop, crop_off, T_ransac, max_dist: float = 0.2, max_iter: int = 2000,
                   estimation: str = "point_to_point", tgt_normals=None, normals_k: int = 30, **kw):
    """ICP of each crop's CAD (object frame) against its observed crop points (camera frame),
    starting from the RANSAC pose: (T f64 [B,4,4], stats f64 [B,4]). With
    estimation="point_to_plane" the crop's normals are estimated on the device (viewpoint: the
    camera, the origin of the crop's frame) unless tgt_normals gives them."""
    return ops.icp(cad, cad_off, crop, crop_off, T_ransac, max_dist, max_iter, estimation=estimation,
                   tgt_normals=tgt_normals, normals_k=normals_k, **kw)
