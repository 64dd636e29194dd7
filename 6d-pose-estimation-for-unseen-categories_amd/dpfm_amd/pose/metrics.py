"""Pose metrics of scripts/test_RANSAC.py:77-81, 154-238 with the reference's
signatures. The per-point work (ADD, the per-row "xyz direction" distances and the
1-D nearest-neighbour ADD-S) runs in pk_pose_metrics for any number of crops."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops


def _metrics(pts3d, pose_gt, pose_pred, device=None):
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    cad = torch.as_tensor(np.asarray(pts3d, dtype=np.float64), device=dev).contiguous()
    off = torch.tensor([0, cad.shape[0]], dtype=torch.int64, device=dev)
    Te = torch.as_tensor(np.asarray(pose_pred, dtype=np.float64).reshape(1, 4, 4), device=dev)
    Tg = torch.as_tensor(np.asarray(pose_gt, dtype=np.float64).reshape(1, 4, 4), device=dev)
    return ops.pose_metrics(cad, off, cad.shape[0], Te, Tg)[0].cpu().numpy()


def add(T_est, T_gt, pcd, diameter, percentage=0.1):
    """Mean distance between the model under the two poses, and whether it is below
    percentage * diameter (test_RANSAC.py:162-173)."""
    e = float(_metrics(pcd, T_gt, T_est)[0])
    return e, int(e < diameter * percentage)


def compute_add_score(pts3d, diameter, pose_gt, pose_pred, percentage=0.1):
    m = _metrics(pts3d, pose_gt, pose_pred)[1:4].astype(np.float32)
    return (m < diameter * percentage).sum() / 3


def compute_adds_score(pts3d, diameter, pose_gt, pose_pred, percentage=0.1):
    t = np.asarray(pose_pred)[:3, 3]
    m = _metrics(pts3d, pose_gt, pose_pred)[4:7].astype(np.float32)
    m[np.isnan(t)] = np.inf
    return (m < diameter * percentage).sum() / 3


def get_angular_error(R_exp, R_est):
    return abs(np.arccos(min(max(((np.matmul(R_exp.T, R_est)).trace() - 1) / 2, -1.0), 1.0)))


def pose_metrics_batched(cad, off, nmax, T_est, T_gt):
    """Device tensors: f64 [B, 7] = (ADD, xyz-direction means x3, ADD-S means x3)."""
    return ops.pose_metrics(cad, off, nmax, T_est, T_gt)


# ------------------------------------------------------------------ BOP pose errors (absent in the reference)
# bop_toolkit pose_error.py mssd / mspd / adi with its names and signatures; the work runs in
# pk_bop_errors. `syms` is bop_toolkit's list of {"R": 3x3, "t": 3x1} (misc.get_symmetry_transformations;
# dataset/formats.py symmetry_transformations builds the same set as one [S, 4, 4] array).

def _pose44(R, t):
    T = np.eye(4)
    T[:3, :3] = np.asarray(R, dtype=np.float64).reshape(3, 3)
    T[:3, 3] = np.asarray(t, dtype=np.float64).reshape(3)
    return T


def _bop_single(R_est, t_est, R_gt, t_gt, pts, syms=None, K=None, device=None):
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    cad = torch.as_tensor(np.asarray(pts, dtype=np.float64).reshape(-1, 3), device=dev).contiguous()
    n = cad.shape[0]
    off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    Te = torch.as_tensor(_pose44(R_est, t_est)[None], device=dev)
    Tg = torch.as_tensor(_pose44(R_gt, t_gt)[None], device=dev)
    sym = sym_off = None
    if syms is not None:
        S = np.stack([_pose44(s["R"], s["t"]) for s in syms]) if len(syms) else np.zeros((0, 4, 4))
        sym = torch.as_tensor(S, device=dev)
        sym_off = torch.tensor([0, len(syms)], dtype=torch.int64, device=dev)
    Kd = None if K is None else torch.as_tensor(np.asarray(K, dtype=np.float64).reshape(1, 3, 3), device=dev)
    out, _ = ops.bop_errors(cad, off, n, Te, Tg, Kd, sym, sym_off)
    return out[0].cpu().numpy()


def mssd(R_est, t_est, R_gt, t_gt, pts, syms):
    """Maximum Symmetry-Aware Surface Distance: min over syms of the largest vertex distance."""
    return float(_bop_single(R_est, t_est, R_gt, t_gt, pts, syms)[0])


def mspd(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """Maximum Symmetry-Aware Projection Distance (pixels)."""
    return float(_bop_single(R_est, t_est, R_gt, t_gt, pts, syms, K)[1])


def adi(R_est, t_est, R_gt, t_gt, pts):
    """Average distance to the nearest vertex of the GT-posed model (the ADD-S of the papers)."""
    return float(_bop_single(R_est, t_est, R_gt, t_gt, pts)[2])


def bop_errors_batched(cad, off, nmax, T_est, T_gt, K=None, sym=None, sym_off=None, smax=None):
    """Device tensors: (f64 [B, 3] = (MSSD, MSPD, ADI), int32 [B, 2] = best symmetry of MSSD / MSPD)."""
    return ops.bop_errors(cad, off, nmax, T_est, T_gt, K, sym, sym_off, smax)


def bop_recall(errors, thresholds):
    """Mean over the thresholds of the fraction of errors strictly below each (a NaN error, a pose
    that was not evaluated, counts as a miss). errors [N]; thresholds [M] or, per estimate, [M, N]."""
    e = torch.as_tensor(errors, dtype=torch.float64).reshape(1, -1)
    th = torch.as_tensor(thresholds, dtype=torch.float64, device=e.device)
    th = th.reshape(-1, 1) if th.dim() < 2 else th
    return float((e < th).to(torch.float64).mean(1).mean())


def bop_average_recall(mssd, mspd, diameter, image_width):
    """BOP's average recall over its two renderer-free errors: the mean of AR_MSSD (thresholds
    0.05 ... 0.5 of the object diameter in steps of 0.05; `diameter` a number or one per estimate)
    and AR_MSPD (5r ... 50r pixels in steps of 5r, r = image_width / 640)."""
    e3 = torch.as_tensor(mssd, dtype=torch.float64).reshape(-1)
    steps = torch.arange(1, 11, dtype=torch.float64, device=e3.device)
    d = torch.as_tensor(diameter, dtype=torch.float64, device=e3.device).reshape(-1).expand(e3.numel())
    ar3 = bop_recall(e3, 0.05 * steps[:, None] * d[None, :])
    ar2 = bop_recall(mspd, 5.0 * steps.cpu() * (float(image_width) / 640.0))
    return 0.5 * (ar3 + ar2)
