"""ZoomOut-refined fmap -> point-map solvers (Melzi et al. 2019; pyFM's zoomout_refine) on the HIP
ZoomOut kernels (ops.zoomout): the 30 x 30 map grows to k_final x k_final in steps of `step`, each
step converting the map to a point map (naive.py's convention) and projecting that point map onto
the next, larger pair of bases. The reference repository has no ZoomOut; these solvers are opt-in
and `choose_fmap2pointmap_solver` does not select them."""
from __future__ import annotations

import torch

from .. import ops
from .spacial_filtering import spacial_filtering


def _run(C12, evecs_x, evecs_y, mass_y, k_final, step):
    if C12.dim() == 3:
        C12 = C12.squeeze(0)
    V1, V2 = evecs_x.shape[0], evecs_y.shape[0]
    dev = evecs_x.device
    n1 = torch.tensor([V1], dtype=torch.int32, device=dev)
    n2 = torch.tensor([V2], dtype=torch.int32, device=dev)
    C, p = ops.zoomout(evecs_x[None].float(), evecs_y[None].float(), mass_y.reshape(1, V2).float(), C12[None].float(),
                       n1, n2, k_final=k_final, step=step)
    return C[0], p[0]


def zoomout_refine(C12, evecs_x, evecs_y, mass_y, k_final=64, step=1):
    """The refined functional map, f32 [k_final, k_final]. C12 [30, 30] (or [1, 30, 30]), evecs_x
    [V1, K >= k_final], evecs_y [V2, K >= k_final], mass_y [V2]."""
    return _run(C12, evecs_x, evecs_y, mass_y, k_final, step)[0]


def zoomout_fmap2pointmap(C12, evecs_x, evecs_y, mass_y, k_final=64, step=1, **kwargs):
    """The refined map's point map, int64 [2, V2] = stack([p2p, arange(V2)]) like naive_fmap2pointmap."""
    pp = _run(C12, evecs_x, evecs_y, mass_y, k_final, step)[1]
    return torch.stack([pp, torch.arange(pp.shape[0], device=pp.device, dtype=torch.int64)], 0)


def zoomout_spacial_filtering_fmap2pointmap(C12, evecs_x, evecs_y, mass_y, CAD, PC, diam_cad, k_final=64, step=1):
    """The refined one-candidate-per-point map through the three rigidity rounds of
    spacial_filtering.py:42-75; returns the surviving columns, int64 [2, n]."""
    return spacial_filtering(CAD, PC, zoomout_fmap2pointmap(C12, evecs_x, evecs_y, mass_y, k_final, step), diam_cad)
