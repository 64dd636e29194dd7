"""TEASER++ pose solver — the (f2) row: scripts/test_teaser.py:327-331, 362-435 builds
`teaserpp_python.RobustRegistrationSolver(params)` with cbar2 = 1, noise_bound = 0.05,
estimate_scaling = False, GNC_TLS rotation (gnc factor 1.4, 100 iterations, cost threshold
1e-12) and calls `solver.solve(src[3,n], dst[3,n])`, `solver.getSolution()` (.rotation,
.translation, .valid).

`RobustRegistrationSolver` keeps that interface; `teaser_batched` solves many crops at once.
The pairwise-consistency graph (O(n^2)) is built on the device (csrc/teaser.hip); the clique
search, GNC-TLS and adaptive voting run as native host code (parity unpinned: the TEASER++
package is absent, restated from its published algorithm).

With estimate_scaling = True (TEASER's default, for a CAD stand-in of another size than the observed
object) the scale is voted first over the distance ratios of all pairs, on the device
(csrc/teaser_scale.hip), and the graph, the rotation and the translation are solved at that scale:
`TeaserSolution.scale`, and `TeaserSolution.transform` = [[scale R, t], [0, 1]] to apply to the CAD.
Build-defined deviation: a pair of coincident source points takes no part in the vote and is never
consistent (upstream would produce inf / NaN)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from .. import ops


@dataclass
class TeaserSolution:
    """The fields of teaser::RegistrationSolution the reference reads, plus the clique."""
    valid: bool
    scale: float
    rotation: np.ndarray
    translation: np.ndarray
    max_clique: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    clique_mode: str = "exact"  # exact | budget | kcore
    rotation_inliers: int = 0
    translation_inliers: int = 0

    @property
    def transform(self) -> np.ndarray:
        """4x4 [[scale R, t], [0, 1]]: maps the source (CAD) points onto the destination."""
        T = np.eye(4)
        T[:3, :3] = self.scale * self.rotation
        T[:3, 3] = self.translation
        return T


class RobustRegistrationSolver:
    """teaserpp_python.RobustRegistrationSolver with the reference's parameter fields."""

    class Params:
        def __init__(self):
            self.cbar2 = 1.0
            self.noise_bound = 0.01
            self.estimate_scaling = True
            self.rotation_gnc_factor = 1.4
            self.rotation_max_iterations = 100
            self.rotation_cost_threshold = 1e-6
            self.kcore_heuristic_threshold = 0.5
            self.max_clique_nodes = 2_000_000

    def __init__(self, params: "RobustRegistrationSolver.Params", device=None):
        self.params = params
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._sol = None

    def solve(self, src, dst):
        """src, dst: [3, n] (TEASER's column convention)."""
        a = torch.as_tensor(np.asarray(src, dtype=np.float64).T.copy(), device=self.device)
        b = torch.as_tensor(np.asarray(dst, dtype=np.float64).T.copy(), device=self.device)
        off = torch.tensor([0, a.shape[0]], dtype=torch.int64, device=self.device)
        p = self.params
        out = ops.teaser(a, b, off, a.shape[0], p.noise_bound, p.cbar2, p.rotation_gnc_factor,
                         p.rotation_max_iterations, p.rotation_cost_threshold, p.kcore_heuristic_threshold,
                         p.max_clique_nodes, threads=1, estimate_scaling=bool(p.estimate_scaling))
        self._sol = _solution(*(x[0] for x in out))
        return self._sol

    def getSolution(self) -> TeaserSolution:  # noqa: N802 (reference API name)
        return self._sol


def _solution(T, clique, size, info, scale=1.0) -> TeaserSolution:
    mode = {1: "exact", 0: "budget", 2: "kcore"}[int(info[1])]
    return TeaserSolution(bool(info[0]), float(scale), T[:3, :3].copy(), T[:3, 3].copy(), clique[:int(size)].copy(),
                          mode, int(info[2]), int(info[3]))


def teaser_batched(src, dst, off, nmax=None, threads: int = 8, estimate_scaling: bool = False, **params):
    """Device tensors (matched pairs packed by off) -> list of TeaserSolution, one per crop."""
    out = ops.teaser(src, dst, off, nmax, threads=threads, estimate_scaling=estimate_scaling, **params)
    return [_solution(*(x[b] for x in out)) for b in range(out[0].shape[0])]
