"""Restatement of the gradient operators and gradient features (upstream diffusion-net geometry.py
build_grad / build_grad_point_cloud / edge_tangent_vectors, layers.py SpatialGradientFeatures and
DiffusionNetBlock.forward with gradient features). The upstream package is absent, so this file
pins what the kernels implement: fp64 numpy for the operator (both neighbour rules, `rev=True`
reverses every sum), torch (any dtype / device) for the layer on dense [n, n] gradX / gradY."""
import numpy as np
import torch
import torch.nn as nn

from oracle import dpfm_model_oracle as M


# ------------------------------------------------------------------------------ neighbours
def cloud_neighbors(pts: np.ndarray, k: int) -> np.ndarray:
    """int32 [n, k]: the k nearest other points by ((dx dx + dy dy) + dz dz), ties to the lower
    index, -1 where the cloud has fewer."""
    n = pts.shape[0]
    d = pts[:, None, :] - pts[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d2[np.arange(n), np.arange(n)] = np.inf
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    out = np.full((n, k), -1, np.int32)
    m = min(k, n - 1)
    out[:, :m] = order[:, :m]
    return out


def mesh_neighbors(faces: np.ndarray, n: int) -> np.ndarray:
    """int32 [n, max degree]: every vertex's edge neighbours, unique and ascending, -1 padded."""
    adj = [set() for _ in range(n)]
    for a, b, c in np.asarray(faces).tolist():
        for u, v in ((a, b), (b, c), (c, a)):
            if u != v:
                adj[u].add(v)
                adj[v].add(u)
    W = max(1, max(len(s) for s in adj))
    out = np.full((n, W), -1, np.int32)
    for i, s in enumerate(adj):
        out[i, :len(s)] = sorted(s)
    return out


# ------------------------------------------------------------------------------ the operator
def _sum(terms, rev):
    acc = 0.0
    for t in (reversed(terms) if rev else terms):
        acc = acc + t
    return acc


def grad_rows(pts: np.ndarray, frames: np.ndarray, nbr: np.ndarray, rev: bool = False):
    """(idx int32 [n, W], val f64 [n, W, 2]) with W = nbr.shape[1] + 1: slot 0 the point itself,
    slot t + 1 the table's entry t (-1 / 0 where empty). Per point, a_t = (e_t . X, e_t . Y),
    M = sum a a^T + 1e-5 I, c_t = M^-1 a_t by the explicit 2 x 2 inverse, c_0 = -sum c_t."""
    n, K = nbr.shape
    idx = np.full((n, K + 1), -1, np.int32)
    val = np.zeros((n, K + 1, 2))
    for i in range(n):
        bx, by = frames[i, 0], frames[i, 1]
        slots = [(t, int(j)) for t, j in enumerate(nbr[i]) if 0 <= j < n and j != i]
        a = {}
        for t, j in slots:
            e = pts[j] - pts[i]
            a[t] = ((e[0] * bx[0] + e[1] * bx[1]) + e[2] * bx[2], (e[0] * by[0] + e[1] * by[1]) + e[2] * by[2])
        m00 = _sum([a[t][0] * a[t][0] for t, _ in slots], rev) + 1e-5
        m01 = _sum([a[t][0] * a[t][1] for t, _ in slots], rev)
        m11 = _sum([a[t][1] * a[t][1] for t, _ in slots], rev) + 1e-5
        det = m00 * m11 - m01 * m01
        for t, j in slots:
            idx[i, t + 1] = j
            val[i, t + 1, 0] = (m11 * a[t][0] - m01 * a[t][1]) / det
            val[i, t + 1, 1] = (m00 * a[t][1] - m01 * a[t][0]) / det
        idx[i, 0] = i
        val[i, 0, 0] = -_sum([val[i, t + 1, 0] for t, _ in slots], rev)
        val[i, 0, 1] = -_sum([val[i, t + 1, 1] for t, _ in slots], rev)
    return idx, val


def dense(idx: np.ndarray, val: np.ndarray, n: int):
    """Dense [n, n] (gradX, gradY) of fixed-width rows."""
    gx, gy = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        for s in range(idx.shape[1]):
            j = idx[i, s]
            if j >= 0:
                gx[i, j] += val[i, s, 0]
                gy[i, j] += val[i, s, 1]
    return gx, gy


def tangent_frames(normals: np.ndarray) -> np.ndarray:
    """build_tangent_frames: [n, 3, 3] rows (basisX, basisY, normal)."""
    n = normals / np.linalg.norm(normals, axis=1, keepdims=True)
    cand = np.where((np.abs(n[:, 0]) < 0.9)[:, None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    bx = cand - (cand * n).sum(-1, keepdims=True) * n
    bx /= np.linalg.norm(bx, axis=1, keepdims=True)
    return np.stack((bx, np.cross(n, bx), n), axis=1)


# ------------------------------------------------------------------------------ the layer
class SpatialGradientFeatures(nn.Module):
    def __init__(self, C, rotations=True):
        super().__init__()
        self.rotations = rotations
        if rotations:
            self.A_re = nn.Linear(C, C, bias=False)
            self.A_im = nn.Linear(C, C, bias=False)
        else:
            self.A = nn.Linear(C, C, bias=False)

    def forward(self, vX, vY):
        if self.rotations:
            b_re = self.A_re(vX) - self.A_im(vY)
            b_im = self.A_re(vY) + self.A_im(vX)
        else:
            b_re, b_im = self.A(vX), self.A(vY)
        return torch.tanh(vX * b_re + vY * b_im)


class Block(nn.Module):
    def __init__(self, C, rotations=True):
        super().__init__()
        self.diffusion = M.LearnedTimeDiffusion(C)
        self.gradient_features = SpatialGradientFeatures(C, rotations)
        self.mlp = M.MiniMLP([3 * C, C, C, C])

    def forward(self, x, mass, evals, evecs, gradX, gradY):
        xd = self.diffusion(x, mass, evals, evecs)
        g = self.gradient_features(torch.matmul(gradX, xd), torch.matmul(gradY, xd))
        return self.mlp(torch.cat((x, xd, g), dim=-1)) + x


class DiffusionNet(nn.Module):
    """DiffusionNet with gradient features on dense batched gradX / gradY [B, N, N]."""

    def __init__(self, C_in=3, C_out=32, C_width=64, N_block=2, rotations=True):
        super().__init__()
        self.first_lin = nn.Linear(C_in, C_width)
        self.last_lin = nn.Linear(C_width, C_out)
        self.blocks = []
        for i in range(N_block):
            self.blocks.append(Block(C_width, rotations))
            self.add_module(f"block_{i}", self.blocks[-1])

    def forward(self, x, mass, evals, evecs, gradX, gradY):
        h = self.first_lin(x)
        for blk in self.blocks:
            h = blk(h, mass, evals, evecs, gradX, gradY)
        return self.last_lin(h)


# ------------------------------------------------------------------------------ shared inputs
def sphere_cap(n: int, seed: int) -> np.ndarray:
    """n random points on a cap of the unit sphere (polar angle <= ~0.6 rad), f64 [n, 3]."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(np.cos(0.6), 1.0, n)
    ph = rng.uniform(0.0, 2 * np.pi, n)
    r = np.sqrt(1.0 - z * z)
    return np.stack((r * np.cos(ph), r * np.sin(ph), z), axis=1)


def hub_ring(seed: int = 0) -> np.ndarray:
    """A ring of 60 points of radius 1 (1e-3 jitter) and its centre (the last point): with
    30 neighbours the centre is a neighbour of every ring point (in-degree 60), a ring point of at
    most 31 others."""
    rng = np.random.default_rng(seed)
    t = 2 * np.pi * np.arange(60) / 60
    ring = np.stack((np.cos(t), np.sin(t), np.zeros(60)), axis=1) + 1e-3 * rng.normal(size=(60, 3))
    return np.concatenate((ring, np.zeros((1, 3))))


def fixed_width(blocks, nmax: int):
    """Stack per-crop (idx [n, W], val [n, W, 2]) into the batch layout padded to nmax rows."""
    W = max(i.shape[1] for i, _ in blocks)
    idx = np.full((len(blocks), nmax, W), -1, np.int32)
    val = np.zeros((len(blocks), nmax, W, 2))
    for b, (i, v) in enumerate(blocks):
        idx[b, :i.shape[0], :i.shape[1]] = i
        val[b, :i.shape[0], :i.shape[1]] = v
    return idx, val
