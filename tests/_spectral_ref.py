"""Plain torch restatement of the spectral path's kernels, taken from the header comments of
include/posekern.h (pk_spectral_diffusion, pk_fmap_head_fwd / _bwd, pk_fmap_solve[_backward]) and
the formulas at the top of csrc/spectral.hip / csrc/fmap.hip. Nothing here calls dpfm_amd.ops.

Every function takes the kernels' f32 inputs and a working precision `dtype`: float64 is the
truth the device results are compared with, float32 (on the CPU) is the yardstick of the
"3x the fp32 reference's own error" rule. Backward passes are written out explicitly, not through
autograd (tests/test_spectral_ref_cpu.py pins them against autograd, the oracle and get_mask).

Errors are measured against componentwise bounds: the same expression with every operand
replaced by its absolute value (the quantity a rounding-error analysis of a sum of products is
stated in), so one dropped or misplaced term of a long sum is not diluted by a tensor maximum.
"""
import torch

U24 = 2.0 ** -24            # unit roundoff of f32
T_MIN = 9.99999993922529e-09  # float32(1e-8): the clamp of LearnedTimeDiffusion, as the kernel's 1e-8f
K_FMAP = 30


# ------------------------------------------------------------------ H7 spectral diffusion
def clamp_time(t, clamp):
    """t f32 [C] -> the diffusion times the kernel uses (f32): max(t, 1e-8f) if clamp."""
    return torch.clamp(t, min=T_MIN) if clamp else t


def _E(evals, tc, dtype):
    return torch.exp(-evals.to(dtype).unsqueeze(-1) * tc.to(dtype))  # [B, K, C]


def diffusion(x, mass, evals, evecs, t, clamp=False, dtype=torch.float64):
    """mode 0: spec = Phi^T (m ⊙ x), y = Phi (E ⊙ spec), E[k, c] = exp(-evals_k t_c).
    x [B,N,C], mass [B,N], evals [B,K], evecs [B,N,K], t [C] -> (y, spec, clamped t (f32))."""
    tc = clamp_time(t, clamp)
    phi = evecs.to(dtype)
    spec = phi.transpose(-2, -1) @ (x.to(dtype) * mass.to(dtype).unsqueeze(-1))
    y = phi @ (_E(evals, tc, dtype) * spec)
    return y, spec, tc


def diffusion_bwd(g, mass, evals, evecs, tc, spec, dtype=torch.float64):
    """mode 1 for an incoming gradient g [B,N,C] and the forward's spec [B,K,C]:
    gs = Phi^T g, gx = m ⊙ Phi (E ⊙ gs), gt_c = -sum_b sum_k evals_k E[k,c] spec[k,c] gs[k,c]."""
    phi = evecs.to(dtype)
    E = _E(evals, tc, dtype)
    gs = phi.transpose(-2, -1) @ g.to(dtype)
    gx = (phi @ (E * gs)) * mass.to(dtype).unsqueeze(-1)
    gt = -(evals.to(dtype).unsqueeze(-1) * E * spec.to(dtype) * gs).sum((0, 1))
    return gx, gt


def diffusion_bounds(x, g, mass, evals, evecs, tc):
    """fp64 componentwise bounds (by, braw, bx, bt) of y, spec, gx, gt."""
    dt = torch.float64
    aphi = evecs.to(dt).abs()
    E = _E(evals, tc, dt)
    braw = aphi.transpose(-2, -1) @ (mass.to(dt).abs().unsqueeze(-1) * x.to(dt).abs())
    by = aphi @ (E * braw)
    bgs = aphi.transpose(-2, -1) @ g.to(dt).abs()
    bx = mass.to(dt).abs().unsqueeze(-1) * (aphi @ (E * bgs))
    bt = (evals.to(dt).abs().unsqueeze(-1) * E * braw * bgs).sum((0, 1))
    return by, braw, bx, bt


# ------------------------------------------------------------------ H9 fmap head
def head_weights(evecs, mass, dtype=torch.float64):
    """W = evecs[..., :30] * mass as an f32 product (the kernel's documented choice), then dtype."""
    return (evecs[..., :K_FMAP].float() * mass.float().unsqueeze(-1)).to(dtype)


def get_mask(evals1, evals2, gamma=0.5, dtype=torch.float64):
    """Resolvent mask for every crop: evals1 [B, K1], evals2 [B, K2] -> D [B, K2, K1],
    D[b, j, i] from evals2[b, j] and evals1[b, i]."""
    e1, e2 = evals1.to(dtype), evals2.to(dtype)
    s = torch.maximum(e1.max(1).values, e2.max(1).values)[:, None]
    g1 = ((e1 / s) ** gamma)[:, None, :]
    g2 = ((e2 / s) ** gamma)[:, :, None]
    re = g2 / (g2 * g2 + 1) - g1 / (g1 * g1 + 1)
    im = 1 / (g2 * g2 + 1) - 1 / (g1 * g1 + 1)
    return re * re + im * im


def fmap_head_fwd(fx, fy, evecs_x, evecs_y, mass_x, mass_y, evals_x, evals_y, gamma=0.5, dtype=torch.float64):
    """fx [B,N1,32], fy [B,N2,32] (any strides), evals [B, >=30] -> A, Bm [B,30,32],
    AAt = A A^T, BAt = Bm A^T, D = get_mask(evals_x[:30], evals_y[:30]) [B,30,30]."""
    Wx, Wy = head_weights(evecs_x, mass_x, dtype), head_weights(evecs_y, mass_y, dtype)
    A = Wx.transpose(1, 2) @ fx.to(dtype)
    Bm = Wy.transpose(1, 2) @ fy.to(dtype)
    D = get_mask(evals_x[:, :K_FMAP], evals_y[:, :K_FMAP], gamma, dtype)
    return A, Bm, A @ A.transpose(1, 2), Bm @ A.transpose(1, 2), D


def fmap_head_fwd_bounds(fx, fy, evecs_x, evecs_y, mass_x, mass_y):
    """fp64 bounds (bA, bBm, bAAt, bBAt): |W|^T |F|, and the products of those bounds (AAt / BAt
    are formed from the rounded A / Bm, whose own error is relative to bA / bBm)."""
    dt = torch.float64
    bA = head_weights(evecs_x, mass_x, dt).abs().transpose(1, 2) @ fx.to(dt).abs()
    bB = head_weights(evecs_y, mass_y, dt).abs().transpose(1, 2) @ fy.to(dt).abs()
    return bA, bB, bA @ bA.transpose(1, 2), bB @ bA.transpose(1, 2)


def fmap_head_bwd(part, dBAt, A, Bm, evecs_x, evecs_y, mass_x, mass_y, dtype=torch.float64):
    """part [B,30,30,30] (pk_fmap_solve_backward's slabs), dBAt [B,30,30], A / Bm [B,30,32] ->
    dA = (dAAt + dAAt^T) A + dBAt^T Bm with dAAt = part.sum(1), dBm = dBAt A,
    dF_x = W_x dA [B,N1,32], dF_y = W_y dBm [B,N2,32]."""
    dAAt = part.to(dtype).sum(1)
    H, A, Bm = dBAt.to(dtype), A.to(dtype), Bm.to(dtype)
    dA = (dAAt + dAAt.transpose(1, 2)) @ A + H.transpose(1, 2) @ Bm
    dBm = H @ A
    return dA, dBm, head_weights(evecs_x, mass_x, dtype) @ dA, head_weights(evecs_y, mass_y, dtype) @ dBm


def fmap_head_bwd_bounds(part, dBAt, A, Bm, evecs_x, evecs_y, mass_x, mass_y):
    """fp64 bounds (bdA, bdBm, bdF_x, bdF_y) of fmap_head_bwd's outputs."""
    dt = torch.float64
    G = part.to(dt).abs().sum(1)
    H, A, Bm = dBAt.to(dt).abs(), A.to(dt).abs(), Bm.to(dt).abs()
    bdA = (G + G.transpose(1, 2)) @ A + H.transpose(1, 2) @ Bm
    bdB = H @ A
    return bdA, bdB, head_weights(evecs_x, mass_x, dt).abs() @ bdA, head_weights(evecs_y, mass_y, dt).abs() @ bdB


# ------------------------------------------------------------------ H9 fmap solve
def solve_matrices(AAt, D, lam, dtype=torch.float64):
    """M[b, i] = AAt_b + lambda diag(D_b[i, :]) -> [B, K, K, K]; lambda as the f32 the kernel gets."""
    lam = float(torch.tensor(lam, dtype=torch.float32))
    return AAt.to(dtype)[:, None] + lam * torch.diag_embed(D.to(dtype))


def fmap_solve(AAt, BAt, D, lam, dtype=torch.float64):
    """C[b, i, :] = M[b, i]^-1 BAt[b, i, :]."""
    return torch.linalg.solve(solve_matrices(AAt, D, lam, dtype), BAt.to(dtype).unsqueeze(-1)).squeeze(-1)


def fmap_solve_bwd(AAt, BAt, D, lam, G, dtype=torch.float64):
    """For symmetric AAt: w_i = M_i^-1 G[b, i, :]; dBAt[b, i, :] = w_i, slabs -w_i x_i^T [B,K,K,K]
    (dL/dAAt = their sum over axis 1)."""
    M = solve_matrices(AAt, D, lam, dtype)
    x = torch.linalg.solve(M, BAt.to(dtype).unsqueeze(-1)).squeeze(-1)
    w = torch.linalg.solve(M.transpose(-2, -1), G.to(dtype).unsqueeze(-1)).squeeze(-1)
    return w, -w.unsqueeze(-1) * x.unsqueeze(-2)


# ------------------------------------------------------------------ the accuracy rule
def err_ratio(got, truth, bound):
    """max |got - truth| / bound over the elements with a positive bound; where the bound is 0
    (every term of the sum vanishes: padded rows) the result must equal the truth exactly."""
    got, truth = got.detach().cpu().to(torch.float64), truth.detach().cpu().to(torch.float64)
    err = (got - truth).abs()
    assert bool(torch.isfinite(got).all()), "non-finite result"
    pos = bound > 0
    assert bool((err[~pos] == 0).all()), "error where the bound vanishes"
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
