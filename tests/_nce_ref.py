"""A plain-torch reference of pk_nce_loss (csrc/nce.hip) for one crop, forward and backward by
explicit formulas (no autograd), and the seeded inputs the NCE tests share.

nce(f1, f2, i1, i2, t, dtype, mm, prenorm) -> (loss, g1, g2) for the crop's valid slots in slot
order: slot a pairs CAD point i1[a] with crop point i2[a].

  q = normalize(f1)[i1], k = normalize(f2)[i2]            (as is under prenorm)
  d[a][o] = |q_a - k_o|;  logits = -d / t;  loss = mean_a (lse_a - logits[a][a])
  r = dL/dd = -(P - I) / (n t d), 0 where d == 0          (torch's cdist backward)
  dq = q sum_o r - R k,  dk = k sum_a r - R^T q           (torch's _euclidean_dist_backward)
  dx = (dv - v (v . dv)) / |x|, dv / 1e-12 where |x| <= 1e-12   (F.normalize's backward, per slot)
  g[p] = sum of the slot rows of point p                   (index_add_, ascending slots)

mm = False takes d as the norm of the difference: in fp64 this is the truth the kernel is held to.
mm = True restates the kernel's arithmetic, d = sqrt(max(|q|^2 + |k|^2 - 2 q.k, 0)), with |.|^2
and q.k summed over the 32 channels in the same order so that a bitwise equal pair gives d == 0
exactly, as the kernel's fmaf chains do: in fp32 on the CPU this is the yardstick whose own error
against the truth scales the GPU bound (e_kernel <= 3 e_yardstick + 1e-5 scale).
n = 0 gives loss 0 and zero gradients (the batched host code's clamp(min=1) convention).
"""
import torch

F64 = torch.float64
F32 = torch.float32
T = 0.07
EPS = 1e-12


def _chain_sq(x):
    s = torch.zeros(x.shape[0], dtype=x.dtype)
    for c in range(x.shape[1]):
        s = s + x[:, c] * x[:, c]
    return s


def _chain_dot(q, k):
    s = torch.zeros((q.shape[0], k.shape[0]), dtype=q.dtype)
    for c in range(q.shape[1]):
        s = s + q[:, c, None] * k[None, :, c]
    return s


def _normalize(f, prenorm):
    if prenorm:
        return f, None
    n = torch.sqrt(_chain_sq(f))
    return f / torch.clamp(n, min=EPS)[:, None], n


def _normalize_bwd(v, dv, n):
    if n is None:
        return dv
    safe = torch.where(n > EPS, n, torch.ones_like(n))
    proj = (dv - v * (v * dv).sum(1, keepdim=True)) / safe[:, None]
    return torch.where((n > EPS)[:, None], proj, dv / EPS)


def nce(f1, f2, i1, i2, t=T, dtype=F64, mm=False, prenorm=False):
    f1, f2 = f1.to(dtype), f2.to(dtype)
    g1, g2 = torch.zeros_like(f1), torch.zeros_like(f2)
    n = int(i1.numel())
    if n == 0:
        return torch.zeros((), dtype=dtype), g1, g2
    v1, n1 = _normalize(f1, prenorm)
    v2, n2 = _normalize(f2, prenorm)
    q, k = v1[i1], v2[i2]
    if mm:
        d2 = (_chain_sq(q)[:, None] + _chain_sq(k)[None, :]) - 2 * _chain_dot(q, k)
        d = torch.sqrt(torch.clamp(d2, min=0))
    else:
        d = (q[:, None, :] - k[None, :, :]).norm(dim=2)
    logits = -d / t
    lse = torch.logsumexp(logits, dim=1)
    loss = (lse - torch.diagonal(logits)).mean()
    G = torch.exp(logits - lse[:, None]) - torch.eye(n, dtype=dtype)
    r = torch.where(d > 0, -G / (n * t * torch.where(d > 0, d, torch.ones_like(d))), torch.zeros_like(d))
    dq = q * r.sum(1, keepdim=True) - r @ k
    dk = k * r.sum(0)[:, None] - r.t() @ q
    g1.index_add_(0, i1, _normalize_bwd(q, dq, None if n1 is None else n1[i1]))
    g2.index_add_(0, i2, _normalize_bwd(k, dk, None if n2 is None else n2[i2]))
    return loss, g1, g2


# ---------------------------------------------------------------- errors and the GPU bound
def scale_free(g, f):
    """A gradient with every point's row multiplied by max(|f_p|, 1e-12) (fp64): d loss / d f_p is
    proportional to 1 / |f_p|, so that without it one tiny-norm row sets the whole scale."""
    return g.to(F64) * torch.clamp(f.to(F64).norm(dim=1), min=EPS)[:, None]


def errors(got, truth, f1, f2):
    """[(name, error, scale)] of one crop's (loss, g1, g2) against the truth: the loss, each side's
    scale-free gradient in the Frobenius norm, and each side's worst single row (against the
    truth's largest row)."""
    out = [("loss", abs(float(got[0]) - float(truth[0])), abs(float(truth[0])))]
    for name, g, gt, f in (("g1", got[1], truth[1], f1), ("g2", got[2], truth[2], f2)):
        a, b = scale_free(g, f), scale_free(gt, f)
        out.append((name + " fro", float((a - b).norm()), float(b.norm())))
        out.append((name + " row", float((a - b).norm(dim=1).max()), float(b.norm(dim=1).max())))
    return out


def rel_error(got, truth, f1, f2):
    """The largest error / scale over errors() (0 / 0 counts as 0)."""
    return max((e / s if s > 0 else (0.0 if e == 0 else float("inf"))) for _, e, s in errors(got, truth, f1, f2))


# ---------------------------------------------------------------- seeded inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gaussian_crop(S, N1, N2, seed):
    """Gaussian features, pair indices drawn with replacement (points in several slots)."""
    g = _gen(seed)
    return dict(f1=torch.randn(N1, 32, generator=g), f2=torch.randn(N2, 32, generator=g),
                i1=torch.randint(0, N1, (S,), generator=g), i2=torch.randint(0, N2, (S,), generator=g))


def converging_crop(eps, S, N, seed):
    """Positive pairs pulled together: f2[i2] = (normalize(f1[i1]) + eps noise / sqrt(32)) s with
    s in [0.5, 1.5], distinct points on both sides; the other crop points stay Gaussian."""
    g = _gen(seed)
    f1, f2 = torch.randn(N, 32, generator=g), torch.randn(N, 32, generator=g)
    i1, i2 = torch.randperm(N, generator=g)[:S], torch.randperm(N, generator=g)[:S]
    s = 0.5 + torch.rand(S, 1, generator=g)
    noise = torch.randn(S, 32, generator=g)
    f2[i2] = (torch.nn.functional.normalize(f1[i1], dim=1) + eps * noise / 32 ** 0.5) * s
    return dict(f1=f1, f2=f2, i1=i1, i2=i2)


def degenerate_crop(S, N, seed):
    """On a Gaussian draw (the loss stays O(1)): 8 diagonal pairs bitwise equal, two slots on the
    same (CAD, crop) pair, one CAD row and one crop row all zero, rows scaled by 10^k, k in [-6, 6]."""
    g = _gen(seed)
    f1, f2 = torch.randn(N, 32, generator=g), torch.randn(N, 32, generator=g)
    i1, i2 = torch.randperm(N, generator=g)[:S], torch.randperm(N, generator=g)[:S]
    k1 = torch.randint(-6, 7, (N, 1), generator=g).float()
    k2 = torch.randint(-6, 7, (N, 1), generator=g).float()
    f1, f2 = f1 * 10.0 ** k1, f2 * 10.0 ** k2
    f2[i2[:8]] = f1[i1[:8]]                  # bitwise equal rows normalize to bitwise equal vectors
    i1[9], i2[9] = i1[8], i2[8]              # slots 8 and 9 on one pair
    f1[i1[10]] = 0.0
    f2[i2[11]] = 0.0
    return dict(f1=f1, f2=f2, i1=i1, i2=i2)


FAMILIES = ("gaussian", "eps1.0", "eps0.7", "eps0.5", "eps0.3", "eps0.03", "degenerate")
# caps of the yardstick's own error (rel_error) per family, held by test_nce_ref_cpu.py
CAPS = {"eps0.03": 5e-2}
CAP_DEFAULT = 1e-3


def family_crops(name):
    """The crops (B = 2: all 512 slots, and 300 of them) of an input family at S = 512, N = 600."""
    if name == "gaussian":
        return [gaussian_crop(512, 600, 600, 100), gaussian_crop(300, 600, 600, 101)]
    if name == "degenerate":
        return [degenerate_crop(512, 600, 110), degenerate_crop(300, 600, 111)]
    eps = float(name[3:])
    return [converging_crop(eps, 512, 600, 120), converging_crop(eps, 300, 600, 121)]


def reference(name):
    """(crops, truths, yardsticks) of a family."""
    crops = family_crops(name)
    truth = [nce(c["f1"], c["f2"], c["i1"], c["i2"]) for c in crops]
    yard = [nce(c["f1"], c["f2"], c["i1"], c["i2"], dtype=F32, mm=True) for c in crops]
    return crops, truth, yard
