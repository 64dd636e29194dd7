"""The spectral path's kernels, called directly, against the fp64 restatement tests/_spectral_ref.py
at their tile and slab edges: pk_spectral_diffusion (H7) through the raw entry with every argument
under the test's control, pk_fmap_head_fwd / _bwd, and pk_fmap_solve / _backward (H9).

The accuracy rule (every dense comparison below): the error is measured per element as a ratio to
the componentwise bound of _spectral_ref (the same expression with every operand replaced by its
absolute value), and the kernel's largest ratio must not exceed 3 x the largest ratio of the SAME
formula evaluated in fp32 on the CPU against the same fp64 truth, plus a floor of 8 x 2^-24 (at
N = 1 the only error is expf plus two or three roundings, and the CPU's exp is not the device's).
A single dropped row at N = 2100 moves a coefficient by ~1/N of its bound, 5e-4: four orders of
magnitude above either term.

MEASURED (MI355X, units of 2^-24 of the bound, kernel / fp32 CPU reference, maxima per group):
  dense, 15 shapes        y 8.03 / 9.88   raw 2.93 / 4.92   gx 7.81 / 7.22   gt 1.85 / 4.64
  production layout       y 3.48 / 3.21   raw 1.65 / 3.77
  clamp (both settings)   y 1.34 / 2.50   raw 1.79 / 2.14   gx 1.27 / 1.82   gt 0.01 / 0.03
  padded crops            y 4.94 / 4.94   raw 2.12 / 4.12   gx 5.17 / 4.48   gt 0.03 / 0.06
  autograd wrapper        y 3.48 / 3.21                     gx 2.55 / 2.92   gt 0.16 / 0.12
  fmap head, 10 cases     A 4.14 / 4.14   Bm 4.47 / 4.47   AAt 5.50 / 5.50   BAt 1.32 / 1.32
                          dA 1.71 / 1.71  dBm 3.51 / 3.51  dF_x 0.16 / 0.16  dF_y 1.16 / 1.16
The largest kernel ratio anywhere is 8.03 x 2^-24 = 4.8e-7 of the bound (y at N = 3, where the fp32
reference itself is at 9.88): a factor 20 inside the project's 1e-5 x bound precedent
(test_linear_wgrad). Per-shape figures are in the docstrings of test_spectral_dense_fp64 and
test_fmap_head_direct. fmap solve: the componentwise residual and slab bounds hold in every case;
against torch.linalg.solve in fp64 the kernel's C / dBAt / dAAt errors were <= 4.6e-7 / 4.6e-7 /
6.0e-6 where the fp32 solve's were 1.7e-4 / 1.5e-4 / 9.6e-4 (B = 3, lambda = 0). ops.fmap_head end to
end: C 1.33e-6 / 1.37e-6, dfx 1.97e-6 / 2.15e-6, dfy 4.10e-7 / 4.10e-7 (absolute, kernel / fp32).
"""
import ctypes
import functools
import itertools
from types import SimpleNamespace

import pytest
import torch

import _spectral_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
FLOOR = 8 * R.U24
NAN = float("nan")


def _p(t, off=0):
    """Device address of element `off` of t's storage view (None passes NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)


def _check(tag, name, got, truth, ref32, bound):
    rk, rr = R.err_ratio(got, truth, bound), R.err_ratio(ref32, truth, bound)
    print(f"[spectral-fp64] {tag} {name}: kernel {rk / R.U24:.2f} fp32ref {rr / R.U24:.2f}")
    assert rk <= 3 * rr + FLOOR, (tag, name, rk / R.U24, rr / R.U24)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------ H7 spectral diffusion
T_CLAMP = [-1.0, 0.0, 1e-9, 1e-8, 1e-3, 2.0]


@functools.lru_cache(maxsize=None)
def _inputs(B, N, tkind="rand"):
    """Random Phi (lbo_operators cannot build 64 orthonormal columns for N < 64), positive mass,
    sorted evals with evals[:, 0] = 0 and evals[:, 63] = 100, so that with t[5] = 2 one (k, c)
    pair has lambda t = 200 and E underflows in fp32."""
    g = torch.Generator().manual_seed(1000 * B + N)
    c = SimpleNamespace(B=B, N=N)
    c.evecs = torch.randn(B, N, 64, generator=g) / N ** 0.5
    c.mass = torch.rand(B, N, generator=g) + 0.1
    c.evals = torch.sort(torch.rand(B, 64, generator=g) * 20, dim=1).values
    c.evals[:, 0] = 0.0
    c.evals[:, 63] = 100.0
    c.x = torch.randn(B, N, 64, generator=g)
    c.g = torch.randn(B, N, 64, generator=g)
    if tkind == "rand":
        c.t = torch.rand(64, generator=g) * 5 + 0.01
        c.t[5] = 2.0
    else:
        vals = T_CLAMP if tkind == "clamp" else T_CLAMP[1:]
        c.t = torch.tensor([vals[i % len(vals)] for i in range(64)], dtype=F32)
    return c


@functools.lru_cache(maxsize=None)
def _forward_ref(B, N, tkind="rand", clamp=False):
    """The forward's truth, fp32 yardstick and bounds, computed once per case."""
    c = _inputs(B, N, tkind)
    r = SimpleNamespace()
    r.y, r.spec, r.tc = R.diffusion(c.x, c.mass, c.evals, c.evecs, c.t, clamp)
    r.y32, r.spec32, _ = R.diffusion(c.x, c.mass, c.evals, c.evecs, c.t, clamp, dtype=F32)
    r.by, r.braw, r.bx, r.bt = R.diffusion_bounds(c.x, c.g, c.mass, c.evals, c.evecs, r.tc)
    return r


def _spectral(dev, src, ld_in, mass, evecs, evals, t, mode, out, ld_out, *, clamp=0, raw=None, saved=None, gt=None,
              acc=0, work=None, scaled=None, B=None, N=None, K=64, C=64):
    """pk_spectral_diffusion with the test's own buffers (src / out: (tensor, element offset))."""
    from dpfm_amd import _lib
    B = mass.shape[0] if B is None else B
    N = mass.shape[1] if N is None else N
    if work is None:
        work = torch.empty((max(B, 1), max((N + 63) // 64, 1), 64, 64), dtype=F32, device=dev)
    if scaled is None:
        scaled = torch.empty((max(B, 1), 64, 64), dtype=F32, device=dev)
    _lib.call("pk_spectral_diffusion", _p(*src), ld_in, _p(mass), _p(evecs), _p(evals), _p(t), int(clamp), B, N, K, C,
              mode, _p(work), _p(raw), _p(scaled), _p(saved), _p(gt), _p(*out), ld_out, int(acc), _lib.stream(dev))


def _both_modes(dev, c, clamp=0, t=None):
    """Mode 0 then mode 1 (saved = the kernel's own raw) on contiguous buffers -> CPU results."""
    B, N = c.B, c.N
    m, ev, el = c.mass.to(dev), c.evecs.to(dev), c.evals.to(dev)
    t = c.t.to(dev) if t is None else t
    y = torch.empty((B, N, 64), dtype=F32, device=dev)
    raw = torch.empty((B, 64, 64), dtype=F32, device=dev)
    _spectral(dev, (c.x.to(dev),), 64, m, ev, el, t, 0, (y,), 64, clamp=clamp, raw=raw)
    t_fwd = t.clone()
    gx, gt = torch.empty_like(y), torch.empty((64,), dtype=F32, device=dev)
    _spectral(dev, (c.g.to(dev),), 64, m, ev, el, t, 1, (gx,), 64, clamp=clamp, saved=raw, gt=gt)
    return SimpleNamespace(y=y.cpu(), raw=raw.cpu(), gx=gx.cpu(), gt=gt.cpu(), t_fwd=t_fwd.cpu(), t=t.cpu())


def _check_both(tag, c, r, k):
    """The accuracy rule on y, raw (mode 0) and gx, gt (mode 1, with the kernel's raw as saved)."""
    _check(tag, "y", k.y, r.y, r.y32, r.by)
    _check(tag, "raw", k.raw, r.spec, r.spec32, r.braw)
    gx, gt = R.diffusion_bwd(c.g, c.mass, c.evals, c.evecs, r.tc, k.raw)
    gx32, gt32 = R.diffusion_bwd(c.g, c.mass, c.evals, c.evecs, r.tc, k.raw, dtype=F32)
    _check(tag, "gx", k.gx, gx, gx32, r.bx)
    _check(tag, "gt", k.gt, gt, gt32, r.bt)


SHAPES = ([(3, n) for n in (1, 3, 63, 64, 65, 255, 256, 257, 513, 2100)] + [(b, 65) for b in (1, 8, 9, 17)] +
          [(2, 2100)])


@pytest.mark.parametrize("B,N", SHAPES)
def test_spectral_dense_fp64(device, B, N):
    """Both modes at the smallest shapes that reach every branch: S = ceil(N / 256) = 1, 2, 3, 9
    slabs (the 8-slab body of the combine plus its tail at N = 2100), a last 64-row chunk with 1,
    63 or 64 live rows, the 8-crop groups of the dL/dt sum plus a tail (B = 8, 9, 17), and grids
    of 1, 2, ... blocks through the XCD block remap.
    Measured on an MI355X, max |error| / bound in units of 2^-24, kernel / fp32 CPU reference:
      B   N       y           raw         gx          gt
      3    1   7.50/8.59   1.81/1.81   7.64/7.22   1.85/4.64
      3    3   8.03/9.88   2.93/2.93   7.81/5.87   1.32/1.04
      3   63   2.72/4.69   1.89/3.96   2.84/2.47   0.20/0.29
      3   64   2.63/3.89   1.62/3.41   2.93/2.88   0.07/0.08
      3   65   3.48/3.21   1.58/3.77   2.55/2.92   0.10/0.14
      3  255   1.66/2.03   1.28/2.17   2.21/2.03   0.03/0.04
      3  256   1.97/1.62   1.55/2.94   1.96/2.56   0.02/0.03
      3  257   3.38/2.86   1.65/2.85   1.68/2.09   0.03/0.03
      3  513   1.66/2.40   1.10/2.14   1.72/1.88   0.01/0.01
      3 2100   0.82/0.84   0.46/0.94   0.68/0.72   0.00/0.02
      1   65   3.10/3.22   2.01/3.91   3.12/4.02   0.15/0.28
      8   65   3.19/3.19   1.84/4.48   3.85/4.14   0.04/0.06
      9   65   4.36/5.41   2.00/4.92   3.53/3.53   0.05/0.06
     17   65   3.42/4.22   1.97/4.87   3.44/4.75   0.03/0.06
      2 2100   0.66/0.80   0.37/0.82   0.53/0.63   0.00/0.01
    """
    c, r = _inputs(B, N), _forward_ref(B, N)
    _check_both(f"dense B={B} N={N}", c, r, _both_modes(device, c))


@pytest.mark.parametrize("N", [65, 257])
def test_spectral_production_layout(device, N):
    """diffusion_net.py's configuration: input and output are the two halves of one [B, N, 128]
    buffer (ld 128), clamp_t = 1. The input half stays bit-unchanged; with ld_out = 68 into a
    NaN-prefilled buffer the 4 columns past the output keep their NaN bit pattern."""
    B = 3
    c, r = _inputs(B, N), _forward_ref(B, N)
    m, ev, el, t = c.mass.to(device), c.evecs.to(device), c.evals.to(device), c.t.to(device)
    cat = torch.randn(B, N, 128, generator=torch.Generator().manual_seed(N))
    cat[..., :64] = c.x
    catd = cat.to(device)
    raw = torch.empty((B, 64, 64), dtype=F32, device=device)
    _spectral(device, (catd,), 128, m, ev, el, t, 0, (catd, 64), 128, clamp=1, raw=raw)
    got = catd.cpu()
    assert torch.equal(_bits(got[..., :64]), _bits(c.x))
    assert torch.equal(_bits(t), _bits(c.t))  # positive times: the clamp's write-back changes nothing
    _check(f"cat128 N={N}", "y", got[..., 64:], r.y, r.y32, r.by)
    _check(f"cat128 N={N}", "raw", raw.cpu(), r.spec, r.spec32, r.braw)
    wide = torch.full((B, N, 68), NAN, dtype=F32, device=device)
    before = _bits(wide[..., 64:])
    _spectral(device, (catd,), 128, m, ev, el, t, 0, (wide,), 68, clamp=1)
    assert torch.equal(_bits(wide[..., 64:]), before)
    assert torch.equal(_bits(wide[..., :64]), _bits(got[..., 64:]))  # the row stride changes no value


def test_spectral_accumulate(device):
    """accumulate: out = p + result with one extra rounded add, in both modes; dL/dt unaffected."""
    B, N = 3, 257
    c = _inputs(B, N)
    m, ev, el, t = c.mass.to(device), c.evecs.to(device), c.evals.to(device), c.t.to(device)
    k = _both_modes(device, c)
    p = torch.randn(B, N, 64, generator=torch.Generator().manual_seed(5))
    out = p.to(device)
    _spectral(device, (c.x.to(device),), 64, m, ev, el, t, 0, (out,), 64, acc=1)
    gout, gt = p.to(device), torch.empty((64,), dtype=F32, device=device)
    _spectral(device, (c.g.to(device),), 64, m, ev, el, t, 1, (gout,), 64, saved=k.raw.to(device), gt=gt, acc=1)
    for name, got, plain in (("y", out, k.y), ("gx", gout, k.gx)):
        want = p.double() + plain.double()
        err = (got.cpu().double() - want).abs()
        assert bool((err <= R.U24 * want.abs()).all()), (name, float((err / want.abs()).max()))
    assert torch.equal(_bits(gt), _bits(k.gt))


def test_spectral_clamp(device):
    """Diffusion times below, at and above the clamp, B = 3 and N = 300 so that several blocks read
    t while crop 0's first block writes it. clamp_t = 1: mode 0 leaves t bitwise clamp(t0, 1e-8)
    and every result is the reference at the clamped times; mode 1 on an unclamped copy uses the
    clamped times and leaves t alone. clamp_t = 0 on non-negative times leaves t bit-unchanged."""
    B, N = 3, 300
    c, r = _inputs(B, N, "clamp"), _forward_ref(B, N, "clamp", True)
    k = _both_modes(device, c, clamp=1)
    assert torch.equal(_bits(k.t_fwd), _bits(torch.clamp(c.t, min=1e-8))) and torch.equal(_bits(k.t), _bits(k.t_fwd))
    assert torch.equal(_bits(k.t_fwd), _bits(r.tc))
    _check_both("clamp=1", c, r, k)
    # mode 1 alone, from the unclamped times
    t0 = c.t.to(device)
    gx, gt = torch.empty((B, N, 64), dtype=F32, device=device), torch.empty((64,), dtype=F32, device=device)
    _spectral(device, (c.g.to(device),), 64, c.mass.to(device), c.evecs.to(device), c.evals.to(device), t0, 1, (gx,),
              64, clamp=1, saved=k.raw.to(device), gt=gt)
    assert torch.equal(_bits(t0), _bits(c.t))
    assert torch.equal(_bits(gx), _bits(k.gx)) and torch.equal(_bits(gt), _bits(k.gt))
    # no clamp asked for
    c0, r0 = _inputs(B, N, "nonneg"), _forward_ref(B, N, "nonneg", False)
    k0 = _both_modes(device, c0, clamp=0)
    assert torch.equal(_bits(k0.t), _bits(c0.t)) and torch.equal(_bits(k0.t_fwd), _bits(c0.t))
    _check_both("clamp=0", c0, r0, k0)


def test_spectral_padded_crops(device):
    """Crops of 300, 2 and 65 real rows in N = 300, padded as collate pads (mass = 0, evecs = 0):
    padded rows of y and gx are exactly 0, real rows obey the accuracy rule against the reference
    run on the unpadded crop alone, dL/dt against the sum of the crops' references."""
    B, N, lens = 3, 300, (300, 2, 65)
    base = _inputs(B, N)
    c = SimpleNamespace(**vars(base))
    c.mass, c.evecs = base.mass.clone(), base.evecs.clone()
    for b, n in enumerate(lens):
        c.mass[b, n:] = 0.0
        c.evecs[b, n:] = 0.0
    k = _both_modes(device, c)
    gt, gt32, bt = torch.zeros(64, dtype=F64), torch.zeros(64, dtype=F32), torch.zeros(64, dtype=F64)
    for b, n in enumerate(lens):
        assert bool((k.y[b, n:] == 0).all()) and bool((k.gx[b, n:] == 0).all())
        a = [v[b:b + 1, :n] for v in (c.x, c.g, c.mass)] + [c.evals[b:b + 1], c.evecs[b:b + 1, :n]]
        x, g, m, el, ev = a
        y, spec, tc = R.diffusion(x, m, el, ev, c.t)
        y32, spec32, _ = R.diffusion(x, m, el, ev, c.t, dtype=F32)
        by, braw, bx, btb = R.diffusion_bounds(x, g, m, el, ev, tc)
        tag = f"padded len={n}"
        _check(tag, "y", k.y[b:b + 1, :n], y, y32, by)
        _check(tag, "raw", k.raw[b:b + 1], spec, spec32, braw)
        gxb, gtb = R.diffusion_bwd(g, m, el, ev, tc, k.raw[b:b + 1])
        gx32, gtb32 = R.diffusion_bwd(g, m, el, ev, tc, k.raw[b:b + 1], dtype=F32)
        _check(tag, "gx", k.gx[b:b + 1, :n], gxb, gx32, bx)
        gt, gt32, bt = gt + gtb, gt32 + gtb32, bt + btb
    _check("padded", "gt", k.gt, gt, gt32, bt)


def test_spectral_scratch_independent_and_deterministic(device):
    """work sized as the header states ([B, ceil(N / 64), K, C]); work, scaled and the outputs
    prefilled with 0, NaN and 1e30 in turn, twice each: finite, bit-identical results."""
    B, N = 9, 513
    c = _inputs(B, N)
    m, ev, el, t = c.mass.to(device), c.evecs.to(device), c.evals.to(device), c.t.to(device)
    x, g = c.x.to(device), c.g.to(device)
    res = []
    for fill in (0.0, NAN, 1e30, 0.0, NAN, 1e30):
        full = lambda *s: torch.full(s, fill, dtype=F32, device=device)  # noqa: E731
        work, scaled = full(B, (N + 63) // 64, 64, 64), full(B, 64, 64)
        y, raw = full(B, N, 64), full(B, 64, 64)
        _spectral(device, (x,), 64, m, ev, el, t, 0, (y,), 64, raw=raw, work=work, scaled=scaled)
        work.fill_(fill)
        scaled.fill_(fill)
        gx, gt = full(B, N, 64), full(64)
        _spectral(device, (g,), 64, m, ev, el, t, 1, (gx,), 64, saved=raw, gt=gt, work=work, scaled=scaled)
        res.append([v.cpu() for v in (y, raw, gx, gt)])
    for r in res:
        for a, b in zip(res[0], r):
            assert bool(torch.isfinite(b).all()) and torch.equal(_bits(a), _bits(b))


def test_spectral_degenerate_and_rejected_arguments(device):
    """B = 0 and N = 0 return OK and touch nothing; unsupported arguments are rejected by the
    entry point's argument checks (which return before any launch)."""
    from dpfm_amd import _lib
    c = _inputs(3, 65)
    m, ev, el, t = c.mass.to(device), c.evecs.to(device), c.evals.to(device), c.t.to(device)
    x = c.x.to(device)
    for B, N in ((0, 65), (3, 0), (0, 0)):
        bufs = [torch.full((3, 65, 64), 7.0, dtype=F32, device=device) for _ in range(2)]
        bufs += [torch.full((3, 64, 64), 7.0, dtype=F32, device=device) for _ in range(2)]
        y, work, raw, scaled = bufs
        t1 = t.clone()
        _spectral(device, (x,), 64, m, ev, el, t1, 0, (y,), 64, clamp=1, raw=raw, work=work, scaled=scaled, B=B, N=N)
        assert all(bool((v == 7.0).all()) for v in bufs) and torch.equal(t1, t)
    y = torch.empty((3, 65, 64), dtype=F32, device=device)
    raw, gt = torch.empty((3, 64, 64), dtype=F32, device=device), torch.empty((64,), dtype=F32, device=device)
    # K = 32; ld_in = 66; ld_out = 60; mode 1 without saved
    for kw, ld_in, mode, ld_out in ((dict(K=32), 64, 0, 64), (dict(), 66, 0, 64), (dict(), 64, 0, 60),
                                    (dict(gt=gt), 64, 1, 64)):
        with pytest.raises(_lib.PoseKernError):
            _spectral(device, (x,), ld_in, m, ev, el, t, mode, (y,), ld_out, raw=raw, **kw)


def test_spectral_autograd_wrapper(device):
    """ops.spectral_diffusion's plumbing of gx / gt at an edge shape, on a contiguous x and on a
    view whose row stride (65) forces the wrapper's .contiguous() branch."""
    from dpfm_amd import ops
    B, N = 3, 65
    c, r = _inputs(B, N), _forward_ref(B, N)
    gx, gt = R.diffusion_bwd(c.g, c.mass, c.evals, c.evecs, r.tc, r.spec)
    gx32, gt32 = R.diffusion_bwd(c.g, c.mass, c.evals, c.evecs, r.tc, r.spec32, dtype=F32)
    m, ev, el = c.mass.to(device), c.evecs.to(device), c.evals.to(device)
    for tag in ("contiguous", "strided"):
        if tag == "contiguous":
            leaf = c.x.to(device).requires_grad_()
            x = leaf
        else:
            leaf = torch.cat([c.x, torch.ones(B, N, 1)], -1).to(device).requires_grad_()
            x = leaf[..., :64]
            assert not x.is_contiguous()
        t = c.t.to(device).requires_grad_()
        y = ops.spectral_diffusion(x, m, el, ev, t)
        (y * c.g.to(device)).sum().backward()
        _check(f"autograd {tag}", "y", y, r.y, r.y32, r.by)
        _check(f"autograd {tag}", "gx", leaf.grad[..., :64], gx, gx32, r.bx)
        _check(f"autograd {tag}", "gt", t.grad, gt, gt32, r.bt)
        if tag == "strided":
            assert bool((leaf.grad[..., 64] == 0).all())


# ------------------------------------------------------------------ H9 fmap head
@functools.lru_cache(maxsize=None)
def _head_inputs(B, N1, N2):
    g = torch.Generator().manual_seed(100000 * B + 1000 * N1 + N2)
    h = SimpleNamespace(B=B, N1=N1, N2=N2)
    h.fx, h.fy = torch.randn(B, N1, 32, generator=g), torch.randn(B, N2, 32, generator=g)
    h.evecs_x = torch.randn(B, N1, 64, generator=g) / N1 ** 0.5
    h.evecs_y = torch.randn(B, N2, 64, generator=g) / N2 ** 0.5
    h.mass_x, h.mass_y = torch.rand(B, N1, generator=g) + 0.1, torch.rand(B, N2, generator=g) + 0.1
    h.evals_x = torch.sort(torch.rand(B, 64, generator=g) * 3, dim=1).values
    h.evals_y = torch.sort(torch.rand(B, 64, generator=g) * 5, dim=1).values
    h.evals_x[:, 0] = 0.0
    h.evals_y[:, 0] = 0.0
    h.part = torch.randn(B, 30, 30, 30, generator=g)
    h.dBAt = torch.randn(B, 30, 30, generator=g)
    return h


def _ref_args(h):
    return dict(evecs_x=h.evecs_x, evecs_y=h.evecs_y, mass_x=h.mass_x, mass_y=h.mass_y)


# (evecs columns stored, evals passed as a [:, :30] slice of [B, 64], features channels-first)
LAYOUTS = [(64, True, False), (30, False, True), (64, True, True), (30, True, False)]
HEAD_SHAPES = [(1, 1), (127, 129), (128, 128), (129, 300), (300, 203)]
HEAD_CASES = [(n1, n2, B) + LAYOUTS[i % 4] for i, ((n1, n2), B) in enumerate(itertools.product(HEAD_SHAPES, (1, 3)))]
GUARD = 64


def _feat(f, cf, dev):
    """Features [B, N, 32] in rows or channels-first storage -> (device tensor, host strides)."""
    B, N, _ = f.shape
    if cf:
        return f.transpose(1, 2).contiguous().to(dev), (ctypes.c_int64 * 3)(32 * N, 1, N)
    return f.contiguous().to(dev), (ctypes.c_int64 * 3)(32 * N, 32, 1)


def _grad_buffer(B, N, cf, dev):
    """A NaN-prefilled, over-allocated gradient buffer: (flat, strides, view [B, N, 32] of its middle)."""
    flat = torch.full((2 * GUARD + B * N * 32,), NAN, dtype=F32, device=dev)
    mid = flat[GUARD:GUARD + B * N * 32]
    if cf:
        return flat, (ctypes.c_int64 * 3)(32 * N, 1, N), mid.view(B, 32, N).transpose(1, 2)
    return flat, (ctypes.c_int64 * 3)(32 * N, 32, 1), mid.view(B, N, 32)


@pytest.mark.parametrize("N1,N2,B,cols,sliced,cf", HEAD_CASES)
def test_fmap_head_direct(device, N1, N2, B, cols, sliced, cf):
    """pk_fmap_head_fwd / _bwd through the C entry points: one 128-point chunk, a chunk boundary
    and unequal chunk counts on the two sides; evecs stored with 64 or exactly 30 columns, evals
    as a slice of [B, 64] or contiguous, features in rows or channels-first storage at the host
    strides. Forward: A, Bm, AAt, BAt under the accuracy rule, D against get_mask in fp64 at
    1e-6 of its maximum, bit-identical for a NaN- and a 1e30-prefilled work buffer. Backward (random
    part / dBAt, the forward's A / Bm): dA, dBm, dF_x, dF_y under the accuracy rule; every
    element of the NaN-prefilled dF written, the memory on both sides of it untouched.
    Measured on an MI355X, max |error| / bound in units of 2^-24, kernel / fp32 CPU reference (the
    two agree where both sum one fmaf chain in the same order):
      N1  N2 B   A         Bm        AAt       BAt       dA        dBm       dF_x      dF_y
       1   1 1   0.96/0.96 0.96/0.96 4.32/4.32 1.32/1.32 0.52/0.37 2.83/2.83 0.11/0.11 0.19/0.16
       1   1 3   0.99/0.99 0.97/0.97 5.50/5.50 1.32/1.32 1.71/1.71 3.18/3.18 0.14/0.12 0.47/0.47
     127 129 1   2.85/2.85 3.01/3.01 0.16/0.16 0.08/0.08 0.50/0.38 2.35/2.35 0.13/0.11 0.87/0.87
     127 129 3   3.33/3.33 3.16/3.16 0.14/0.14 0.08/0.08 0.68/0.36 3.51/3.51 0.14/0.12 0.90/0.90
     128 128 1   2.42/2.42 2.54/2.54 0.15/0.15 0.09/0.09 0.52/0.36 2.23/2.23 0.13/0.11 0.83/0.83
     128 128 3   4.14/4.14 4.47/4.47 0.16/0.16 0.10/0.10 0.72/0.47 2.67/2.67 0.13/0.12 1.16/1.16
     129 300 1   2.85/2.85 2.22/1.94 0.12/0.12 0.05/0.05 0.45/0.32 3.02/3.02 0.10/0.11 0.88/0.88
     129 300 3   2.88/2.88 1.79/1.93 0.16/0.16 0.05/0.06 0.48/0.43 2.92/2.92 0.15/0.13 1.15/1.15
     300 203 1   2.00/1.72 2.94/2.17 0.06/0.05 0.04/0.05 0.52/0.40 2.44/2.44 0.15/0.14 0.75/0.75
     300 203 3   2.21/1.85 2.32/2.42 0.07/0.06 0.04/0.05 0.57/0.42 2.83/2.83 0.16/0.16 0.98/0.98
    """
    from dpfm_amd import _lib
    from dpfm_amd.dpfm_utils import get_mask
    h = _head_inputs(B, N1, N2)
    tag = f"head {N1}x{N2} B={B} cols={cols} sliced={int(sliced)} cf={int(cf)}"
    ex, ey = (e[..., :cols].contiguous().to(device) for e in (h.evecs_x, h.evecs_y))
    mx, my = h.mass_x.to(device), h.mass_y.to(device)
    vx, vy = ((v if sliced else v[:, :30].contiguous()).to(device) for v in (h.evals_x, h.evals_y))
    ldv = 64 if sliced else 30
    (fx, sx), (fy, sy) = _feat(h.fx, cf, device), _feat(h.fy, cf, device)
    wl = int(_lib.lib().pk_fmap_head_work_len(B, N1, N2))
    assert wl == B * ((N1 + 127) // 128 + (N2 + 127) // 128) * 30 * 32
    outs = []
    for fill in (NAN, 1e30):
        work = torch.full((wl,), fill, dtype=F32, device=device)
        o = [torch.full(s, NAN, dtype=F32, device=device) for s in ((B, 30, 32), (B, 30, 32)) + ((B, 30, 30),) * 3]
        _lib.call("pk_fmap_head_fwd", _p(ex), cols, _p(mx), _p(fx), sx, N1, _p(ey), cols, _p(my), _p(fy), sy, N2,
                  _p(vx), ldv, _p(vy), ldv, B, 30, 32, 0.5, *(_p(v) for v in o), _p(work), wl, _lib.stream(device))
        outs.append([v.cpu() for v in o])
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))
    A, Bm, AAt, BAt, D = outs[0]
    truth = R.fmap_head_fwd(h.fx, h.fy, evals_x=h.evals_x, evals_y=h.evals_y, **_ref_args(h))
    ref32 = R.fmap_head_fwd(h.fx, h.fy, evals_x=h.evals_x, evals_y=h.evals_y, dtype=F32, **_ref_args(h))
    bounds = R.fmap_head_fwd_bounds(h.fx, h.fy, **_ref_args(h))
    for name, got, tr, r32, bd in zip(("A", "Bm", "AAt", "BAt"), outs[0], truth, ref32, bounds):
        _check(tag, name, got, tr, r32, bd)
    for b in range(B):
        ref = get_mask(h.evals_x[b, :30].double(), h.evals_y[b, :30].double(), 0.5)
        assert (D[b].double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item() + 1e-12
        assert (truth[4][b] - ref).abs().max().item() <= 1e-12
    # backward
    part, dBAt = h.part.to(device), h.dBAt.to(device)
    dA, dBm = (torch.full((B, 30, 32), NAN, dtype=F32, device=device) for _ in range(2))
    (flx, stx, dfx), (fly, sty, dfy) = _grad_buffer(B, N1, cf, device), _grad_buffer(B, N2, cf, device)
    guard = _bits(flx[:GUARD])
    Ad, Bd = A.to(device), Bm.to(device)
    _lib.call("pk_fmap_head_bwd", _p(part), _p(dBAt), _p(Ad), _p(Bd), _p(ex), cols, _p(mx), N1,
              _p(ey), cols, _p(my), N2, B, 30, 32, _p(dA), _p(dBm), _p(flx, GUARD), stx, _p(fly, GUARD), sty,
              _lib.stream(device))
    for fl in (flx, fly):
        assert torch.equal(_bits(fl[:GUARD]), guard) and torch.equal(_bits(fl[-GUARD:]), guard)
    got = (dA, dBm, dfx, dfy)
    assert all(not bool(torch.isnan(v).any()) for v in got)
    truth = R.fmap_head_bwd(h.part, h.dBAt, A, Bm, **_ref_args(h))
    ref32 = R.fmap_head_bwd(h.part, h.dBAt, A, Bm, dtype=F32, **_ref_args(h))
    bounds = R.fmap_head_bwd_bounds(h.part, h.dBAt, A, Bm, **_ref_args(h))
    for name, gv, tr, r32, bd in zip(("dA", "dBm", "dF_x", "dF_y"), got, truth, ref32, bounds):
        _check(tag, name, gv, tr, r32, bd)


def test_fmap_head_end_to_end(device):
    """ops.fmap_head (head + lambda = 100 solve, forward and backward) at (129, 300), B = 3, against
    fp64 autograd of the reference chain; per output (C, dfx, dfy) within 3 x the error of the same
    chain in fp32 on the CPU, so the solve's amplification sits in the yardstick."""
    from dpfm_amd import ops
    B, N1, N2, lam = 3, 129, 300, 100.0
    h = _head_inputs(B, N1, N2)
    G = torch.randn(B, 30, 30, generator=torch.Generator().manual_seed(8))
    res = []
    for dt in (F64, F32):
        fx, fy = h.fx.clone().to(dt).requires_grad_(), h.fy.clone().to(dt).requires_grad_()
        _, _, AAt, BAt, D = R.fmap_head_fwd(fx, fy, evals_x=h.evals_x, evals_y=h.evals_y, dtype=dt, **_ref_args(h))
        C = torch.linalg.solve(AAt[:, None] + lam * torch.diag_embed(D), BAt.unsqueeze(-1)).squeeze(-1)
        (C * G.to(dt)).sum().backward()
        res.append([v.detach().double() for v in (C, fx.grad, fy.grad)])
    fx, fy = h.fx.to(device).requires_grad_(), h.fy.to(device).requires_grad_()
    C = ops.fmap_head(fx, fy, h.evecs_x.to(device), h.evecs_y.to(device), h.mass_x.to(device), h.mass_y.to(device),
                      h.evals_x.to(device)[:, :30], h.evals_y.to(device)[:, :30], lam, 0.5)
    (C * G.to(device)).sum().backward()
    res.append([v.detach().cpu().double() for v in (C, fx.grad, fy.grad)])
    for name, t, r, d in zip(("C", "dfx", "dfy"), *res):
        e_ref, e_mine, scale = (r - t).abs().max().item(), (d - t).abs().max().item(), t.abs().max().item()
        print(f"[spectral-fp64] fmap_head e2e {name}: kernel {e_mine:.3e} fp32ref {e_ref:.3e} scale {scale:.3e}")
        assert e_mine <= 3 * e_ref + 1e-6 * (1 + scale), (name, e_mine, e_ref)


# ------------------------------------------------------------------ H9 fmap solve
def _solve(dev, AAt, BAt, D, lam):
    from dpfm_amd import _lib
    C = torch.full(BAt.shape, NAN, dtype=F32, device=dev)
    a, b, d = AAt.to(dev), BAt.to(dev), D.to(dev)
    _lib.call("pk_fmap_solve", _p(a), _p(b), _p(d), float(lam), AAt.shape[0], 30, _p(C), _lib.stream(dev))
    return C.cpu()


def _residual_ok(M, x, v, what):
    """|M x - v| <= 2 x 2^-24 (|M| |x|) componentwise: one f32 rounding of the fp64 elimination's
    x, with a factor 2 for the elimination's own growth. Independent of M's conditioning."""
    x = x.double()
    res = ((M @ x.unsqueeze(-1)).squeeze(-1) - v.double()).abs()
    bound = 2 * R.U24 * (M.abs() @ x.abs().unsqueeze(-1)).squeeze(-1)
    assert bool(torch.isfinite(x).all()), what
    assert bool((res <= bound).all()), (what, float((res / bound).max()))


@pytest.mark.parametrize("lam", [0.0, 100.0, 1000.0])
@pytest.mark.parametrize("B", [1, 3])
def test_fmap_solve_spd_edges(device, B, lam):
    """B x 30 systems not a multiple of the 4 waves per block (idle waves in the last block),
    lambda = 0 / 100 / 1000, a mask with an all-zero row, symmetric positive definite AAt. Forward
    and dBAt: the componentwise residual bound. Slabs: |slab[b,i,r,c] + w_r x_c| <= 4 x 2^-24
    |w_r x_c| with the kernels' own f32 w (dBAt) and x (the forward's C) — three roundings plus
    slack, which also pins that forward and backward eliminate identically. Truth: C, dBAt and
    dAAt against torch.linalg.solve in fp64, within 3 x the fp32 solve's error plus the roundings
    the kernel's f32 outputs carry (1 for C / dBAt, 3 per slab element + slack for dAAt)."""
    from dpfm_amd import _lib
    g = torch.Generator().manual_seed(int(lam) + B)
    A = torch.randn(B, 30, 32, generator=g)
    AAt = A @ A.transpose(1, 2)
    AAt = (AAt + AAt.transpose(1, 2)) / 2
    BAt, G = torch.randn(B, 30, 30, generator=g), torch.randn(B, 30, 30, generator=g)
    D = torch.rand(B, 30, 30, generator=g)
    D[:, 4] = 0.0
    M = R.solve_matrices(AAt, D, lam)
    C = _solve(device, AAt, BAt, D, lam)
    _residual_ok(M, C, BAt, "C")
    dBAt = torch.full((B, 30, 30), NAN, dtype=F32, device=device)
    part = torch.full((B, 30, 30, 30), NAN, dtype=F32, device=device)
    a, b, d, gd = (v.to(device) for v in (AAt, BAt, D, G))
    _lib.call("pk_fmap_solve_backward", _p(a), _p(b), _p(d), float(lam), B, 30, _p(gd), _p(dBAt), _p(part),
              _lib.stream(device))
    dBAt, part = dBAt.cpu(), part.cpu()
    _residual_ok(M, dBAt, G, "dBAt")
    wx = dBAt.double().unsqueeze(-1) * C.double().unsqueeze(-2)
    assert bool(((part.double() + wx).abs() <= 4 * R.U24 * wx.abs()).all())
    Ct = R.fmap_solve(AAt, BAt, D, lam)
    wt, st = R.fmap_solve_bwd(AAt, BAt, D, lam, G)
    w32, s32 = R.fmap_solve_bwd(AAt, BAt, D, lam, G, dtype=F32)
    for name, got, t, r, floor in (("C", C, Ct, R.fmap_solve(AAt, BAt, D, lam, dtype=F32), R.U24 * Ct.abs().max()),
                                   ("dBAt", dBAt, wt, w32, R.U24 * wt.abs().max()),
                                   ("dAAt", part.double().sum(1), st.sum(1), s32.double().sum(1),
                                    4 * R.U24 * st.abs().sum(1).max())):
        e_mine, e_ref = (got.double() - t).abs().max().item(), (r.double() - t).abs().max().item()
        print(f"[spectral-fp64] solve B={B} lam={lam:g} {name}: kernel {e_mine:.3e} fp32ref {e_ref:.3e}")
        assert e_mine <= 3 * e_ref + float(floor), (name, e_mine, e_ref)


def test_fmap_solve_off_diagonal_pivots(device):
    """Forward only, lambda = 0, systems whose partial pivoting leaves the diagonal: a row-permuted
    diagonally dominant matrix, a matrix with zero diagonal, and one whose first column holds its
    maximum magnitude twice (+5 in row 3, -5 in row 7: the lowest row index wins the tie). The
    residual bound needs no reference solve and holds whatever the conditioning."""
    g = torch.Generator().manual_seed(21)
    M0 = (torch.randn(30, 30, generator=g) + 40 * torch.eye(30)).roll(7, 0)
    M1 = torch.randn(30, 30, generator=g)
    M1.fill_diagonal_(0.0)
    M2 = torch.randn(30, 30, generator=g).clamp(-1, 1)
    M2[3, 0], M2[7, 0] = 5.0, -5.0
    for AAt in (torch.stack([M0, M1, M2]), M1[None]):
        B = AAt.shape[0]
        BAt, D = torch.randn(B, 30, 30, generator=g), torch.rand(B, 30, 30, generator=g)
        C = _solve(device, AAt, BAt, D, 0.0)
        _residual_ok(R.solve_matrices(AAt, D, 0.0), C, BAt, f"pivot B={B}")
