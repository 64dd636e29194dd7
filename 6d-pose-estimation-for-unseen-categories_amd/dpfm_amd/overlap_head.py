"""OverlapPredictorNet (modeling/dpfm.py:125-145) for both shapes as one fused autograd node, alone
(`overlap_head`) or together with the refinement's last_lin that feeds it (`lastlin_overlap_head`):
pk_overlap_head_fwd / _bwd, one launch per direction. The weight gradients go through
wgrad.weight_grad: to the training step's grouped launch, or computed here."""
from __future__ import annotations

import ctypes

import torch

from . import _lib, ops
from ._lib import call
from .wgrad import weight_grad


def _ovh_args(fx, fy, w0, b0, w1, b1):
    a = _lib.OverlapHeadArgs()
    for s, f in enumerate((fx, fy)):
        a.x[s] = f.data_ptr()
        for j in range(3):
            a.strides[s][j] = f.stride(j)
        a.N[s] = f.shape[1]
    a.B = fx.shape[0]
    a.w0, a.b0, a.w1, a.b1 = w0.data_ptr(), b0.data_ptr(), w1.data_ptr(), b1.data_ptr()
    return a


def _ovh_forward(fx, fy, w0, b0, w1, b1, want: bool):
    """pk_overlap_head_fwd on both shapes: ((s_x, s_y, nrows_x, nrows_y), the saved tensors)."""
    B = fx.shape[0]
    dev = fx.device
    a = _ovh_args(fx, fy, w0, b0, w1, b1)
    outs = []
    for s, f in enumerate((fx, fy)):
        N = f.shape[1]
        n = torch.empty_strided(f.shape, f.stride(), dtype=torch.float32, device=dev)
        nrm = torch.empty((B * N,), dtype=torch.float32, device=dev)
        nrows = torch.empty((B, N, 32), dtype=torch.float32, device=dev) if want else None
        h = torch.empty((B, N, 32), dtype=torch.float32, device=dev) if want else None
        sc = torch.empty((B, N), dtype=torch.float32, device=dev)
        a.n[s], a.nrm[s] = n.data_ptr(), nrm.data_ptr()
        a.nrows[s] = nrows.data_ptr() if nrows is not None else None
        a.h[s] = h.data_ptr() if h is not None else None
        a.s[s] = sc.data_ptr()
        outs.append((n, nrm, nrows, h, sc))
    call("pk_overlap_head_fwd", ctypes.addressof(a), _lib.stream(dev),
         work=("hbm", 4 * B * (fx.shape[1] + fy.shape[1]) * (32 + 32 + (64 if want else 0) + 2)))
    (nx, nrx, rx, hx, sx), (ny, nry, ry, hy, sy) = outs
    return (sx, sy, rx, ry), (nx, nrx, rx, hx, sx, ny, nry, ry, hy, sy)


def _ovh_backward(saved, params, dsx, dsy, drx, dry, dadd=(None, None)):
    """pk_overlap_head_bwd on both shapes: (d f_x, d f_y (+ dadd, another consumer's gradient of
    the features, added in the launch), the four weight gradients (None where the grouped launch
    takes them))."""
    nx, nrx, rx, hx, sx, ny, nry, ry, hy, sy = saved
    w0, b0, w1, b1 = params
    dev = nx.device
    a = _ovh_args(nx, ny, w0, b0, w1, b1)
    B = nx.shape[0]
    res = []
    for s, (n, nrm, rows, h, sc, ds, dr, da) in enumerate(((nx, nrx, rx, hx, sx, dsx, drx, dadd[0]),
                                                           (ny, nry, ry, hy, sy, dsy, dry, dadd[1]))):
        N = n.shape[1]
        ds = torch.zeros((B, N), dtype=torch.float32, device=dev) if ds is None else ds.contiguous()
        dr = dr.contiguous() if dr is not None else None
        g = torch.empty((B, N, 1), dtype=torch.float32, device=dev)
        dh = torch.empty((B, N, 32), dtype=torch.float32, device=dev)
        dx = torch.empty_strided(n.shape, n.stride(), dtype=torch.float32, device=dev)
        if da is not None and da.stride() != n.stride():
            da = torch.empty_strided(n.shape, n.stride(), dtype=torch.float32, device=dev).copy_(da)
        a.n[s], a.nrm[s], a.h[s], a.s[s] = n.data_ptr(), nrm.data_ptr(), h.data_ptr(), sc.data_ptr()
        a.ds[s], a.dnr[s] = ds.data_ptr(), (dr.data_ptr() if dr is not None else None)
        a.g[s], a.dh[s], a.dx[s] = g.data_ptr(), dh.data_ptr(), dx.data_ptr()
        a.dadd[s] = da.data_ptr() if da is not None else None
        res.append((rows, h, g, dh, dx, ds, dr, da))
    call("pk_overlap_head_bwd", ctypes.addressof(a), _lib.stream(dev),
         work=("hbm", 4 * B * (nx.shape[1] + ny.shape[1]) * (32 * 5 + 4) +
               sum(4 * d.numel() for d in dadd if d is not None)))
    g0 = g1 = None
    for rows, h, g, dh, _, _, _, _ in res:
        g1 = weight_grad(h, g, w1, b1, False, acc=g1)
        g0 = weight_grad(rows, dh, w0, b0, False, acc=g0)
    return res[0][4], res[1][4], *g0, *g1


class _OverlapHeadFn(torch.autograd.Function):
    """OverlapPredictorNet (modeling/dpfm.py:125-145) for both shapes as one autograd node:
    F.normalize -> Linear(32, 32) + ReLU -> Linear(32, 1) + Sigmoid in one launch per direction
    (pk_overlap_head_fwd / _bwd, bit-identical to the per-layer path). Outputs the two score maps
    and the rows copies of the normalized features (the NCE term's input, utils/loss.py:23-24);
    the weight gradients go to the grouped launch (wgrad.GroupedWgrad) or are computed here."""

    @staticmethod
    def forward(ctx, fx, fy, w0, b0, w1, b1):
        outs, saved = _ovh_forward(fx, fy, w0, b0, w1, b1, any(ctx.needs_input_grad))
        ctx.params = (w0, b0, w1, b1)
        ctx.save_for_backward(*saved)
        return outs

    @staticmethod
    def backward(ctx, dsx, dsy, drx, dry):
        return _ovh_backward(ctx.saved_tensors, ctx.params, dsx, dsy, drx, dry)


class _LastLinOverlapFn(torch.autograd.Function):
    """The refinement's last_lin on both shapes (modeling/dpfm.py:111-112, desc.transpose(1, 2)
    read in place: channels-first in and out) and the overlap head on its outputs (:125-145) as
    one node, so the two consumers of the refined features — the overlap head and the fmap head
    (models/dpfm.py:80-90) — meet inside it: the fmap head's gradient enters
    pk_overlap_head_bwd's dadd and the features' total gradient leaves that launch (no autograd
    accumulation kernel), then last_lin's input gradient and grouped weight gradient."""

    @staticmethod
    def forward(ctx, d0, d1, wl, bl, w0, b0, w1, b1):
        w2 = wl.view(wl.shape[0], -1)
        Co, Ci = w2.shape
        ys = [torch.empty((d.shape[0], Co, d.shape[2]), dtype=torch.float32, device=d.device) for d in (d0, d1)]
        ops.linear_ex2(*[a for d, y in zip((d0, d1), ys)
                         for a in ((d, w2, bl, 1, d.shape[0] * d.shape[2], d.shape[2], Ci, Co, y), {})])
        fx, fy = ys[0].transpose(1, 2), ys[1].transpose(1, 2)
        want = any(ctx.needs_input_grad)
        (sx, sy, rx, ry), saved = _ovh_forward(fx, fy, w0, b0, w1, b1, want)
        ctx.params = (w0, b0, w1, b1)
        ctx.lin = (wl, bl)
        ctx.save_for_backward(d0, d1, wl, *saved)
        return ys[0], ys[1], sx, sy, rx, ry

    @staticmethod
    def backward(ctx, gy0, gy1, dsx, dsy, drx, dry):
        sv = ctx.saved_tensors
        d0, d1, wl = sv[:3]
        wl_p, bl = ctx.lin
        w2 = wl.view(wl.shape[0], -1)
        Co, Ci = w2.shape
        dadd = tuple(None if g is None else g.transpose(1, 2) for g in (gy0, gy1))
        dfx, dfy, *g01 = _ovh_backward(sv[3:], ctx.params, dsx, dsy, drx, dry, dadd=dadd)
        dd = [torch.empty_like(d0), torch.empty_like(d1)]
        dys = [df.transpose(1, 2) for df in (dfx, dfy)]  # [B, Co, N] contiguous (y's storage)
        ops.linear_ex2(*[a for d, dy, o in zip((d0, d1), dys, dd)
                         for a in ((dy, w2, None, 1, d.shape[0] * d.shape[2], d.shape[2], Co, Ci, o),
                                   dict(transw=True))])
        # weight gradients: shape 1 first, the order autograd ran the two last_lin calls' backward in
        # (a missing db leaves the running sum as it is: wgrad.weight_grad)
        gl = weight_grad(d1, dys[1], wl_p, bl, True)
        gl = weight_grad(d0, dys[0], wl_p, bl, True, acc=gl)
        return dd[0], dd[1], *gl, *g01


def lastlin_overlap_head(d0: torch.Tensor, d1: torch.Tensor, wl, bl, w0, b0, w1, b1):
    """(y0, y1 [B, 32, N] channels-first last_lin outputs, s_x, s_y, nrows_x, nrows_y): the
    refinement's last_lin + overlap head node (_LastLinOverlapFn)."""
    return _LastLinOverlapFn.apply(d0, d1, wl, bl, w0.contiguous(), b0.contiguous(), w1.contiguous(), b1.contiguous())


def overlap_head(fx: torch.Tensor, fy: torch.Tensor, w0, b0, w1, b1):
    """(s_x [B, N1], s_y [B, N2], nrows_x, nrows_y) of OverlapPredictorNet's score net applied to
    F.normalize(f, dim=-1) of both shapes, f32 [B, N, 32] in rows or channels-first storage."""
    if (fx.dim() != 3 or fy.dim() != 3 or fx.shape[-1] != 32 or fy.shape[-1] != 32 or fx.shape[0] != fy.shape[0]
            or fx.dtype != torch.float32 or fy.dtype != torch.float32):
        raise _lib.PoseKernError("overlap_head takes f32 [B, N, 32] features of both shapes")
    fx, _ = ops._l2_layout(fx)
    fy, _ = ops._l2_layout(fy)
    w0, b0, w1, b1 = (t.contiguous() for t in (w0, b0, w1, b1))
    return _OverlapHeadFn.apply(fx, fy, w0, b0, w1, b1)
