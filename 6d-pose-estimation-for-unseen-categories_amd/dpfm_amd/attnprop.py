"""One fused autograd node per AttentionalPropagation call of the cross-attention refinement,
with its residual update (reference modeling/dpfm.py:45-82 and :101-103):

    desc' = desc + mlp(cat(desc, merge(attention(Pq desc, Pk src, Pv src))))

The module path (modeling/dpfm.py here) issues, per call, three projection launches, the
attention, the merge, a concatenation, the MLP (two layers + InstanceNorm/ReLU) and the residual
add forward; backward adds the slices' copies and the gradient accumulations of desc and src.
This node issues (forward) q, the stacked key/value projection (one 32 -> 64 launch reading
`src` once, pk_linear_ex w2), the attention on the stacked buffer (batch strides), the merge
written straight into the concatenation buffer, a copy of desc beside it (pk_copy_rows), mlp.0,
InstanceNorm+ReLU and mlp.3 with the residual in its epilogue; backward: mlp.3^T, the norm
backward, mlp.0^T, the merge^T reading its slice in place, the attention backward writing dk / dv
into one stacked buffer, Pq^T with BOTH other contributions to d desc (the residual and the
concatenation slice) added in its epilogue (add / add2), and [Pk; Pv]^T as one 64 -> 32 launch.
Weight gradients go to the grouped launch (wgrad.GroupedWgrad) reading the stacked / sliced
operands in place (pk_wgrad_call batch strides). Parameters and their names are the module's.

At C = 32, unmasked, with rows of at most ops.ATTN_MLP_MAX_N points, the launches around the
InstanceNorm are fused (ATTN_MLP_FUSE): forward, the copy + merge + mlp.0 + InstanceNorm/ReLU are
one entry point (pk_attn_mlp_fwd: one launch when hc / h1 are not kept, else a per-point chain
launch and the norm launch); backward, mlp.3^T + the norm backward are one (pk_attn_mlp_bwd_norm)
and mlp.0^T + merge^T another (pk_attn_mlp_bwd_in). Every tensor is bit-identical either way."""
from __future__ import annotations

import os

import torch

from . import _lib, ops
from ._lib import call, ptr
from .wgrad import weight_grad


# True: the fused launches of the MLP around the attention, both directions; "fwd" / "bwd": that
# direction only; False (PK_ATTN_MLP_FUSE=0 at import): the per-layer launches.
ATTN_MLP_FUSE = {"0": False, "fwd": "fwd", "bwd": "bwd"}.get(os.environ.get("PK_ATTN_MLP_FUSE", "1"), True)


def _mlp_fused(direction: str, C: int, N: int, masked: bool) -> bool:
    """Whether this call's MLP launches of `direction` ("fwd" / "bwd") take the fused kernels."""
    return (ATTN_MLP_FUSE in (True, direction) and C == ops.ATTN_MLP_C and not masked
            and N <= ops.ATTN_MLP_MAX_N)


def _prop_fwd(x, src, P, heads, eps, nx=None, nsrc=None, keep=True):
    """desc' = x + layer(x, src) in the launches above; returns (desc', saved tensors).
    keep=False (no backward will run): the fused MLP launch does not store hc and h1, which only
    the backward reads (they are None in the returned tuple).
    nx / nsrc (masked mode; int32 [B] on the device or None): the real points of x (the queries,
    and the rows the norm's statistics run over) and of src (the keys) — the attention and the norm
    then go to their varlen entry points (ops.*_raw); every other launch is per point."""
    wq, bq, wk, bk, wv, bv, wm, bm, w0, b0, w3, b3 = P
    B, C, N = x.shape
    M = src.shape[2]
    D = C // heads
    dev = x.device
    f = lambda w: w.view(w.shape[0], -1)  # noqa: E731  Conv1d [O, I, 1] -> [O, I]
    q = torch.empty((B, C, N), dtype=torch.float32, device=dev)
    kv = torch.empty((B, 2 * C, M), dtype=torch.float32, device=dev)
    # the query and the stacked key / value projections: independent, one launch (pk_linear_ex2)
    ops.linear_ex2((x, f(wq), bq, 1, B * N, N, C, C, q), {},
                   (src, f(wk), bk, 1, B * M, M, C, 2 * C, kv), dict(w2=f(wv), bias2=bv, wsplit=C))
    a = torch.empty((B, C, N), dtype=torch.float32, device=dev)
    lse = torch.empty((B, heads, N, 2), dtype=torch.float32, device=dev)
    masked = nx is not None or nsrc is not None
    ops.attention_fwd_raw(q, kv[:, :C], kv[:, C:], B, D, heads, N, M, a, lse, nx, nsrc, ldkv=2 * C * M)
    h1n = torch.empty((B, 2 * C, N), dtype=torch.float32, device=dev)
    mean = torch.empty((B * 2 * C,), dtype=torch.float32, device=dev)
    invstd = torch.empty_like(mean)
    hc = h1 = None
    if _mlp_fused("fwd", C, N, masked):
        if keep:
            hc = torch.empty((B, 2 * C, N), dtype=torch.float32, device=dev)  # cat(desc, message)
            h1 = torch.empty((B, 2 * C, N), dtype=torch.float32, device=dev)
        ops.attn_mlp_fwd(x, a, f(wm), bm, f(w0), b0, eps, h1n, mean, invstd, hc=hc, h1=h1)
    else:
        hc = torch.empty((B, 2 * C, N), dtype=torch.float32, device=dev)  # cat(desc, message)
        call("pk_copy_rows", ptr(hc), 2 * C * N, ptr(x), C * N, B, C * N, _lib.stream(dev),
             work=("hbm", 8 * B * C * N))
        ops.linear_ex(a, f(wm), bm, 1, B * N, N, C, C, y=hc[:, C:], ldy=2 * C * N)
        h1 = torch.empty((B, 2 * C, N), dtype=torch.float32, device=dev)
        ops.linear_ex(hc, f(w0), b0, 1, B * N, N, 2 * C, 2 * C, y=h1)
        ops.instnorm_relu_fwd_raw(h1, B * 2 * C, N, eps, h1n, mean, invstd, 2 * C, nx, varlen=masked)
    out = torch.empty((B, C, N), dtype=torch.float32, device=dev)
    ops.linear_ex(h1n, f(w3), b3, 1, B * N, N, 2 * C, C, y=out, add=x, add_cols=C)
    return out, (x, src, q, kv, a, lse, hc, h1, h1n, mean, invstd)


def _prop_bwd(saved, P, heads, dout, dsrc_add=None, nx=None, nsrc=None):
    """Gradients of one call: (d x, d src (+ dsrc_add, added in the launch's epilogue), the 12
    parameter gradients — None where the active GroupedWgrad takes them)."""
    x, src, q, kv, a, lse, hc, h1, h1n, mean, invstd = saved
    wq, bq, wk, bk, wv, bv, wm, bm, w0, b0, w3, b3 = P
    B, C, N = x.shape
    M = src.shape[2]
    D = C // heads
    dev = x.device
    f = lambda w: w.view(w.shape[0], -1)  # noqa: E731
    dout = dout.contiguous()
    masked = nx is not None or nsrc is not None
    dh1 = torch.empty((B, 2 * C, N), dtype=torch.float32, device=dev)
    dhc = torch.empty((B, 2 * C, N), dtype=torch.float32, device=dev)
    da = torch.empty((B, C, N), dtype=torch.float32, device=dev)
    if _mlp_fused("bwd", C, N, masked):
        # mlp.3^T + the norm backward, then mlp.0^T + merge^T: two launches, dh1n never stored
        ops.attn_mlp_bwd_norm(dout, f(w3), h1, mean, invstd, dh1)
        g_w3, g_b3 = weight_grad(h1n, dout, w3, b3, True)
        ops.attn_mlp_bwd_in(dh1, f(w0), f(wm), dhc, da)
        g_w0, g_b0 = weight_grad(hc, dh1, w0, b0, True)
    else:
        # mlp.3 (its residual: dout flows to desc unchanged, added in Pq^T's epilogue below)
        dh1n = torch.empty((B, 2 * C, N), dtype=torch.float32, device=dev)
        ops.linear_ex(dout, f(w3), None, 1, B * N, N, C, 2 * C, y=dh1n, transw=True)
        g_w3, g_b3 = weight_grad(h1n, dout, w3, b3, True)
        ops.instnorm_relu_bwd_raw(h1, dh1n, mean, invstd, B * 2 * C, N, dh1, 2 * C, nx, varlen=masked)
        ops.linear_ex(dh1, f(w0), None, 1, B * N, N, 2 * C, 2 * C, y=dhc, transw=True)
        g_w0, g_b0 = weight_grad(hc, dh1, w0, b0, True)
        # merge^T on the message half of the concatenation gradient, read in place
        ops.linear_ex(dhc[:, C:], f(wm), None, 1, B * N, N, C, C, y=da, transw=True, ldx=2 * C * N)
    g_wm, g_bm = weight_grad(a, dhc[:, C:], wm, bm, True)
    # attention backward: dk / dv into one stacked buffer
    dq = torch.empty((B, C, N), dtype=torch.float32, device=dev)
    dkv = torch.empty((B, 2 * C, M), dtype=torch.float32, device=dev)
    ops.attention_bwd_raw(q, kv[:, :C], kv[:, C:], a, da, lse, B, D, heads, N, M, dq, dkv[:, :C], dkv[:, C:],
                          nx, nsrc, ldkv=2 * C * M)
    # d desc = Pq^T dq + dout (residual) + dhc[:, :C] (concatenation) and d src = Pk^T dk + Pv^T dv
    # (+ the source's other gradient; the stacked weight's transpose, 64 -> 32): independent, one
    # launch (pk_linear_ex2)
    dx = torch.empty((B, C, N), dtype=torch.float32, device=dev)
    dsrc = torch.empty((B, C, M), dtype=torch.float32, device=dev)
    if dsrc_add is not None:
        dsrc_add = dsrc_add.contiguous()
    ops.linear_ex2((dq, f(wq), None, 1, B * N, N, C, C, dx),
                   dict(transw=True, add=dout, add_cols=C, add2=dhc[:, :C], lda2=2 * C * N),
                   (dkv, f(wk), None, 1, B * M, M, 2 * C, C, dsrc),
                   dict(transw=True, w2=f(wv), wsplit=C, add=dsrc_add, add_cols=C if dsrc_add is not None else 0))
    g_wq, g_bq = weight_grad(x, dq, wq, bq, True)
    g_wk, g_bk = weight_grad(src, dkv[:, :C], wk, bk, True)
    g_wv, g_bv = weight_grad(src, dkv[:, C:], wv, bv, True)
    return dx, dsrc, [g_wq, g_bq, g_wk, g_bk, g_wv, g_bv, g_wm, g_bm, g_w0, g_b0, g_w3, g_b3]


class _AttnPropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, src, wq, bq, wk, bk, wv, bv, wm, bm, w0, b0, w3, b3, heads, eps, nx=None, nsrc=None):
        P = (wq, bq, wk, bk, wv, bv, wm, bm, w0, b0, w3, b3)
        out, saved = _prop_fwd(x, src, P, heads, eps, nx, nsrc, keep=any(ctx.needs_input_grad))
        ctx.heads = heads
        ctx.params = P
        ctx.lens = (nx, nsrc)  # (not differentiable, never outputs: plain attributes)
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        dx, dsrc, g = _prop_bwd(ctx.saved_tensors, ctx.params, ctx.heads, dout, None, *ctx.lens)
        return (dx, dsrc, *g, None, None, None, None)


class _AttnPropPairFn(torch.autograd.Function):
    """One refinement layer's two calls (modeling/dpfm.py:101-103) as one node:
        out0 = x0 + layer(x0, x1);  out1 = x1 + layer(x1, out0)
    so each gradient that two consumers feed is summed in a launch epilogue instead of by the
    autograd engine: d out0 = g0 + (the second call's d src) in that launch's `add`, d x1 =
    (the second call's d x) + (the first call's d src) likewise. Parameter gradients: the second
    call's, then the first's, autograd's order for a layer applied twice."""

    @staticmethod
    def forward(ctx, x0, x1, wq, bq, wk, bk, wv, bv, wm, bm, w0, b0, w3, b3, heads, eps, n0=None, n1=None):
        P = (wq, bq, wk, bk, wv, bv, wm, bm, w0, b0, w3, b3)
        # masked mode: the first call's queries are x0 (n0 real points) and its keys x1 (n1); the
        # second call's are reversed
        keep = any(ctx.needs_input_grad)
        out0, s0 = _prop_fwd(x0, x1, P, heads, eps, n0, n1, keep=keep)
        out1, s1 = _prop_fwd(x1, out0, P, heads, eps, n1, n0, keep=keep)
        ctx.heads = heads
        ctx.params = P
        ctx.lens = (n0, n1)
        ctx.save_for_backward(*s0, *s1)
        return out0, out1

    @staticmethod
    def backward(ctx, g0, g1):
        sv = ctx.saved_tensors
        s0, s1 = sv[:11], sv[11:]
        n0, n1 = ctx.lens
        dx1_b, dout0, gb = _prop_bwd(s1, ctx.params, ctx.heads, g1, dsrc_add=g0, nx=n1, nsrc=n0)
        dx0, dx1, ga = _prop_bwd(s0, ctx.params, ctx.heads, dout0, dsrc_add=dx1_b, nx=n0, nsrc=n1)
        g = [b if a is None else (a if b is None else b + a) for a, b in zip(ga, gb)]
        return (dx0, dx1, *g, None, None, None, None)


def _fusable(layer, x, src) -> bool:
    attn, mlp = layer.attn, layer.mlp
    C = x.shape[1] if x.dim() == 3 else 0
    return (x.is_cuda and x.dim() == 3 and src.dim() == 3 and x.is_contiguous() and src.is_contiguous()
            and x.dtype == torch.float32 and src.dtype == torch.float32 and C in (16, 32, 64)
            and attn.dim == 16 and C == attn.dim * attn.num_heads and len(mlp) == 4
            and x.shape[0] == src.shape[0] and src.shape[1] == C
            and mlp[0].out_channels == 2 * C and mlp[3].out_channels == C)


def _params(layer):
    attn, mlp = layer.attn, layer.mlp
    pq, pk, pv = attn.proj
    return (pq.weight, pq.bias, pk.weight, pk.bias, pv.weight, pv.bias, attn.merge.weight, attn.merge.bias,
            mlp[0].weight, mlp[0].bias, mlp[3].weight, mlp[3].bias)


def attn_prop_pair(layer, x0: torch.Tensor, x1: torch.Tensor, nx=None, nsrc=None):
    """(x0', x1') = (x0 + layer(x0, x1), x1 + layer(x1, x0')) — both calls of one refinement layer
    (modeling/dpfm.py:101-103) as one fused node — or None outside the fused shapes.
    nx / nsrc (masked mode): the real points of x0 / x1, int32 [B] on the device."""
    if not (_fusable(layer, x0, x1) and _fusable(layer, x1, x0)):
        return None
    B, dev = x0.shape[0], x0.device
    return _AttnPropPairFn.apply(x0, x1, *_params(layer), layer.attn.num_heads, float(layer.mlp[1].eps),
                                 ops._lens(nx, B, dev), ops._lens(nsrc, B, dev))


def attn_prop_residual(layer, x: torch.Tensor, src: torch.Tensor, nx=None, nsrc=None) -> torch.Tensor:
    """x + layer(x, src) for a modeling.dpfm.AttentionalPropagation `layer` as one fused node, or
    None when the shapes / storage fall outside it (the caller then takes the module path).
    nx / nsrc (masked mode): the real points of x / src, int32 [B] on the device."""
    if not _fusable(layer, x, src):
        return None
    B, dev = x.shape[0], x.device
    return _AttnPropFn.apply(x, src, *_params(layer), layer.attn.num_heads, float(layer.mlp[1].eps),
                             ops._lens(nx, B, dev), ops._lens(nsrc, B, dev))
