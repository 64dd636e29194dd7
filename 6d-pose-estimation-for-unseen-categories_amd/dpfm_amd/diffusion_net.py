"""Spectral DiffusionNet encoder — the DPFM point encoder (H7).

Mirrors upstream diffusion-net `layers.py` as vendored by the DPFM submodule (imported at
models/dpfm.py:11, built at models/dpfm.py:22-30 with C_in=3, C_out=32, C_width=64,
N_block=2, dropout=False, with_gradient_features=False): same module and parameter
names as weights/weights.pt (`first_lin`, `block_{i}.diffusion.diffusion_time`,
`block_{i}.mlp.miniMLP_mlp_layer_{000,001,002}`, `last_lin`).

The diffusion step (to_basis -> exp(-lambda t) -> from_basis) runs in one fused HIP kernel
per direction (ops.spectral_diffusion); the per-point MLPs are GEMMs.

with_gradient_features=True (upstream's default, off in the reference configuration) adds
SpatialGradientFeatures to every block: the spatial gradient of the diffused features through the
fixed-width gradient operator (geometry.GradOperator; ops.grad_apply), a learned complex rotation
and the tanh of the per-channel inner product (ops.gradfeat_fwd), concatenated as a third 64-wide
input of the block MLP. Such a network runs the module path (not _EncoderFn).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import ops
from .layers import Linear
from .wgrad import direct_grad, weight_grad

# The whole configured DiffusionNet as one autograd node (_EncoderFn); False runs the per-module
# path (the parity tests compare the two)
FUSED_ENCODER = True

# _EncoderFn runs each block's MLP as one launch per direction (ops.mlp3_fwd / ops.mlp3_bwd,
# bit-identical to the three per-layer launches); False (PK_BLOCK_MLP_CHAIN=0 at import) runs the
# per-layer launches — the A/B partner and the tests' reference; "fwd" / "bwd" chain one direction
# only (the measurements of each direction alone)
BLOCK_MLP_CHAIN = {"0": False, "fwd": "fwd", "bwd": "bwd"}.get(os.environ.get("PK_BLOCK_MLP_CHAIN", "1"), True)


def _chain(direction: str) -> bool:
    return BLOCK_MLP_CHAIN is True or BLOCK_MLP_CHAIN == direction


class LearnedTimeDiffusion(nn.Module):
    def __init__(self, C_inout: int, method: str = "spectral"):
        super().__init__()
        if method != "spectral":
            raise ValueError("only spectral diffusion is on the hot path (models/dpfm.py:22-30)")
        self.C_inout = C_inout
        self.diffusion_time = nn.Parameter(torch.zeros(C_inout))

    def forward(self, x, L, mass, evals, evecs):
        # upstream clamps diffusion_time in place (clamp_(min=1e-8)) before
        # every diffusion; the spectral kernel applies and writes back that clamp itself (same
        # storage, so HIP-graph replays see it), saving a launch per block
        return ops.spectral_diffusion(x, mass, evals, evecs, self.diffusion_time, clamp_t=True)


class MiniMLP(nn.Sequential):
    def __init__(self, layer_sizes, dropout=False, activation=nn.ReLU, name="miniMLP"):
        super().__init__()
        for i in range(len(layer_sizes) - 1):
            if dropout and i > 0:
                self.add_module(name + "_mlp_layer_dropout_{:03d}".format(i), nn.Dropout(p=0.5))
            lin = Linear(layer_sizes[i], layer_sizes[i + 1])
            self.add_module(name + "_mlp_layer_{:03d}".format(i), lin)
            if i + 2 != len(layer_sizes):
                if activation is nn.ReLU:  # fused into the layer's epilogue (same module names)
                    lin.relu_out = True
                    self.add_module(name + "_mlp_act_{:03d}".format(i), nn.Identity())
                else:
                    self.add_module(name + "_mlp_act_{:03d}".format(i), activation())


class _BlockMLPFn(torch.autograd.Function):
    """mlp(cat[x_in, x_diffuse]) + x_in for the configured MiniMLP (128 -> 64 -> 64 -> 64, ReLU
    between): one launch per direction (ops.mlp3_fwd / ops.mlp3_bwd: the activations stay in the
    wave between the layers, the ReLU masks on the saved h1 / h2 and the residual are epilogues),
    and the weight gradients recorded for the grouped launch (wgrad.GroupedWgrad) or computed
    per layer."""

    @staticmethod
    def forward(ctx, x_in, x_diff, w1, b1, w2, b2, w3, b3):
        x_in, x_diff = x_in.contiguous(), x_diff.contiguous()
        R = x_in.numel() // 64
        w1, w2, w3 = w1.contiguous(), w2.contiguous(), w3.contiguous()
        h1 = torch.empty_like(x_in)
        h2 = torch.empty_like(x_in)
        y = torch.empty_like(x_in)
        ops.mlp3_fwd(x_in, x_diff, w1, b1, w2, b2, w3, b3, R, y, h1=h1, h2=h2)
        ctx.save_for_backward(x_in, x_diff, h1, h2, w1, w2, w3)
        ctx.params = (w1, b1, w2, b2, w3, b3)
        return y

    @staticmethod
    def backward(ctx, dy):
        x_in, x_diff, h1, h2, w1, w2, w3 = ctx.saved_tensors
        p1, b1, p2, b2, p3, b3 = ctx.params
        dy = dy.contiguous()
        d2, d1, dx_in, dx_diff = (torch.empty_like(dy) for _ in range(4))
        ops.mlp3_bwd(dy, h2, h1, w3, w2, w1, dy.numel() // 64, d2, d1, dx_in, dx_diff)
        g3 = weight_grad(h2, dy, p3, b3, False)
        g2 = weight_grad(h1, d2, p2, b2, False)
        cat = torch.cat((x_in, x_diff), dim=-1)  # (the module path: not the training step's)
        g1 = weight_grad(cat, d1, p1, b1, False)
        return (dx_in, dx_diff, *g1, *g2, *g3)


class SpatialGradientFeatures(nn.Module):
    """Upstream layers.SpatialGradientFeatures: from the spatial gradient (vX, vY) of each channel,
    B = A v as a complex product (with_gradient_rotations: B_re = A_re vX - A_im vY, B_im = A_re vY +
    A_im vX; else B_re = A vX, B_im = A vY; bias-free [C, C] layers under upstream's names) and the
    feature tanh(vX . B_re + vY . B_im). forward takes upstream's [..., C, 2] (real, imaginary)
    vectors or the kernels' packed [..., 2C] = [vX | vY]; one launch per direction (C = 64)."""

    def __init__(self, C_inout, with_gradient_rotations=True):
        super().__init__()
        self.C_inout = C_inout
        self.with_gradient_rotations = with_gradient_rotations
        if with_gradient_rotations:
            self.A_re = nn.Linear(C_inout, C_inout, bias=False)
            self.A_im = nn.Linear(C_inout, C_inout, bias=False)
        else:
            self.A = nn.Linear(C_inout, C_inout, bias=False)

    def weights(self):
        """(A_re, A_im) or (A, None): the kernels' weight operands."""
        if self.with_gradient_rotations:
            return self.A_re.weight, self.A_im.weight
        return self.A.weight, None

    def forward(self, vectors):
        C = self.C_inout
        if vectors.dim() >= 3 and vectors.shape[-1] == 2 and vectors.shape[-2] == C:
            vectors = torch.cat((vectors[..., 0], vectors[..., 1]), dim=-1)
        if C != 64 or vectors.shape[-1] != 128 or vectors.dtype != torch.float32:
            raise ops._lib.PoseKernError("gradient features kernels are built for f32, C_width = 64")
        return ops._GradFeatFn.apply(vectors, *self.weights())


class _Linear192Fn(torch.autograd.Function):
    """relu(cat W^T + b) for the 192-input first MLP layer of a block with gradient features
    (pk_linear192_fwd: pk_linear_ex stops at 128 inputs). Backward: the ReLU mask, the input
    gradient as two transposed products written side by side into one [R, 192] buffer (columns
    0..127 and 128..191), the weight gradient as two pk_linear_wgrad column blocks."""

    @staticmethod
    def forward(ctx, cat, weight, bias):
        cat = cat.contiguous()
        w = weight.contiguous()
        R = cat.numel() // 192
        y = torch.empty(cat.shape[:-1] + (64,), dtype=torch.float32, device=cat.device)
        ops.linear192_fwd(cat, 192, w, bias, R, True, y)
        ctx.save_for_backward(cat, w, y)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        cat, w, y = ctx.saved_tensors
        R = cat.numel() // 192
        dy = torch.ops.aten.threshold_backward(dy.contiguous(), y, 0.0)
        dcat = torch.empty_like(cat)
        ops.linear_ex(dy, w[:, :128].contiguous(), None, 0, R, 0, 64, 128, y=dcat, ldy=192, transw=True)
        ops.linear_ex(dy, w[:, 128:].contiguous(), None, 0, R, 0, 64, 64, y=dcat[..., 128:], ldy=192, transw=True)
        dw0, db = ops.linear_wgrad(cat[..., :128], dy, channels_first=False, want_bias=ctx.has_bias)
        dw1, _ = ops.linear_wgrad(cat[..., 128:], dy, channels_first=False, want_bias=False)
        return dcat, torch.cat((dw0, dw1), dim=1), db


class DiffusionNetBlock(nn.Module):
    def __init__(self, C_width, mlp_hidden_dims, dropout=False, diffusion_method="spectral",
                 with_gradient_features=False, with_gradient_rotations=True):
        super().__init__()
        self.C_width = C_width
        self.with_gradient_features = with_gradient_features
        self.diffusion = LearnedTimeDiffusion(C_width, method=diffusion_method)
        self.MLP_C = 2 * C_width
        if with_gradient_features:
            self.gradient_features = SpatialGradientFeatures(C_width, with_gradient_rotations=with_gradient_rotations)
            self.MLP_C += C_width
        self.mlp = MiniMLP([self.MLP_C] + list(mlp_hidden_dims) + [C_width], dropout=dropout)

    # The module path's own block node (_BlockMLPFn on pk_mlp3_fwd / pk_mlp3_bwd) is opt-in: the
    # configured network runs as _EncoderFn, which uses the same kernels in place (BLOCK_MLP_CHAIN)
    fused_mlp = False

    def _fusable(self, x_in) -> bool:
        lins = [m for m in self.mlp if isinstance(m, Linear)]
        return (self.fused_mlp and x_in.is_cuda and len(lins) == 3 and self.C_width == 64 and len(self.mlp) == 5
                and all(l.relu_out for l in lins[:2]) and not lins[2].relu_out
                and all(l.bias is not None for l in lins)
                and [tuple(l.weight.shape) for l in lins] == [(64, 128), (64, 64), (64, 64)])

    def _forward_grad(self, x_in, x_diffuse, grad):
        """mlp(cat[x_in, x_diffuse, g]) + x_in, g = the gradient features of x_diffuse on the
        GradOperator `grad`: the concatenation is one [B, N, 192] buffer the gradient kernels read
        and write in place (ops._GradCatFn), the 192-input layer its own launch (_Linear192Fn)."""
        mods = list(self.mlp)
        if (grad is None or self.C_width != 64 or not isinstance(mods[0], Linear) or not mods[0].relu_out
                or tuple(mods[0].weight.shape) != (64, 192) or x_in.dtype != torch.float32):
            if grad is None:
                raise ValueError("a DiffusionNet with gradient features needs gradX (a geometry.GradOperator, or "
                                 "per-crop sparse gradX / gradY)")
            raise ops._lib.PoseKernError("gradient features kernels are built for f32, C_width = 64 and a ReLU MLP")
        cat = ops._GradCatFn.apply(x_in.contiguous(), x_diffuse.contiguous(), grad.idx, grad.val, grad.tptr,
                                   grad.tsrc, *self.gradient_features.weights())
        h = _Linear192Fn.apply(cat, mods[0].weight, mods[0].bias)
        for m in mods[1:]:
            h = m(h)
        return h + x_in

    def forward(self, x_in, mass, L, evals, evecs, gradX, gradY):
        x_diffuse = self.diffusion(x_in, L, mass, evals, evecs)
        if self.with_gradient_features:
            return self._forward_grad(x_in, x_diffuse, gradX)
        if self._fusable(x_in):  # the configured block: one fused forward launch
            l0, l1, l2 = [m for m in self.mlp if isinstance(m, Linear)]
            return _BlockMLPFn.apply(x_in, x_diffuse, l0.weight, l0.bias, l1.weight, l1.bias, l2.weight, l2.bias)
        return self.mlp(torch.cat((x_in, x_diffuse), dim=-1)) + x_in


class _EncoderFn(torch.autograd.Function):
    """The configured DiffusionNet (first_lin 3 -> 64, N_block blocks of spectral diffusion +
    MLP 128 -> 64 -> 64 -> 64 with ReLUs and the residual, last_lin 64 -> C_out) over rows
    [R, C] as one autograd node with a hand-written backward, so no concatenation, residual
    add, slice copy or gradient accumulation runs as a separate launch:
      forward : block i works in one [R, 128] buffer CAT_i: x_in in columns 0..63 (written
                there by its producer: first_lin or block i-1's last layer, whose residual add
                is its epilogue), the diffusion writes x_diffuse into columns 64..127;
      backward: the first MLP layer's input gradient is split in its epilogue into dX (columns
                0..63, plus the residual's dy) and dD (64..127); the diffusion backward of dD
                accumulates into dX, which is the previous layer's output gradient.
    Same arithmetic per layer as the module path (models/dpfm.py:22-30; upstream layers.py)."""

    @staticmethod
    def forward(ctx, fcat, mass, evals, evecs, nblock, save, *params):
        R = fcat.shape[0] * fcat.shape[1]
        B, N = fcat.shape[0], fcat.shape[1]
        dev = fcat.device
        w0, b0 = params[0], params[1]
        wl, bl = params[-2], params[-1]
        blocks = [params[2 + 7 * i: 9 + 7 * i] for i in range(nblock)]
        Cout = wl.shape[0]
        cats = [torch.empty((B, N, 128), dtype=torch.float32, device=dev) for _ in range(nblock)]
        ops.linear_ex(fcat, w0, b0, 0, R, 0, fcat.shape[-1], 64, y=cats[0], ldy=128)
        h1s, h2s, raws = [], [], []
        Y = torch.empty((B, N, 64), dtype=torch.float32, device=dev)
        for i, (t, w1, b1, w2, b2, w3, b3) in enumerate(blocks):
            cat = cats[i]
            raws.append(ops.spectral_raw(cat, 128, mass, evals, evecs, t, True, 0, cat[..., 64:], 128))
            nxt = cats[i + 1] if i + 1 < nblock else Y
            ldy = 128 if i + 1 < nblock else 0
            if _chain("fwd") and not save:  # save: grad mode at the call; off, h1 / h2 are not stored
                ops.mlp3_fwd(cat, cat[..., 64:], w1, b1, w2, b2, w3, b3, R, nxt, ld_in=128, ld_diff=128, ldy=ldy)
                continue
            h1 = torch.empty((B, N, 64), dtype=torch.float32, device=dev)
            h2 = torch.empty_like(h1)
            if _chain("fwd"):
                ops.mlp3_fwd(cat, cat[..., 64:], w1, b1, w2, b2, w3, b3, R, nxt, ld_in=128, ld_diff=128, ldy=ldy,
                             h1=h1, h2=h2)
            else:
                ops.linear_ex(cat, w1, b1, 0, R, 0, 128, 64, y=h1, relu=True)
                ops.linear_ex(h1, w2, b2, 0, R, 0, 64, 64, y=h2, relu=True)
                ops.linear_ex(h2, w3, b3, 0, R, 0, 64, 64, y=nxt, ldy=ldy, add=cat, lda=128, add_cols=64)
            h1s.append(h1)
            h2s.append(h2)
        feat = torch.empty((B, N, Cout), dtype=torch.float32, device=dev)
        ops.linear_ex(Y, wl, bl, 0, R, 0, 64, Cout, y=feat)
        ctx.nblock = nblock
        ctx.save_for_backward(fcat, mass, evals, evecs, Y, *cats, *h1s, *h2s, *raws, *params)
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        nb = ctx.nblock
        sv = ctx.saved_tensors
        fcat, mass, evals, evecs, Y = sv[:5]
        cats = sv[5:5 + nb]
        h1s = sv[5 + nb:5 + 2 * nb]
        h2s = sv[5 + 2 * nb:5 + 3 * nb]
        raws = sv[5 + 3 * nb:5 + 4 * nb]
        params = sv[5 + 4 * nb:]
        w0, b0, wl, bl = params[0], params[1], params[-2], params[-1]
        blocks = [params[2 + 7 * i: 9 + 7 * i] for i in range(nb)]
        B, N = fcat.shape[0], fcat.shape[1]
        R = B * N
        dev = fcat.device
        dfeat = dfeat.contiguous()
        Cout = wl.shape[0]
        grads = [None] * len(params)
        grads[-2], grads[-1] = weight_grad(Y, dfeat, wl, bl, False)
        dy = torch.empty((B, N, 64), dtype=torch.float32, device=dev)
        ops.linear_ex(dfeat, wl, None, 0, R, 0, Cout, 64, y=dy, transw=True)
        for i in reversed(range(nb)):
            t, w1, b1, w2, b2, w3, b3 = blocks[i]
            k = 2 + 7 * i
            grads[k + 5], grads[k + 6] = weight_grad(h2s[i], dy, w3, b3, False)
            d2 = torch.empty_like(dy)
            d1 = torch.empty_like(dy)
            dX = torch.empty_like(dy)
            dD = torch.empty_like(dy)
            chain = _chain("bwd")
            if chain:  # the three input-gradient layers below as one launch
                ops.mlp3_bwd(dy, h2s[i], h1s[i], w3, w2, w1, R, d2, d1, dX, dD)
            else:
                ops.linear_ex(dy, w3, None, 0, R, 0, 64, 64, y=d2, transw=True, mask=h2s[i])
            grads[k + 3], grads[k + 4] = weight_grad(h1s[i], d2, w2, b2, False)
            if not chain:
                ops.linear_ex(d2, w2, None, 0, R, 0, 64, 64, y=d1, transw=True, mask=h1s[i])
            grads[k + 1], grads[k + 2] = weight_grad(cats[i], d1, w1, b1, False)
            if not chain:
                # dcat = d1 W1: columns 0..63 (+ the residual's dy) -> dX, 64..127 -> dD
                ops.linear_ex(d1, w1, None, 0, R, 0, 64, 128, y=dX, transw=True, y2=dD, split=64, add=dy, add_cols=64)
            # dL/dt straight into t's persistent .grad when the grouped weight gradient owns it (no
            # autograd accumulation launch)
            gbuf = direct_grad(t)
            gt = gbuf if gbuf is not None else torch.empty((64,), dtype=torch.float32, device=dev)
            ops.spectral_raw(dD, 64, mass, evals, evecs, t, True, 1, dX, 64, saved=raws[i], gt=gt, accumulate=True)
            grads[k] = None if gbuf is not None else gt
            dy = dX
        grads[0], grads[1] = weight_grad(fcat, dy, w0, b0, False)
        dfcat = None
        if ctx.needs_input_grad[0]:  # the features are data in DPFM; kept for API completeness
            dfcat = torch.empty_like(fcat)
            ops.linear_ex(dy, w0, None, 0, R, 0, 64, fcat.shape[-1], y=dfcat, transw=True)
        return (dfcat, None, None, None, None, None, *grads)


class DiffusionNet(nn.Module):
    def __init__(self, C_in, C_out, C_width=128, N_block=4, last_activation=None, outputs_at="vertices",
                 mlp_hidden_dims=None, dropout=True, with_gradient_features=True, with_gradient_rotations=True,
                 diffusion_method="spectral"):
        super().__init__()
        if outputs_at != "vertices":
            raise ValueError("DPFM reads features at vertices")
        self.C_in, self.C_out, self.C_width, self.N_block = C_in, C_out, C_width, N_block
        self.last_activation = last_activation
        if mlp_hidden_dims is None:
            mlp_hidden_dims = [C_width, C_width]
        self.first_lin = Linear(C_in, C_width)
        self.last_lin = Linear(C_width, C_out)
        self.blocks = []
        for i_block in range(N_block):
            blk = DiffusionNetBlock(C_width, mlp_hidden_dims, dropout=dropout, diffusion_method=diffusion_method,
                                    with_gradient_features=with_gradient_features,
                                    with_gradient_rotations=with_gradient_rotations)
            self.blocks.append(blk)
            self.add_module("block_" + str(i_block), blk)

    def _fused_params(self, x_in):
        """The parameter list of _EncoderFn when this is the configured network, else None."""
        if any(b.with_gradient_features for b in self.blocks):
            return None  # gradient features run the module path
        if not (x_in.is_cuda and x_in.dtype == torch.float32 and self.C_width == 64 and self.last_activation is None
                and self.first_lin.in_features <= 4 and self.last_lin.out_features in (16, 32, 64)):
            return None
        ps = [self.first_lin.weight, self.first_lin.bias]
        for b in self.blocks:
            lins = [m for m in b.mlp if isinstance(m, Linear)]
            if (len(b.mlp) != 5 or len(lins) != 3 or [tuple(l.weight.shape) for l in lins] != [(64, 128), (64, 64), (64, 64)]
                    or not (lins[0].relu_out and lins[1].relu_out and not lins[2].relu_out)
                    or any(l.bias is None for l in lins) or b.diffusion.diffusion_time.shape != (64,)):
                return None
            ps += [b.diffusion.diffusion_time, lins[0].weight, lins[0].bias, lins[1].weight, lins[1].bias,
                   lins[2].weight, lins[2].bias]
        ps += [self.last_lin.weight, self.last_lin.bias]
        if any(p is None for p in ps):
            return None
        return ps

    @staticmethod
    def _grad_operator(gradX, gradY, x_in):
        from .geometry import GradOperator
        if not isinstance(gradX, GradOperator):
            if torch.is_tensor(gradX):
                gradX, gradY = [gradX], [gradY]
            gradX = GradOperator.from_coo(list(gradX), list(gradY), nmax=x_in.shape[1])
        if gradX.val.dtype != torch.float32 or gradX.val.device != x_in.device:
            gradX = gradX.to(device=x_in.device, dtype=torch.float32)
        if gradX.idx.shape[1] != x_in.shape[1]:
            raise ValueError(f"gradX covers {gradX.idx.shape[1]} points per crop, x_in has {x_in.shape[1]}")
        return gradX

    def forward(self, x_in, mass, L=None, evals=None, evecs=None, gradX=None, gradY=None, edges=None, faces=None):
        """gradX: a geometry.GradOperator (val f32, on x_in's device), or — upstream-style batches —
        gradX / gradY as per-crop lists of sparse [n, n] tensors (one sparse tensor each for a single
        unbatched shape), converted with GradOperator.from_coo. Read only with gradient features."""
        appended = x_in.dim() == 2
        if appended:
            x_in, mass, evals, evecs = x_in[None], mass[None], evals[None], evecs[None]
        if gradX is not None and any(b.with_gradient_features for b in self.blocks):
            gradX = self._grad_operator(gradX, gradY, x_in)
        ps = self._fused_params(x_in) if evecs is not None and evecs.shape[-1] == 64 else None
        if ps is not None and FUSED_ENCODER:
            x = _EncoderFn.apply(x_in.contiguous(), mass.contiguous(), evals.contiguous(), evecs.contiguous(),
                                 len(self.blocks), torch.is_grad_enabled(), *ps)
            return x[0] if appended else x
        x = self.first_lin(x_in)
        for b in self.blocks:
            x = b(x, mass, L, evals, evecs, gradX, gradY)
        x = self.last_lin(x)
        if self.last_activation is not None:
            x = self.last_activation(x)
        return x[0] if appended else x
