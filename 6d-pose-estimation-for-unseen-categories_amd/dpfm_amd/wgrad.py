"""Where every hand-written backward gets a per-point layer's weight gradient from.

A backward calls `weight_grad` for each (x, dy) product of a layer, and `direct_grad` for a
parameter whose whole gradient one of its kernels can write itself. With no recorder active
(module-level training, the tests' eager steps) `weight_grad` launches pk_linear_wgrad and
returns the gradients to autograd. Between `GroupedWgrad.begin()` and `end()` (TrainStep's
backward) the calls on the recorder's parameters are recorded instead and run as one grouped
launch pair at `end()`, which writes the parameters' persistent .grad buffers.

A node whose layer the recorder owns MUST take that layer's gradient through `weight_grad`:
`end()` zeroes the buffer of every owned parameter no call named, as "not used by this forward".
A node that launches ops.linear_wgrad itself and returns the result to autograd would have it
added to .grad before `end()` and then zeroed. `diffusion_net._Linear192Fn` (the 192-input layer
of a block with gradient features) is such a node: it is safe only because a gradient-features
model is never handed to TrainStep(grouped=True).
"""
from __future__ import annotations

import torch

from . import ops

_ACTIVE = None  # the GroupedWgrad between its begin() and end() (TrainStep's backward), or None


class GroupedWgrad:
    """Weight gradients of all per-point layers of one backward in two launches.

    Each layer's backward records (x, dy) instead of launching pk_linear_wgrad (two
    launches per layer, 56 per training step, each too small to fill the chip) and returns
    None for its weight / bias so autograd leaves their .grad alone. `end()` issues one
    grouped pk_linear_wgrad_grouped on the same stream, writing into persistent .grad
    buffers; a weight used twice in the forward (the refinement layer, modeling/dpfm.py:
    100-104; first/last_lin on both shapes) accumulates in autograd's order. Everything
    stays on one stream: a single-stream HIP graph replays without cross-queue
    dependencies (a forked side stream measured slower on MI355X)."""

    def __init__(self, params, bufs=None, direct_params=()):
        """params: the per-point layers' weights / biases (gradients from the grouped launch);
        direct_params: parameters whose gradient a kernel may write whole through direct() (the
        diffusion times under the fused encoder) and that otherwise get autograd's ordinary
        accumulation (the non-fused encoder path) — never zeroed by end()."""
        self.params = [p for p in params]
        self.direct_params = [p for p in direct_params]
        self.direct_ids = {id(p) for p in self.direct_params}
        self.caller_bufs = bufs is not None
        # persistent .grad buffers (optionally the caller's, e.g. views of one flat buffer the
        # caller zeroes before each backward)
        self.bufs = {id(p): (bufs[id(p)] if bufs is not None else
                             torch.zeros_like(p, memory_format=torch.contiguous_format))
                     for p in self.params + self.direct_params}
        self.seen = set()
        self.calls = []

    def begin(self):
        global _ACTIVE
        for p in self.params:
            p.grad = self.bufs[id(p)]
        for p in self.direct_params:
            # autograd accumulates into .grad when no kernel writes it whole: start it from zero
            # (a caller's flat buffer is already zeroed; an own buffer holds the last step's value)
            if not self.caller_bufs:
                self.bufs[id(p)].zero_()
            p.grad = self.bufs[id(p)]
        self.seen = set()
        self.calls = []
        _ACTIVE = self

    def owns(self, p) -> bool:
        return id(p) in self.bufs

    def direct(self, p):
        """p's persistent .grad buffer for a kernel that writes p's whole gradient itself (e.g. the
        diffusion-time gradient of pk_spectral_diffusion's backward), on p's first use in this
        backward; None otherwise (the caller then returns the gradient to autograd)."""
        if id(p) not in self.bufs or id(p) in self.seen:
            return None
        self.seen.add(id(p))
        return self.bufs[id(p)]

    def launch(self, x, dy, weight, bias, channels_first: bool):
        acc = id(weight) in self.seen
        self.seen.add(id(weight))
        if bias is not None:
            self.seen.add(id(bias))
        dw = self.bufs[id(weight)]
        db = self.bufs[id(bias)] if bias is not None else None
        self.calls.append((x, dy, channels_first, dw.view(dw.shape[0], -1), db, acc))

    @staticmethod
    def _groupable(c) -> bool:
        x, dy, cf, dw, _, _ = c
        O, I = dw.shape
        return ((O + 31) // 32) * ((I + 31) // 32) <= 8

    def end(self, run: bool = True):
        global _ACTIVE
        _ACTIVE = None
        if run:
            if all(self._groupable(c) for c in self.calls):
                ops.linear_wgrad_grouped(self.calls)
            else:  # a shape outside the grouped kernel's range: one launch pair per call, in order
                for x, dy, cf, dw, db, acc in self.calls:
                    ops.linear_wgrad(x, dy, channels_first=cf, want_bias=db is not None, dw=dw, db=db,
                                     accumulate=acc)
            for p in self.params:  # a layer the forward did not use gets a zero gradient
                if id(p) not in self.seen:
                    p.grad.zero_()
            # (direct_params: written by direct(), or accumulated by autograd into the zeroed buffer)
        self.calls = []


def weight_grad(x, dy, weight, bias, channels_first: bool, acc=None):
    """(dW viewed as weight's shape, db or None) of one (x, dy) product of the layer (weight, bias).
    When the active recorder owns the layer the product is recorded for its grouped launch and
    nothing is computed: `acc` comes back as given ((None, None) without one). `acc`, the
    (dW, db) of the layer's earlier products in this node, is added to: acc + new."""
    side = _ACTIVE
    if side is not None and side.owns(weight) and (bias is None or side.owns(bias)):
        side.launch(x, dy, weight, bias, channels_first=channels_first)
        return (None, None) if acc is None else acc
    dw, db = ops.linear_wgrad(x, dy, channels_first=channels_first, want_bias=bias is not None)
    dw = dw.view(weight.shape)
    if acc is None:
        return dw, db
    return acc[0] + dw, (acc[1] + db if db is not None else acc[1])


def direct_grad(param):
    """param's persistent .grad buffer for a kernel that writes param's whole gradient itself, on
    its first use in the recorded backward (GroupedWgrad.direct); None otherwise: the caller then
    returns the gradient to autograd."""
    return _ACTIVE.direct(param) if _ACTIVE is not None else None
