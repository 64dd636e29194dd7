"""Pins tests/_nce_ref.py (the reference test_nce_edges_gpu.py holds pk_nce_loss to) on the CPU:
both fp64 variants against autograd through the oracle's nce_loss, the conventions on degenerate
inputs (d == 0, a zero-norm row, an empty crop), and the conditioning of the input families of
_nce_ref (Gaussian, converging positives, degenerate rows): the fp32 yardstick's own error against
the fp64 truth stays under a stated cap, so that a GPU bound of 3 x yardstick + floor on them can
never go vacuous."""
import pytest
import torch

import _nce_ref as R
from oracle import dpfm_model_oracle as M

F64 = torch.float64


def _close(a, b, tol):
    assert (a - b).abs().max().item() <= tol * (1 + b.abs().max().item())


@pytest.mark.parametrize("S", [1, 5, 64])
def test_matches_oracle_autograd(S):
    c = R.gaussian_crop(S, 40, 50, 7 + S)
    r1, r2 = c["f1"].double().requires_grad_(), c["f2"].double().requires_grad_()
    pairs = torch.stack([c["i1"], c["i2"]], 1)
    ref = M.nce_loss(r1, r2, pairs, torch.arange(S))
    ref.backward()
    for mm in (False, True):
        loss, g1, g2 = R.nce(c["f1"], c["f2"], c["i1"], c["i2"], mm=mm)
        assert loss.dtype == F64
        _close(loss, ref.detach(), 1e-10)
        _close(g1, r1.grad, 1e-10)
        _close(g2, r2.grad, 1e-10)


def test_prenorm_matches_autograd():
    """prenorm: the features are used as they are and the gradients are with respect to them."""
    c = R.gaussian_crop(33, 40, 50, 3)
    u1 = torch.nn.functional.normalize(c["f1"], dim=1)
    u2 = torch.nn.functional.normalize(c["f2"], dim=1)
    r1, r2 = u1.double().requires_grad_(), u2.double().requires_grad_()
    logits = -torch.cdist(r1[c["i1"]], r2[c["i2"]]) / 0.07
    ref = torch.nn.functional.cross_entropy(logits, torch.arange(33))
    ref.backward()
    for mm in (False, True):
        loss, g1, g2 = R.nce(u1, u2, c["i1"], c["i2"], mm=mm, prenorm=True)
        _close(loss, ref.detach(), 1e-10)
        _close(g1, r1.grad, 1e-10)
        _close(g2, r2.grad, 1e-10)


def test_empty_crop():
    c = R.gaussian_crop(4, 6, 7, 1)
    e = torch.zeros(0, dtype=torch.int64)
    loss, g1, g2 = R.nce(c["f1"], c["f2"], e, e)
    assert float(loss) == 0.0 and g1.shape == (6, 32) and g2.shape == (7, 32)
    assert not g1.any() and not g2.any()


@pytest.mark.parametrize("dtype,mm", [(torch.float64, False), (torch.float64, True), (torch.float32, True)])
def test_degenerate_conventions(dtype, mm):
    """A bitwise equal pair: d == 0 there, in the product form too, and the entry contributes
    nothing. A zero-norm row: normalized to 0, its gradient is dv / 1e-12. All finite."""
    c = R.gaussian_crop(6, 6, 6, 2)
    f1, f2 = c["f1"].clone(), c["f2"].clone()
    i1, i2 = torch.arange(6), torch.arange(6)
    f2[0] = f1[0]   # slot 0: q == k bit for bit
    f1[1] = 0.0     # slot 1: a zero-norm CAD row
    loss, g1, g2 = R.nce(f1, f2, i1, i2, dtype=dtype, mm=mm)
    assert torch.isfinite(loss) and torch.isfinite(g1).all() and torch.isfinite(g2).all()
    # the zero row: q = 0, dq = -R k (q sum r vanishes), gradient dq / 1e-12
    v2 = torch.nn.functional.normalize(f2.to(dtype), dim=1)
    v1 = torch.nn.functional.normalize(f1.to(dtype), dim=1)
    d = torch.cdist(v1, v2, compute_mode="donot_use_mm_for_euclid_dist")
    assert float(d[0, 0]) == 0.0
    P = torch.softmax(-d / 0.07, dim=1)
    r = -(P - torch.eye(6, dtype=dtype)) / (6 * 0.07 * torch.where(d > 0, d, torch.ones_like(d)))
    r[0, 0] = 0.0
    tol = 1e-10 if dtype == torch.float64 else 1e-4
    _close(g1[1] * 1e-12, -(r[1] @ v2), tol)
    assert g1[1].abs().max() > 1e9
    # the d == 0 entry contributes nothing: slot 0's query gradient is the sum over the other keys
    dq0 = v1[0] * (r[0].sum()) - r[0] @ v2
    n0 = f1[0].to(dtype).norm()
    _close(g1[0], (dq0 - v1[0] * (v1[0] @ dq0)) / n0, tol)
    # against autograd in fp64 (norm's subgradient at 0 is 0, clamp passes dv / eps)
    if dtype == torch.float64:
        r1, r2 = f1.double().requires_grad_(), f2.double().requires_grad_()
        q, k = torch.nn.functional.normalize(r1, dim=1), torch.nn.functional.normalize(r2, dim=1)
        lg = -torch.cdist(q, k, compute_mode="donot_use_mm_for_euclid_dist") / 0.07
        torch.nn.functional.cross_entropy(lg, torch.arange(6)).backward()
        _close(g1, r1.grad, 1e-10)
        _close(g2, r2.grad, 1e-10)


@pytest.mark.parametrize("name", R.FAMILIES)
def test_family_is_conditioned(name):
    """The yardstick (mm = True, fp32, CPU) against the truth (mm = False, fp64), per crop: loss
    relative error and scale-free gradient errors (Frobenius and worst row) under the family's cap.
    A family that misses its cap needs other inputs, not another cap."""
    crops, truth, yard = R.reference(name)
    cap = R.CAPS.get(name, R.CAP_DEFAULT)
    for b, (c, tr, ya) in enumerate(zip(crops, truth, yard)):
        assert torch.isfinite(ya[0]) and torch.isfinite(ya[1]).all() and torch.isfinite(ya[2]).all()
        if name in ("gaussian", "degenerate"):
            assert 0.1 < float(tr[0]) < 10  # the loss stays O(1) there
        e = R.rel_error(ya, tr, c["f1"], c["f2"])
        print(f"nce yardstick {name} crop {b}: loss {float(tr[0]):.4f}, error {e:.2e} (cap {cap:.0e})")
        assert 0 < e <= cap
