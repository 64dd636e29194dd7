"""GPU: the DiffusionNet block MLP as one launch per direction (pk_mlp3_fwd / pk_mlp3_bwd) against
the three per-layer pk_linear_ex launches of _EncoderFn (diffusion_net.BLOCK_MLP_CHAIN off) on the
same buffers: every tensor the chain writes is bit-equal (the same MFMA chains in the same order)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (R, max_blocks): below one tile, one full tile, 4 x 700 (ragged last tile, many blocks), and 21
# tiles on one block (5-6 tiles per wave: more than the ring is deep, ragged last tile)
CASES = [(7, 0), (16, 0), (2800, 0), (329, 1)]
SENTINEL = -12345.0


@functools.lru_cache(maxsize=None)
def _weights():
    g = torch.Generator().manual_seed(21)

    def u(*shape, fan_in):
        return (torch.rand(*shape, generator=g) * 2 - 1) / fan_in ** 0.5

    return (u(64, 128, fan_in=128), u(64, fan_in=128), u(64, 64, fan_in=64), u(64, fan_in=64),
            u(64, 64, fan_in=64), u(64, fan_in=64))


@functools.lru_cache(maxsize=None)
def _reference(R):
    """Inputs and the per-layer path's outputs for R rows, computed once (read-only afterwards):
    forward h1, h2, y (contiguous) and backward d2, d1, dX, dD for a seeded dy, with the masks h1 /
    h2 from that real ReLU forward (exact zeros where the pre-activation was negative)."""
    from dpfm_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(100 + R)
    cat = torch.randn(R, 128, generator=g).to(dev)
    dy = torch.randn(R, 64, generator=g).to(dev)
    w1, b1, w2, b2, w3, b3 = (t.to(dev) for t in _weights())
    h1, h2, y, d2, d1, dX, dD = (torch.empty(R, 64, device=dev) for _ in range(7))
    ops.linear_ex(cat, w1, b1, 0, R, 0, 128, 64, y=h1, relu=True)
    ops.linear_ex(h1, w2, b2, 0, R, 0, 64, 64, y=h2, relu=True)
    ops.linear_ex(h2, w3, b3, 0, R, 0, 64, 64, y=y, add=cat, lda=128, add_cols=64)
    ops.linear_ex(dy, w3, None, 0, R, 0, 64, 64, y=d2, transw=True, mask=h2)
    ops.linear_ex(d2, w2, None, 0, R, 0, 64, 64, y=d1, transw=True, mask=h1)
    ops.linear_ex(d1, w1, None, 0, R, 0, 64, 128, y=dX, transw=True, y2=dD, split=64, add=dy, add_cols=64)
    torch.cuda.synchronize()
    return dict(cat=cat, dy=dy, W=(w1, b1, w2, b2, w3, b3), h1=h1, h2=h2, y=y, d2=d2, d1=d1, dX=dX, dD=dD)


@pytest.mark.parametrize("R,max_blocks", CASES)
@pytest.mark.parametrize("one_buffer", [True, False])
@pytest.mark.parametrize("strided_y", [True, False])
def test_chain_forward_matches_layers(device, R, max_blocks, one_buffer, strided_y):
    from dpfm_amd import ops
    ref = _reference(R)
    assert (ref["h1"] == 0).any() and (ref["h2"] == 0).any()  # the ReLUs cut something
    cat = ref["cat"]
    if one_buffer:
        xi, xd, ld = cat, cat[:, 64:], 128
    else:
        xi, xd, ld = cat[:, :64].contiguous(), cat[:, 64:].contiguous(), 0
    h1, h2 = torch.empty(R, 64, device=device), torch.empty(R, 64, device=device)
    ybuf = torch.full((R, 128 if strided_y else 64), SENTINEL, device=device)
    ops.mlp3_fwd(xi, xd, *ref["W"], R, ybuf, ld_in=ld, ld_diff=ld, ldy=128 if strided_y else 0, h1=h1, h2=h2,
                 max_blocks=max_blocks)
    assert torch.equal(h1, ref["h1"]) and torch.equal(h2, ref["h2"])
    assert torch.equal(ybuf[:, :64], ref["y"])
    if strided_y:
        assert (ybuf[:, 64:] == SENTINEL).all()
    # no-grad variant: h1 / h2 not stored, the same y
    y2 = torch.full_like(ybuf, SENTINEL)
    ops.mlp3_fwd(xi, xd, *ref["W"], R, y2, ld_in=ld, ld_diff=ld, ldy=128 if strided_y else 0, max_blocks=max_blocks)
    assert torch.equal(y2, ybuf)


@pytest.mark.parametrize("R,max_blocks", CASES)
def test_chain_backward_matches_layers(device, R, max_blocks):
    from dpfm_amd import ops
    ref = _reference(R)
    w1, _, w2, _, w3, _ = ref["W"]
    d2, d1, dX, dD = (torch.full((R, 64), SENTINEL, device=device) for _ in range(4))
    ops.mlp3_bwd(ref["dy"], ref["h2"], ref["h1"], w3, w2, w1, R, d2, d1, dX, dD, max_blocks=max_blocks)
    assert (ref["d2"] == 0).any() and (ref["d1"] == 0).any()  # the masks cut something
    for name, got in (("d2", d2), ("d1", d1), ("dX", dX), ("dD", dD)):
        assert torch.equal(got, ref[name]), name


def test_chain_empty_is_ok(device):
    from dpfm_amd import ops
    e = torch.empty(0, 64, device=device)
    W = tuple(t.to(device) for t in _weights())
    ops.mlp3_fwd(e, e, *W, 0, e, h1=e, h2=e)
    ops.mlp3_bwd(e, e, e, W[4], W[2], W[0], 0, e, e, e, e)


def test_chain_forward_against_fp64(device):
    """The chain forward at R = 2,800 against the same three layers in float64 on the CPU, within
    1e-5 of the output's scale (the bound test_block_mlp_fused_matches_layers uses for this MLP)."""
    from dpfm_amd import ops
    R = 2800
    ref = _reference(R)
    y = torch.empty(R, 64, device=device)
    ops.mlp3_fwd(ref["cat"], ref["cat"][:, 64:], *ref["W"], R, y, ld_in=128, ld_diff=128)
    cat = ref["cat"].cpu().double()
    w1, b1, w2, b2, w3, b3 = (t.double() for t in _weights())
    h = torch.relu(torch.relu(cat @ w1.t() + b1) @ w2.t() + b2)
    y64 = h @ w3.t() + b3 + cat[:, :64]
    err = (y.cpu().double() - y64).abs().max().item()
    print(f"chain forward vs fp64: max abs err {err:.3e}, scale {y64.abs().max().item():.3e}")
    assert err <= 1e-5 * y64.abs().max().item() + 1e-12


def test_encoder_chain_matches_per_layer(device, monkeypatch):
    """The configured DiffusionNet (as _EncoderFn) with BLOCK_MLP_CHAIN on vs off: output, input
    gradient and every parameter gradient bit-equal, through a plain .backward() (per-layer weight
    gradients, no grouped launch); the no-grad forward (h1 / h2 not stored) gives the same output."""
    from dpfm_amd import diffusion_net as DN
    torch.manual_seed(5)
    net = DN.DiffusionNet(C_in=3, C_out=32, C_width=64, N_block=2, dropout=False,
                          with_gradient_features=False).to(device)
    g = torch.Generator().manual_seed(8)
    B, N = 2, 300
    x = torch.randn(B, N, 3, generator=g).to(device)
    mass = (torch.rand(B, N, generator=g) * 1e-3 + 1e-4).to(device)
    evals = torch.sort(torch.rand(B, 64, generator=g) * 2, dim=1)[0].to(device)
    evecs = (torch.randn(B, N, 64, generator=g) * 0.1).to(device)
    dy = torch.randn(B, N, 32, generator=g).to(device)
    assert net._fused_params(x) is not None and DN.FUSED_ENCODER
    res = {}
    for chain in (True, False):
        monkeypatch.setattr(DN, "BLOCK_MLP_CHAIN", chain)
        net.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        y = net(xi, mass, evals=evals, evecs=evecs)
        y.backward(dy)
        with torch.no_grad():
            y0 = net(x, mass, evals=evals, evecs=evecs)
        assert torch.equal(y0, y.detach())
        res[chain] = [y.detach(), xi.grad.clone()] + [p.grad.clone() for p in net.parameters()]
    assert all(t is not None for t in res[True])
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
