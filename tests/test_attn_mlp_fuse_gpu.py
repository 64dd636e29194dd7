"""GPU: the MLP around the cross-attention as three fused launches (pk_attn_mlp_fwd: copy + merge +
mlp.0 + InstanceNorm/ReLU; pk_attn_mlp_bwd_norm: mlp.3^T + the norm backward; pk_attn_mlp_bwd_in:
mlp.0^T + merge^T) against the per-layer launches of attnprop (ATTN_MLP_FUSE off) on the same
buffers: every tensor the fused kernels write is bit-equal (the same MFMA chains and the same
row sums in the same order)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 32
EPS = 1e-5
SENTINEL = -12345.0
# rows of the norm: below one wave row (16), a ragged point tile in the second wave row (80), the
# ragged PER = 16 variant (513), the flagship row (1024: 32-/64-point vector tiles, PER = 16) and the
# longest supported row (2048, PER = 32); B = 3 exercises the crop stride
NS = [16, 80, 513, 1024, 2048]
BS = [1, 3]
ZERO_CH = 37  # mlp.0 output channel with zero weight and bias: a constant h1 row


@functools.lru_cache(maxsize=None)
def _weights():
    g = torch.Generator().manual_seed(31)

    def u(*shape, fan_in):
        return (torch.rand(*shape, generator=g) * 2 - 1) / fan_in ** 0.5

    wm, bm = u(C, C, fan_in=C), u(C, fan_in=C)
    w0, b0 = u(2 * C, 2 * C, fan_in=2 * C), u(2 * C, fan_in=2 * C)
    w3 = u(C, 2 * C, fan_in=2 * C)
    w0[ZERO_CH] = 0.
    b0[ZERO_CH] = 0.
    return wm, bm, w0, b0, w3


@functools.lru_cache(maxsize=None)
def _reference(B, N):
    """Inputs and the per-layer launches' outputs for B crops of N points, computed once (read-only
    afterwards): forward hc, h1, h1n, mean, invstd; backward dh1, dhc, da for a seeded dout and the
    h1 / mean / invstd of that forward."""
    from dpfm_amd import _lib, ops
    from dpfm_amd._lib import call, ptr
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * B + N)
    x = torch.randn(B, C, N, generator=g).to(dev)
    a = torch.randn(B, C, N, generator=g).to(dev)
    dout = torch.randn(B, C, N, generator=g).to(dev)
    wm, bm, w0, b0, w3 = (t.to(dev) for t in _weights())
    st = _lib.stream(dev)
    hc, h1, h1n, dh1n, dh1, dhc = (torch.empty(B, 2 * C, N, device=dev) for _ in range(6))
    mean, invstd = torch.empty(B * 2 * C, device=dev), torch.empty(B * 2 * C, device=dev)
    da = torch.empty(B, C, N, device=dev)
    call("pk_copy_rows", ptr(hc), 2 * C * N, ptr(x), C * N, B, C * N, st)
    ops.linear_ex(a, wm, bm, 1, B * N, N, C, C, y=hc[:, C:], ldy=2 * C * N)
    ops.linear_ex(hc, w0, b0, 1, B * N, N, 2 * C, 2 * C, y=h1)
    call("pk_instnorm_relu_fwd", ptr(h1), B * 2 * C, N, EPS, ptr(h1n), ptr(mean), ptr(invstd), st)
    ops.linear_ex(dout, w3, None, 1, B * N, N, C, 2 * C, y=dh1n, transw=True)
    call("pk_instnorm_relu_bwd", ptr(h1), ptr(dh1n), ptr(mean), ptr(invstd), B * 2 * C, N, ptr(dh1), st)
    ops.linear_ex(dh1, w0, None, 1, B * N, N, 2 * C, 2 * C, y=dhc, transw=True)
    ops.linear_ex(dhc[:, C:], wm, None, 1, B * N, N, C, C, y=da, transw=True, ldx=2 * C * N)
    torch.cuda.synchronize()
    return dict(x=x, a=a, dout=dout, W=(wm, bm, w0, b0, w3), hc=hc, h1=h1, h1n=h1n, mean=mean, invstd=invstd,
                dh1=dh1, dhc=dhc, da=da)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_fused_forward_matches_layers(device, B, N):
    from dpfm_amd import ops
    ref = _reference(B, N)
    wm, bm, w0, b0, _ = ref["W"]
    assert (ref["h1n"] == 0).any() and (ref["h1n"] > 0).any()  # the ReLU cuts something, not everything
    hc, h1, h1n = (torch.full((B, 2 * C, N), SENTINEL, device=device) for _ in range(3))
    mean, invstd = (torch.full((B * 2 * C,), SENTINEL, device=device) for _ in range(2))
    ops.attn_mlp_fwd(ref["x"], ref["a"], wm, bm, w0, b0, EPS, h1n, mean, invstd, hc=hc, h1=h1)
    for name, got in (("hc", hc), ("h1", h1), ("h1n", h1n), ("mean", mean), ("invstd", invstd)):
        assert torch.equal(got, ref[name]), name
    # the constant row: var = 0, invstd = 1 / sqrt(eps), finite and bit-equal
    rows = torch.arange(B, device=device) * 2 * C + ZERO_CH
    assert torch.isfinite(invstd).all() and torch.isfinite(h1n).all()
    assert torch.equal(invstd[rows], ref["invstd"][rows]) and (mean[rows] == 0).all()
    assert ((invstd[rows] - EPS ** -0.5).abs() <= 1e-6 * EPS ** -0.5).all()
    assert (h1n[:, ZERO_CH] == 0).all()
    # no-grad variant: hc / h1 not stored (null pointers), the same h1n and statistics
    h1n2 = torch.full((B, 2 * C, N), SENTINEL, device=device)
    mean2, invstd2 = (torch.full((B * 2 * C,), SENTINEL, device=device) for _ in range(2))
    ops.attn_mlp_fwd(ref["x"], ref["a"], wm, bm, w0, b0, EPS, h1n2, mean2, invstd2)
    assert torch.equal(h1n2, ref["h1n"]) and torch.equal(mean2, ref["mean"]) and torch.equal(invstd2, ref["invstd"])
    # one of the two only: the other buffer is written exactly as before
    hc3, h13 = (torch.full((B, 2 * C, N), SENTINEL, device=device) for _ in range(2))
    ops.attn_mlp_fwd(ref["x"], ref["a"], wm, bm, w0, b0, EPS, h1n2, mean2, invstd2, hc=hc3)
    ops.attn_mlp_fwd(ref["x"], ref["a"], wm, bm, w0, b0, EPS, h1n2, mean2, invstd2, h1=h13)
    assert torch.equal(hc3, ref["hc"]) and torch.equal(h13, ref["h1"]) and torch.equal(h1n2, ref["h1n"])


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_fused_backward_matches_layers(device, B, N):
    from dpfm_amd import ops
    ref = _reference(B, N)
    wm, _, w0, _, w3 = ref["W"]
    dh1, dhc = (torch.full((B, 2 * C, N), SENTINEL, device=device) for _ in range(2))
    da = torch.full((B, C, N), SENTINEL, device=device)
    ops.attn_mlp_bwd_norm(ref["dout"], w3, ref["h1"], ref["mean"], ref["invstd"], dh1)
    assert torch.equal(dh1, ref["dh1"])
    ops.attn_mlp_bwd_in(dh1, w0, wm, dhc, da)
    assert torch.equal(dhc, ref["dhc"]) and torch.equal(da, ref["da"])
    assert torch.isfinite(dh1).all()


def _params(device, seed):
    """The 12 parameters of an AttentionalPropagation layer (Conv1d(k=1) shapes), seeded."""
    g = torch.Generator().manual_seed(seed)

    def u(*shape, fan_in):
        return ((torch.rand(*shape, generator=g) * 2 - 1) / fan_in ** 0.5).to(device).requires_grad_(True)

    P = []
    for _ in range(4):  # q, k, v projections and the merge
        P += [u(C, C, 1, fan_in=C), u(C, fan_in=C)]
    P += [u(2 * C, 2 * C, 1, fan_in=2 * C), u(2 * C, fan_in=2 * C), u(C, 2 * C, 1, fan_in=2 * C), u(C, fan_in=2 * C)]
    return P


def _pair_run(device, monkeypatch, mode, N1, N2, B=2):
    """_AttnPropPairFn forward + backward with ATTN_MLP_FUSE = mode; returns (tensors, launch names)."""
    from dpfm_amd import _lib, attnprop
    monkeypatch.setattr(attnprop, "ATTN_MLP_FUSE", mode)
    g = torch.Generator().manual_seed(77)
    x0 = torch.randn(B, C, N1, generator=g).to(device).requires_grad_(True)
    x1 = torch.randn(B, C, N2, generator=g).to(device).requires_grad_(True)
    g0, g1 = torch.randn(B, C, N1, generator=g).to(device), torch.randn(B, C, N2, generator=g).to(device)
    P = _params(device, 78)
    names = []

    def probe(name, thunk, work):
        names.append(name)
        return thunk()

    _lib.set_probe(probe)
    try:
        o0, o1 = attnprop._AttnPropPairFn.apply(x0, x1, *P, 2, EPS)
        torch.autograd.backward([o0, o1], [g0, g1])
        with torch.no_grad():
            n0, n1 = attnprop._AttnPropPairFn.apply(x0, x1, *P, 2, EPS)
    finally:
        _lib.set_probe(None)
    assert torch.equal(n0, o0) and torch.equal(n1, o1)  # hc / h1 not stored: the same outputs
    assert all(p.grad is not None for p in P)
    return [o0.detach(), o1.detach(), x0.grad, x1.grad] + [p.grad for p in P], names


def test_pair_node_fused_matches_per_layer(device, monkeypatch):
    """_AttnPropPairFn at N1 = 80, N2 = 48 with the switch on (and each single direction) against
    off: both outputs, both input gradients and all 12 parameter gradients bit-equal."""
    ref, names_off = _pair_run(device, monkeypatch, False, 80, 48)
    assert not any(n.startswith("pk_attn_mlp") for n in names_off)
    assert names_off.count("pk_instnorm_relu_fwd") == 4 and names_off.count("pk_instnorm_relu_bwd") == 2
    for mode in (True, "fwd", "bwd"):
        got, names = _pair_run(device, monkeypatch, mode, 80, 48)
        # two calls per forward (one with grad, one without), two per backward
        assert names.count("pk_attn_mlp_fwd") == (4 if mode in (True, "fwd") else 0), mode
        assert names.count("pk_attn_mlp_bwd_norm") == names.count("pk_attn_mlp_bwd_in") == \
            (2 if mode in (True, "bwd") else 0), mode
        assert ("pk_instnorm_relu_fwd" in names) == (mode == "bwd") and \
            ("pk_instnorm_relu_bwd" in names) == (mode == "fwd"), mode
        assert len(got) == len(ref) == 16
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), (mode, i)


def test_rows_above_the_maximum_take_the_per_layer_launches(device, monkeypatch):
    """One point more than the longest supported row: the node falls back to the per-layer
    launches (and still matches the fused path's arithmetic on the shorter shape, which takes the
    fused launches); the entry points themselves refuse the shape."""
    from dpfm_amd import _lib, ops
    N = ops.ATTN_MLP_MAX_N + 1
    _, names = _pair_run(device, monkeypatch, True, N, 2048, B=1)
    # the first call's rows are N long (fallback), the second call's 2048 (fused): per forward one
    # of each, and the node ran twice forward, once backward
    assert names.count("pk_attn_mlp_fwd") == 2 and names.count("pk_instnorm_relu_fwd") == 2
    assert names.count("pk_attn_mlp_bwd_norm") == 1 and names.count("pk_attn_mlp_bwd_in") == 1
    assert names.count("pk_instnorm_relu_bwd") == 1
    wm, bm, w0, b0, w3 = (t.to(device) for t in _weights())
    x = torch.zeros(1, C, N, device=device)
    h = torch.zeros(1, 2 * C, N, device=device)
    s = torch.zeros(2 * C, device=device)
    with pytest.raises(_lib.PoseKernError):
        ops.attn_mlp_fwd(x, x, wm, bm, w0, b0, EPS, h, s, s)
    with pytest.raises(_lib.PoseKernError):
        ops.attn_mlp_bwd_norm(x, w3, h, s, s, h)


def test_empty_batch_is_ok(device):
    from dpfm_amd import ops
    wm, bm, w0, b0, w3 = (t.to(device) for t in _weights())
    x, h, s = torch.empty(0, C, 64, device=device), torch.empty(0, 2 * C, 64, device=device), torch.empty(0, device=device)
    ops.attn_mlp_fwd(x, x, wm, bm, w0, b0, EPS, h, s, s, hc=h, h1=h)
    ops.attn_mlp_bwd_norm(x, w3, h, s, s, h)
    ops.attn_mlp_bwd_in(h, w0, wm, h, x)
