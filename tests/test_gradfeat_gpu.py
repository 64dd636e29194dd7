"""GPU: the gradient-feature kernels (pk_grad_apply, pk_grad_apply_t, pk_gradfeat_fwd / bwd,
pk_linear192_fwd) and the modules built on them against the fp64 restatement in
tests/_gradfeat_ref.py. Shapes: 3 crops of 70 padded points with 70, 3 and 45 real ones (no full
tile anywhere, empty slots, padded rows), and a hub cloud for the transposed apply."""
import numpy as np
import pytest
import torch

import _gradfeat_ref as R

pytestmark = pytest.mark.gpu

COUNTS = (70, 3, 45)


def _operator(clouds, normals, nmax):
    """GradOperator (fp64, host) of clouds from the restatement: 30 neighbours, the given normals."""
    from dpfm_amd.geometry import GradOperator
    rows = [R.grad_rows(c, R.tangent_frames(n), R.cloud_neighbors(c, 30)) for c, n in zip(clouds, normals)]
    idx, val = R.fixed_width(rows, nmax)
    return GradOperator.build(torch.from_numpy(idx), torch.from_numpy(val), [c.shape[0] for c in clouds])


@pytest.fixture(scope="module")
def cap_op():
    clouds = [R.sphere_cap(n, 30 + n) for n in COUNTS]
    return _operator(clouds, clouds, 70)  # (a unit sphere's normals are its points)


@pytest.fixture(scope="module")
def hub_op():
    hub, cap = R.hub_ring(), R.sphere_cap(45, 5)
    return _operator([hub, cap], [np.tile(np.array([0.0, 0.0, 1.0]), (61, 1)), cap], 61)


def _apply_ref(op32, x64):
    """fp64 v = [gradX x | gradY x] and the bound's sum |val| |x| from the f32 operator's values."""
    idx = op32.idx.long().clamp(min=0)
    val = torch.where((op32.idx >= 0)[..., None], op32.val.double(), torch.zeros((), dtype=torch.float64))
    B, N, W = op32.idx.shape
    xg = torch.stack([x64[b][idx[b]] for b in range(B)])  # [B, N, W, 64]
    v = torch.cat([(val[..., c, None] * xg).sum(2) for c in range(2)], dim=-1)
    mag = torch.cat([(val[..., c, None].abs() * xg.abs()).sum(2) for c in range(2)], dim=-1)
    return v, mag


def test_grad_apply(device, cap_op):
    from dpfm_amd import ops
    op = cap_op.to(device=device, dtype=torch.float32)
    g = torch.Generator().manual_seed(0)
    wide = torch.randn(3, 70, 128, generator=g).to(device)
    x = wide[..., 64:]
    v = ops.grad_apply(x, 128, op.idx, op.val)
    v2 = ops.grad_apply(x.contiguous(), 64, op.idx, op.val)
    assert torch.equal(v, v2)  # the strided read gives the same bits as a contiguous copy
    ref, mag = _apply_ref(op.to(device="cpu"), x.cpu().double())
    err = (v.cpu().double() - ref).abs()
    print("grad_apply max err / bound", float((err / (1e-5 * mag).clamp(min=1e-30)).max()))
    assert (err <= 1e-5 * mag).all()
    for b, n in enumerate(COUNTS):
        assert (v[b, n:] == 0).all()  # padded rows are exactly 0
    assert float(v[1, :3].abs().max()) > 0


def _apply_t_ref(op32, dv64):
    """fp64 dx[b, j] = sum over (i, s) with idx[b, i, s] = j of valX dv[i, :64] + valY dv[i, 64:]
    (the dense transpose), and the bound's sum of magnitudes."""
    B, N, W = op32.idx.shape
    dx = torch.zeros((B, N, 64), dtype=torch.float64)
    mag = torch.zeros_like(dx)
    for b in range(B):
        keep = op32.idx[b] >= 0
        rows = torch.arange(N)[:, None].expand(N, W)[keep]
        dst = op32.idx[b][keep].long()
        vx, vy = op32.val[b][keep].double().unbind(-1)
        c = vx[:, None] * dv64[b, rows, :64] + vy[:, None] * dv64[b, rows, 64:]
        m = vx.abs()[:, None] * dv64[b, rows, :64].abs() + vy.abs()[:, None] * dv64[b, rows, 64:].abs()
        dx[b].index_add_(0, dst, c)
        mag[b].index_add_(0, dst, m)
    return dx, mag


@pytest.mark.parametrize("which", ["caps", "hub"])
def test_grad_apply_t(device, cap_op, hub_op, which):
    from dpfm_amd import ops
    host = cap_op if which == "caps" else hub_op
    B, N, W = host.idx.shape
    if which == "hub":  # the precondition: the centre's in-degree is twice k, the others' about k
        deg = (host.tptr[0, 1:] - host.tptr[0, :-1]).numpy() - 1  # minus the point's own slot 0
        assert deg[60] == 60 and deg[:60].max() <= 31, (deg[60], deg[:60].max())
    op = host.to(device=device, dtype=torch.float32)
    g = torch.Generator().manual_seed(1)
    dv = torch.randn(B, N, 128, generator=g).to(device)
    pre = torch.randn(B, N, 64, generator=g).to(device)
    dx = torch.empty(B, N, 64, device=device)
    ops.grad_apply_t(dv, op.tptr, op.tsrc, op.val, dx, 64)
    ref, mag = _apply_t_ref(op.to(device="cpu"), dv.cpu().double())
    err = (dx.cpu().double() - ref).abs()
    print("grad_apply_t max err / bound", float((err / (1e-5 * mag).clamp(min=1e-30)).max()))
    assert (err <= 1e-5 * mag).all()
    # accumulate adds to a prefilled dx (one more rounded add on top of the sum)
    acc = pre.clone()
    ops.grad_apply_t(dv, op.tptr, op.tsrc, op.val, acc, 64, accumulate=True)
    err = (acc.cpu().double() - (ref + pre.cpu().double())).abs()
    assert (err <= 1e-5 * (mag + pre.cpu().double().abs())).all()
    # bitwise reproducible, whatever the output held before (there is no scratch buffer)
    again = torch.full_like(dx, float("nan"))
    ops.grad_apply_t(dv, op.tptr, op.tsrc, op.val, again, 64)
    assert torch.equal(again, dx)
    # a strided destination (columns 64..127 of a wider buffer) gets the same bits
    wide = torch.full((B, N, 128), float("nan"), device=device)
    ops.grad_apply_t(dv, op.tptr, op.tsrc, op.val, wide[..., 64:], 128)
    assert torch.equal(wide[..., 64:], dx) and bool(torch.isnan(wide[..., :64]).all())


def test_linear192(device):
    """The 192-input first layer: rows read at a stride out of a wider buffer, against fp64 with
    the f32 summation bound."""
    from dpfm_amd import ops
    g = torch.Generator().manual_seed(4)
    wide = torch.randn(210, 256, generator=g).to(device)
    w = (torch.randn(64, 192, generator=g) * 0.1).to(device)
    b = torch.randn(64, generator=g).to(device)
    y = torch.empty(210, 64, device=device)
    ops.linear192_fwd(wide[:, 64:], 256, w, b, 210, True, y)
    x64, w64, b64 = wide[:, 64:].cpu().double(), w.cpu().double(), b.cpu().double()
    ref = torch.relu(x64 @ w64.t() + b64)
    mag = x64.abs() @ w64.abs().t() + b64.abs()
    assert ((y.cpu().double() - ref).abs() <= 1e-5 * mag).all()
    y2 = torch.empty_like(y)
    ops.linear192_fwd(wide[:, 64:].contiguous(), 192, w, None, 210, False, y2)
    assert ((y2.cpu().double() - x64 @ w64.t()).abs() <= 1e-5 * mag).all()


def _yardstick(truth, cpu32, gpu32, mine, floor):
    """model_parity's rule on one tensor: max |error| for outputs, within 3 x the larger error of
    the same arithmetic in f32 on the CPU and with torch on the GPU."""
    e = [(t.detach().cpu().double() - truth).abs().max().item() for t in (cpu32, gpu32, mine)]
    assert e[2] <= 3 * max(e[0], e[1]) + floor, e


def _grad_check(named_truth, grads32, gradsg, gradsm, label):
    floor = 1e-6 * torch.cat([g.reshape(-1) for _, g in named_truth]).norm().item()
    for (name, t), a, b, d in zip(named_truth, grads32, gradsg, gradsm):
        e = [(x.detach().cpu().double() - t).norm().item() for x in (a, b, d)]
        assert e[2] <= 3 * max(e[0], e[1]) + floor, (label, name, e, floor, t.norm().item())


@pytest.mark.parametrize("rotations", [True, False])
def test_spatial_gradient_features(device, rotations):
    from dpfm_amd.diffusion_net import SpatialGradientFeatures
    torch.manual_seed(3)
    mine = SpatialGradientFeatures(64, with_gradient_rotations=rotations).to(device)
    ref = R.SpatialGradientFeatures(64, rotations)
    ref.load_state_dict(mine.state_dict(), strict=True)
    truth = R.SpatialGradientFeatures(64, rotations).double()
    truth.load_state_dict(ref.state_dict())
    gref = R.SpatialGradientFeatures(64, rotations).to(device)
    gref.load_state_dict(ref.state_dict())
    v = torch.randn(3, 70, 128) * 0.7  # R = 210 rows: no 32-row tile of the last wave is full
    w = torch.randn(3, 70, 64)
    outs, dvs, wgs = [], [], []
    for m, dev, dt in ((truth, "cpu", torch.float64), (ref, "cpu", torch.float32), (gref, device, torch.float32),
                       (mine, device, torch.float32)):
        vv = v.to(device=dev, dtype=dt).detach().clone().requires_grad_(True)
        out = m(vv) if m is mine else m(vv[..., :64], vv[..., 64:])
        m.zero_grad()
        (out * w.to(device=dev, dtype=dt)).sum().backward()
        outs.append(out.detach())
        dvs.append(vv.grad)
        wgs.append([p.grad for p in m.parameters()])
    t = outs[0]
    _yardstick(t, outs[1], outs[2], outs[3], 1e-6 * (1 + t.abs().max().item()))
    named = [("dv", dvs[0])] + [(n, g) for (n, _), g in zip(truth.named_parameters(), wgs[0])]
    _grad_check(named, [dvs[1]] + wgs[1], [dvs[2]] + wgs[2], [dvs[3]] + wgs[3], f"rotations={rotations}")
    # upstream's [..., C, 2] (real, imaginary) layout of the vectors is the same input
    vd = v.to(device)
    assert torch.equal(mine(torch.stack((vd[..., :64], vd[..., 64:]), dim=-1)), mine(vd))


@pytest.fixture(scope="module")
def net_batch(device):
    """B = 2, N = 70 with 70 and 45 real points: random M-orthonormal evecs (the existing model
    tests' lbo_operators; rows past a crop's count zeroed, as get_operators pads) and the real
    gradient operators of two sphere caps from get_operators."""
    from dpfm_amd import geometry
    from dpfm_amd.dataset.synthetic import lbo_operators
    counts = (70, 45)
    clouds = [R.sphere_cap(n, 40 + n) for n in counts]
    grad = geometry.get_operators(clouds, k_eig=8, device=device).grad
    mass, evals, evecs = (np.stack(a) for a in zip(*[lbo_operators(70, 64, 7 + b) for b in range(2)]))
    mass[1, 45:] = 0.0
    evecs[1, 45:] = 0.0
    rng = np.random.default_rng(5)
    x = rng.normal(size=(2, 70, 3)).astype(np.float32)
    x[1, 45:] = 0.0
    dense = torch.zeros(2, 2, 70, 70, dtype=torch.float64)
    g32 = grad.float()  # the values the kernels read
    for b, n in enumerate(counts):
        for c, m in enumerate(g32.coo(b)):
            dense[c, b, :n, :n] = m.to_dense().double().cpu()
    return {"x": torch.from_numpy(x), "mass": torch.from_numpy(mass), "evals": torch.from_numpy(evals),
            "evecs": torch.from_numpy(evecs), "grad": g32, "gradX": dense[0], "gradY": dense[1], "counts": counts}


def test_diffusion_net_with_gradient_features(device, net_batch):
    from dpfm_amd.diffusion_net import DiffusionNet
    nb = net_batch
    torch.manual_seed(11)
    mine = DiffusionNet(3, 32, C_width=64, N_block=2, dropout=False, with_gradient_features=True).to(device)
    with torch.no_grad():
        for blk in mine.blocks:
            blk.diffusion.diffusion_time.uniform_(-0.001, 12)
    ref = R.DiffusionNet()
    ref.load_state_dict(mine.state_dict(), strict=True)
    truth = R.DiffusionNet().double()
    truth.load_state_dict(ref.state_dict())
    gref = R.DiffusionNet().to(device)
    gref.load_state_dict(ref.state_dict())
    w = torch.randn(2, 70, 32)
    keys = ("x", "mass", "evals", "evecs", "gradX", "gradY")
    outs, grads = [], []
    for m, dev, dt in ((truth, "cpu", torch.float64), (ref, "cpu", torch.float32), (gref, device, torch.float32)):
        out = m(*[nb[k].to(device=dev, dtype=dt) for k in keys])
        m.zero_grad()
        (out * w.to(device=dev, dtype=dt)).sum().backward()
        outs.append(out.detach())
        grads.append([p.grad for p in m.parameters()])
    d = {k: nb[k].to(device) for k in ("x", "mass", "evals", "evecs")}
    out = mine(d["x"], d["mass"], evals=d["evals"], evecs=d["evecs"], gradX=nb["grad"])
    mine.zero_grad()
    (out * w.to(device)).sum().backward()
    t = outs[0]
    _yardstick(t, outs[1], outs[2], out, 1e-6 * (1 + t.abs().max().item()))
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in truth.named_parameters()]
    named = [(n, g) for (n, _), g in zip(truth.named_parameters(), grads[0])]
    _grad_check(named, grads[1], grads[2], [p.grad for p in mine.parameters()], "diffusion net")
    # upstream-style input: per-crop sparse gradX / gradY lists -> the same operator, the same bits
    coos = [nb["grad"].coo(b) for b in range(2)]
    with torch.no_grad():
        a = mine(d["x"], d["mass"], evals=d["evals"], evecs=d["evecs"], gradX=nb["grad"])
        b = mine(d["x"], d["mass"], evals=d["evals"], evecs=d["evecs"], gradX=[c[0] for c in coos],
                 gradY=[c[1] for c in coos])
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        mine(d["x"], d["mass"], evals=d["evals"], evecs=d["evecs"])


def test_dpfmnet_with_gradient_features(device, net_batch):
    from dpfm_amd.models.dpfm import DPFMNet
    nb = net_batch
    shape = {"xyz": (nb["x"] * 6 + 100).to(device), "mass": nb["mass"].to(device), "evals": nb["evals"].to(device),
             "evecs": nb["evecs"].to(device)}
    batch = {"shape1": dict(shape, grad=nb["grad"]), "shape2": dict(shape, grad=nb["grad"])}
    torch.manual_seed(2)
    net = DPFMNet(with_gradient_features=True).to(device)
    out = net(batch)
    (out[0].sum() + out[1].sum() + out[3].square().sum()).backward()
    assert all(bool(torch.isfinite(o).all()) for o in out[:5])
    gf = net.feature_extractor.block_0.gradient_features
    assert gf.A_re.weight.grad is not None and float(gf.A_re.weight.grad.abs().max()) > 0
    assert float(gf.A_im.weight.grad.abs().max()) > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.feature_extractor.parameters())
    with pytest.raises(ValueError, match="grad"):
        net({"shape1": dict(shape), "shape2": dict(shape, grad=nb["grad"])})
    # the default construction is the reference configuration, bit for bit (fused encoder on)
    from dpfm_amd import diffusion_net
    assert diffusion_net.FUSED_ENCODER
    a = DPFMNet().to(device)
    b = DPFMNet(with_gradient_features=False).to(device)
    b.load_state_dict(a.state_dict(), strict=True)
    plain = {"shape1": dict(shape), "shape2": dict(shape)}
    with torch.no_grad():
        for x, y in zip(a(plain), b(plain)):
            assert torch.equal(x, y)
